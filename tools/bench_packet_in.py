"""Times the packet-in collection on one GPU: C3 with per-rule counters on, as four rows --

    plain       gpc_classify_on (no queue)
    queue       gpc_classify_pin_on in the same context: no packet-in flow installed, so the three
                collection launches run over verdicts that yield nothing (their floor)
    logged1%    gpc_classify_pin_on, 1 % of the rules installed with enable_logging
    denytrack   gpc_classify_pin_on in a context with enable_deny_tracking (every ACNP Drop stores the deny)

    python tools/bench_packet_in.py [--packets N] [--steps K] [--warmup W] [--rounds R] [--policies P]

Every row classifies the same packets. Per row: HIP events around every step, every shape warmed up
first, rounds alternating between the rows; prints one JSON line per round and row (ms per step,
Mpps, the mean ms per launch kind from gpc_launch_times -- "pin_count", "pin_scan" and "pin_scatter"
among them -- and the batch's record count), whether the verdicts of "plain" and "queue" are
byte-identical, and a closing line with the ratios of the medians and the bytes the three passes
move (16 B per packet of verdicts read once, 1/4 B per packet of masks written and read, 16 B per
record and its verdict read again). bench.py stays the flagship yardstick; this only measures the new path."""
import argparse
import copy
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1 << 24)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--policies", type=int, default=500)  # C3: policies per direction (x 100 rules)
    args = ap.parse_args()

    import torch
    from antrea_amd import gpc, workload
    from antrea_amd.build import build
    build()
    dev = torch.device("cuda", 0)
    n = args.packets
    wl = workload.config3(n_policies_per_dir=args.policies)

    def context(name, logged_every=0, **kw):
        t0 = time.time()
        rules = copy.deepcopy(wl.rules)
        if logged_every:
            for r in rules[::logged_every]:
                r["enable_logging"] = True
        clf = gpc.Classifier(**kw)
        clf.initialize()
        clf.batch_install_policy_rule_flows(rules)
        clf.commit()
        print("# %s: %d rules built in %.1f s, packet-in image %d words" % (name, len(rules), time.time() - t0,
                                                                          clf.debug_pin_image()[1]), file=sys.stderr, flush=True)
        return clf

    base = context("plain / queue")
    sb = gpc.Classifier.pin_scratch_bytes(n)

    def row(name, clf, queue):
        w = {"name": name, "clf": clf, "out": torch.zeros(2 * n * 8, dtype=torch.uint8, device=dev), "queue": None}
        if queue:
            w["records"] = torch.zeros(2 * n * 16, dtype=torch.uint8, device=dev)  # room for every record
            w["count"] = torch.zeros(1, dtype=torch.int64, device=dev)
            w["scratch"] = torch.zeros(sb, dtype=torch.uint8, device=dev)
            w["queue"] = gpc.gpc_pin_queue(records=w["records"].data_ptr(), cap=2 * n, count=w["count"].data_ptr(),
                                           scratch=w["scratch"].data_ptr(), scratch_bytes=sb)
        return w

    ws = [row("plain", base, False), row("queue", base, True), row("logged1%", context("logged1%", logged_every=100), True),
          row("denytrack", context("denytrack", enable_deny_tracking=True), True)]
    cols = workload.gen_packets_torch(wl, n, seed=workload.PKT_SEED, device=dev)
    soa = gpc.pkt_soa_device(cols)

    def run(w, steps, timed):
        clf = w["clf"]
        if timed:
            clf.set_launch_timing(steps)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        torch.cuda.synchronize()
        for a, b in ev:
            a.record()
            if w["queue"] is None:
                clf.classify_device(soa, n, w["out"].data_ptr(), count=True)
            else:
                clf.classify_pin_device(soa, n, w["out"].data_ptr(), w["queue"], count=True)
            b.record()
        torch.cuda.synchronize()
        if not timed:
            return None
        ms = [a.elapsed_time(b) for a, b in ev]
        kinds = {k: round(v["mean_ms"], 4) for k, v in clf.launch_times().items() if v["launches"]}
        clf.set_launch_timing(0)
        return {"workload": w["name"], "packets": n, "steps": steps, "ms_per_step": round(statistics.mean(ms), 4),
                "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "mpps": round(n / statistics.mean(ms) / 1e3, 1),
                "launch_ms": kinds, "records": int(w["count"].item()) if w["queue"] is not None else None}

    for w in ws:
        run(w, args.warmup, False)
    same = bool(torch.equal(ws[0]["out"], ws[1]["out"]))
    print(json.dumps({"plain_and_queue_verdicts_identical": same}), flush=True)
    res = {w["name"]: [] for w in ws}
    last = {}
    for _ in range(args.rounds):
        for w in ws:
            r = run(w, args.steps, True)
            res[w["name"]].append(r["ms_per_step"])
            last[w["name"]] = r
            print(json.dumps(r), flush=True)
    med = {k: statistics.median(v) for k, v in res.items()}
    out = {"median_ms_per_step": med}
    for name in ("queue", "logged1%", "denytrack"):
        r = last[name]
        pin_ms = sum(r["launch_ms"].get(k, 0.0) for k in ("pin_count", "pin_scan", "pin_scatter"))
        moved = 16 * n + 2 * (n // 4) + 32 * r["records"]
        out[name] = {"over_plain": round(med[name] / med["plain"], 4), "pin_ms": round(pin_ms, 4), "records": r["records"],
                     "bytes_moved": moved, "gb_per_s": round(moved / max(pin_ms, 1e-9) / 1e6, 1)}
    print(json.dumps(out), flush=True)
    if not same:
        sys.exit("the queue changed the verdicts")


if __name__ == "__main__":
    main()
