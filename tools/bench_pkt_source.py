"""Times the packet-source column on one GPU: C4 (C3 + 10k Services x 10 Endpoints) as it is, C4 in a
gpc_config.packet_source context whose batches carry the `source` column but whose Service image
holds no short-circuit Service (the column is never loaded), and C4 with a share of its Services
external with externalTrafficPolicy: Local (both groups installed, the column loaded by the Service
stage of every packet).

    python tools/bench_pkt_source.py [--packets N] [--steps K] [--warmup W] [--rounds R]
                                     [--short-circuit-frac F]

The three rows classify the same packets: the generator's C4 batch plus a `source` column mixing POD,
GATEWAY, UPLINK and TUNNEL (the first row's batch has none). Per row: gpc_classify over N packets
with per-rule counters on, HIP events around every step, every shape warmed up first, rounds
alternating between the rows; prints one JSON line per round and row (ms per step, Mpps, the mean ms
per launch kind from gpc_launch_times), whether the first two rows' verdicts and LB results are
byte-identical, the short-circuit share of the third row's packets, and a closing line with the
ratios of the medians. bench.py stays the flagship yardstick; this only measures the new path."""
import argparse
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
    ap.add_argument("--short-circuit-frac", type=float, default=0.2)
    args = ap.parse_args()

    import torch
    from antrea_amd import gpc, workload
    from antrea_amd.build import build
    build()
    dev = torch.device("cuda", 0)
    n = args.packets

    def setup(name, packet_source, frac):
        t0 = time.time()
        wl = workload.add_services(workload.config3(), 10000, 10, short_circuit_frac=frac)
        clf = gpc.Classifier(packet_source=packet_source)
        clf.initialize()
        clf.batch_install_policy_rule_flows(wl.rules)
        workload.install_services(clf, wl)
        clf.commit()
        print("# %s: built in %.1f s, %d short-circuit Services" % (
            name, time.time() - t0, sum(1 for s in wl.services if s.get("is_external") and s.get("traffic_policy_local"))),
            file=sys.stderr, flush=True)
        return {"name": name, "clf": clf, "wl": wl, "out": torch.zeros(2 * n * 8, dtype=torch.uint8, device=dev),
                "lb": torch.zeros(n * 16, dtype=torch.uint8, device=dev)}

    ws = [setup("C4", 0, 0.0), setup("C4+source", 1, 0.0), setup("C4sc", 1, args.short_circuit_frac)]
    cols = workload.gen_packets_torch(ws[2]["wl"], n, seed=workload.PKT_SEED, device=dev)  # (the column is drawn last)
    ws[1]["soa"] = ws[2]["soa"] = gpc.pkt_soa_device(cols)
    ws[0]["soa"] = gpc.pkt_soa_device({k: v for k, v in cols.items() if k != "source"})

    def run(w, steps, timed, lb=False):
        clf = w["clf"]
        if timed:
            clf.set_launch_timing(steps)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        torch.cuda.synchronize()
        for a, b in ev:
            a.record()
            clf.classify_device(w["soa"], n, w["out"].data_ptr(), count=True, lb_ptr=w["lb"].data_ptr() if lb else 0)
            b.record()
        torch.cuda.synchronize()
        if not timed:
            return None
        ms = [a.elapsed_time(b) for a, b in ev]
        kinds = {k: round(v["mean_ms"], 4) for k, v in clf.launch_times().items() if v["launches"]}
        clf.set_launch_timing(0)
        return {"workload": w["name"], "packets": n, "steps": steps, "ms_per_step": round(statistics.mean(ms), 4),
                "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                "mpps": round(n / statistics.mean(ms) / 1e3, 1), "launch_ms": kinds}

    for w in ws:  # the LB results once, then every shape warm
        run(w, 1, False, lb=True)
        run(w, args.warmup, False)
    same = bool(torch.equal(ws[0]["out"], ws[1]["out"]) and torch.equal(ws[0]["lb"], ws[1]["lb"]))
    print(json.dumps({"C4_and_C4+source_outputs_identical": same}), flush=True)
    flags = ws[2]["lb"].view(n, 16)[:, 6]
    print(json.dumps({"workload": "C4sc", "hit_frac": round(float((flags & 1).ne(0).float().mean()), 4),
                      "short_circuit_frac_of_packets": round(float((flags & 0x40).ne(0).float().mean()), 4),
                      "no_endpoint_frac_of_packets": round(float((flags & 0x2).ne(0).float().mean()), 4)}), flush=True)
    res = {w["name"]: [] for w in ws}
    for _ in range(args.rounds):
        for w in ws:
            r = run(w, args.steps, True)
            res[w["name"]].append(r["ms_per_step"])
            print(json.dumps(r), flush=True)
    med = {k: statistics.median(v) for k, v in res.items()}
    print(json.dumps({"median_ms_per_step": med, "C4+source_over_C4": round(med["C4+source"] / med["C4"], 4),
                      "C4sc_over_C4": round(med["C4sc"] / med["C4"], 4)}), flush=True)
    if not same:
        sys.exit("the column alone changed the results")


if __name__ == "__main__":
    main()
