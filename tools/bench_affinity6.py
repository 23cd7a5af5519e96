"""Times the IPv6 session-affinity path on one GPU: C4 (C3 + 10k Services x 10 Endpoints) embedded in
IPv6 as it is, C4v6 in a context with an IPv6 affinity table but no affinity Service, and C4v6 with a
share of its Services under sessionAffinity: ClientIP in steady state (a warm-up batch has learned,
the timed batches hit).

    python tools/bench_affinity6.py [--packets N] [--steps K] [--warmup W] [--rounds R]
                                    [--affinity-frac F] [--table-log2 L] [--clients C] [--embed 96|multi48]

The three rows classify the same packets: the generator's C4 batch with its sources folded onto
`--clients` addresses (tools/bench_affinity.py), embedded in IPv6. Per row: gpc_classify6 over N
packets with per-rule counters on, HIP events around every step, every shape warmed up first, rounds
alternating between the rows; prints one JSON line per round and row (ms per step, Mpps, the mean ms
per launch kind from gpc_launch_times, "aff6_learn" / "aff6_resolve" / "aff6_sweep" among them),
whether the first two rows' verdicts and LB results are byte-identical and their launch kinds the
same, the table's counters, and a closing line with the ratios of the medians. bench.py stays the
flagship yardstick; this only measures the new path."""
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
    ap.add_argument("--affinity-frac", type=float, default=0.3)
    ap.add_argument("--affinity-timeout", type=int, default=10800)  # the Kubernetes default, seconds
    ap.add_argument("--table-log2", type=int, default=23)
    ap.add_argument("--clients", type=int, default=1 << 16)
    ap.add_argument("--embed", default="96", choices=("96", "multi48"))
    args = ap.parse_args()

    import torch
    from antrea_amd import gpc, workload
    from antrea_amd.build import build
    build()
    dev = torch.device("cuda", 0)
    n = args.packets

    def setup(name, log2, frac):
        t0 = time.time()
        wl = workload.add_services(workload.config3(), 10000, 10, affinity_frac=frac, affinity_timeout=args.affinity_timeout)
        w6 = workload.services_to_ipv6(wl, args.embed)
        clf = gpc.Classifier(ipv4=False, ipv6=True, session_affinity6=log2)
        clf.initialize()
        clf.batch_install_policy_rule_flows(w6.rules)
        workload.install_services(clf, w6)
        clf.commit()
        clf.set_affinity_clock(1000)
        print("# %s: built in %.1f s, %d affinity Services" % (name, time.time() - t0,
                                                                sum(1 for s in w6.services if s.get("affinity_timeout"))),
              file=sys.stderr, flush=True)
        return {"name": name, "clf": clf, "wl": wl, "out": torch.zeros(2 * n * 8, dtype=torch.uint8, device=dev),
                "lb": torch.zeros(n * 32, dtype=torch.uint8, device=dev)}

    ws = [setup("C4v6", 0, 0.0), setup("C4v6+table", args.table_log2, 0.0), setup("C4v6aff", args.table_log2, args.affinity_frac)]
    cols4 = workload.gen_packets_torch(ws[0]["wl"], n, seed=workload.PKT_SEED, device=dev)  # (the same for all three)
    pool = cols4["src"][:args.clients].view(torch.int32).clone()  # (the same bits: indexing wants a signed type)
    cols4["src"] = pool[torch.randint(0, len(pool), (n,), device=dev, generator=torch.Generator(device=dev).manual_seed(7))]
    cols = workload.packets_to_v6_torch(cols4, embed=args.embed)  # (C4 has no NodePort Services: no virtual IP)
    del cols4
    soa = gpc.pkt_soa_device(cols)

    def run(w, steps, timed, lb=False):
        clf = w["clf"]
        if timed:
            clf.set_launch_timing(steps)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        torch.cuda.synchronize()
        for a, b in ev:
            a.record()
            clf.classify6_lb_device(soa, n, w["out"].data_ptr(), w["lb"].data_ptr() if lb else 0, count=True)
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

    for w in ws:  # the LB results once (and the affinity row's learning batch), then every shape warm
        run(w, 1, False, lb=True)
        run(w, args.warmup, False)
    same = bool(torch.equal(ws[0]["out"], ws[1]["out"]) and torch.equal(ws[0]["lb"], ws[1]["lb"]))
    flags = ws[2]["lb"].view(n, 32)[:, 18]
    print(json.dumps({"workload": "C4v6aff", "hit_frac": round(float((flags & 1).ne(0).float().mean()), 4),
                      "affinity_frac_of_packets": round(float((flags & 0x10).ne(0).float().mean()), 4),
                      "learned_in_first_batch": int((flags & 0x20).ne(0).sum()),
                      "table": ws[2]["clf"].affinity_stats6()}), flush=True)
    res = {w["name"]: [] for w in ws}
    kinds = {w["name"]: set() for w in ws}
    for _ in range(args.rounds):
        for w in ws:
            r = run(w, args.steps, True)
            res[w["name"]].append(r["ms_per_step"])
            kinds[w["name"]] |= set(r["launch_ms"])
            print(json.dumps(r), flush=True)
    same_launches = kinds["C4v6"] == kinds["C4v6+table"]
    print(json.dumps({"C4v6_and_C4v6+table_outputs_identical": same, "launch_kinds_identical": same_launches,
                      "launch_kinds": sorted(kinds["C4v6+table"])}), flush=True)
    print(json.dumps({"workload": "C4v6aff", "table_after": ws[2]["clf"].affinity_stats6()}), flush=True)
    med = {k: statistics.median(v) for k, v in res.items()}
    print(json.dumps({"median_ms_per_step": med, "C4v6+table_over_C4v6": round(med["C4v6+table"] / med["C4v6"], 4),
                      "C4v6aff_over_C4v6": round(med["C4v6aff"] / med["C4v6"], 4)}), flush=True)
    if not (same and same_launches):
        sys.exit("the table alone changed the results or the launches")


if __name__ == "__main__":
    main()
