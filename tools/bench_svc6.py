"""Times the IPv6 AntreaProxy path: C4 (C3 + 10k Services x 10 Endpoints) embedded in IPv6, beside
C3 embedded in IPv6 on the same build, alternating, on one GPU.

    python tools/bench_svc6.py [--packets N] [--steps K] [--warmup W] [--rounds R] [--embed 96|multi48]

Per workload: gpc_classify6 over N packets with per-rule counters on, HIP events around every step,
every shape warmed up first; prints one JSON line per round and workload (ms per step, Mpps, the mean
ms per launch kind from gpc_launch_times, "v6_lb" among them) and a closing line with the C4v6 / C3v6
ratio of the medians. bench.py stays the flagship yardstick; this only measures the new path."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1 << 26)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--embed", default="96", choices=("96", "multi48"))
    args = ap.parse_args()

    import torch
    from antrea_amd import gpc, workload
    from antrea_amd.build import build
    build()
    dev = torch.device("cuda", 0)
    n = args.packets

    def setup(name):
        t0 = time.time()
        wl = workload.CONFIGS[name]()
        w6 = workload.services_to_ipv6(wl, args.embed) if name == "C4" else workload.to_ipv6(wl, embed=args.embed)
        clf = gpc.Classifier(ipv4=False, ipv6=True)
        clf.initialize()
        clf.batch_install_policy_rule_flows(w6.rules)
        if name == "C4":
            workload.install_services(clf, w6)
        clf.commit()
        cols4 = workload.gen_packets_torch(wl, n, seed=workload.PKT_SEED, device=dev)
        cols = workload.packets_to_v6_torch(cols4, embed=args.embed)  # (C4 has no NodePort Services: no virtual IP)
        del cols4
        out = torch.empty(2 * n * 8, dtype=torch.uint8, device=dev)
        lb = torch.empty(n * 32, dtype=torch.uint8, device=dev) if name == "C4" else None
        print("# %sv6: built in %.1f s, Service image %s" % (name, time.time() - t0,
                                                            "bound" if clf.debug_service_image6() else "none"),
              file=sys.stderr, flush=True)
        return {"name": name + "v6", "clf": clf, "cols": cols, "soa": gpc.pkt_soa_device(cols), "out": out, "lb": lb}

    def run(w, steps, timed):
        clf = w["clf"]
        if timed:
            clf.set_launch_timing(steps)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        torch.cuda.synchronize()
        for a, b in ev:
            a.record()
            clf.classify6_device(w["soa"], n, w["out"].data_ptr(), count=True)
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

    ws = [setup("C3"), setup("C4")]
    for w in ws:  # every shape warm before anything is timed
        run(w, args.warmup, False)
    if ws[1]["lb"] is not None:  # the LB results of the C4 batch, once: how many packets the stage rewrote
        w = ws[1]
        C = __import__("ctypes")
        gpc._check(w["clf"].lib.gpc_classify6_lb(w["clf"].h, C.byref(w["soa"]), n, w["out"].data_ptr(), w["lb"].data_ptr(), 0,
                                                 None), "gpc_classify6_lb")
        torch.cuda.synchronize()
        flags = w["lb"].view(n, 32)[:, 18]
        print(json.dumps({"workload": "C4v6", "hit_frac": round(float((flags & 1).ne(0).float().mean()), 4),
                          "no_endpoint_frac": round(float((flags & 2).ne(0).float().mean()), 4)}), flush=True)
    res = {w["name"]: [] for w in ws}
    for _ in range(args.rounds):
        for w in ws:
            r = run(w, args.steps, True)
            res[w["name"]].append(r["ms_per_step"])
            print(json.dumps(r), flush=True)
    med = {k: statistics.median(v) for k, v in res.items()}
    print(json.dumps({"median_ms_per_step": med, "C4v6_over_C3v6": round(med["C4v6"] / med["C3v6"], 4)}), flush=True)


if __name__ == "__main__":
    main()
