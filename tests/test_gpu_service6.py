"""GPU tier: the IPv6 AntreaProxy stage on the device (classify.hip v6_lb_kernel in front of the code
pass, the policy launches over the rewritten columns). The device's verdicts and gpc_lb_result6 equal
the test-side executor (tests/svc6_model.py: OVS semantics over the realized IPv6 flow / group text,
then the unmodified oracle) and its counters equal the host emulation's (tests/emu_svc6.py)."""
import copy
import ipaddress

import numpy as np
import pytest

from antrea_amd import gpc, workload
from tests import emu, emu_svc6, svc6_model
from tests.test_emu_parity import _cmp
from tests.test_service6 import check_input_conditions, executor, product6, svc_workload6

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _built():
    from antrea_amd.build import build
    build()
    import torch
    assert torch.cuda.is_available(), "GPU tier needs a HIP device"


def _metrics(c):
    return {k: tuple(v) for k, v in c.network_policy_metrics().items() if any(v)}


@pytest.mark.parametrize("group", [0, 1])
@pytest.mark.parametrize("name,seed", [("C1", 71), ("C1np", 72)])
def test_gpu_service6_stage(name, seed, group):
    wl, w6 = svc_workload6(name, seed)
    n = 3000
    cols = workload.gen_packets(wl, n, seed=seed)
    cols6 = workload.service_packets_to_v6(cols)
    c = product6(w6, group_packets=1 if group else -1)
    c.commit()
    got, lb = c.classify6_host(cols6, count=True, lb=True)
    want, want_lb = svc6_model.run(executor(w6, c), cols6, n)
    _cmp(got, want, cols)
    bad = np.nonzero(lb != want_lb)[0]
    assert len(bad) == 0, (bad[:5], lb[bad[:3]], want_lb[bad[:3]])
    check_input_conditions(lb, cols, name)
    _, slots = c.counters()
    arr = np.zeros((len(slots), 3), dtype=np.uint64)
    _cmp(got, emu_svc6.classify6(c, cols6, counters=arr), cols)
    exp = {conj: tuple(int(x) for x in arr[i]) for i, conj in enumerate(slots) if conj and arr[i].any()}
    assert exp and _metrics(c) == exp
    # packets of a Service without Endpoints add to no slot
    noep = (lb["flags"] & gpc.LB_NO_ENDPOINT) != 0
    c.reset_counters()
    sub = {k: np.ascontiguousarray(v[noep]) for k, v in cols6.items()}
    v = c.classify6_host(sub, count=True)
    assert noep.sum() > 3 and (v[:, 0]["table"] == gpc.VTABLE_ENDPOINT_DNAT).all() and (v[:, 1]["action"] == 0).all()
    assert _metrics(c) == {}
    # without lb_out the stage still runs (gpc_classify6 == gpc_classify6_lb minus the results)
    _cmp(c.classify6_host(cols6), got, cols)


# ---- edge table
A1, A2, A3 = "fd00:10::a60:64", "fd01:10::a60:64", "fd00:10::a60:65"  # A2: top word differs; A3: low word differs


def _edge_workload():
    wl = workload.config1(seed=58)
    w6 = workload.to_ipv6(wl)
    w6.svc_family = 6
    w6.pods = {workload.v6_embed(int(ip)): int(p) for ip, p in zip(wl.local_ips, wl.local_ports)}
    local = lambda j: {"ip": str(ipaddress.IPv6Address(workload.v6_embed(int(wl.local_ips[j % len(wl.local_ips)])))),
                       "port": 8000 + j, "is_local": True, "node_name": "node0"}
    remote = lambda j: {"ip": "fd00:10::a80:%x" % (j + 1), "port": 9000 + j, "is_local": False, "node_name": "node7"}
    w6.groups = {1: [local(0)], 2: [remote(0), local(1), remote(1)],
                 3: [remote(10 + j) if j % 3 else local(10 + j) for j in range(65)],  # lg > 6, slot % 65
                 4: [local(2), local(3), remote(2)], 5: [remote(3)], 6: []}
    w6.endpoint_flows = [("TCP", w6.groups[g]) for g in (1, 2, 3, 4)] + [("UDP", w6.groups[5])]
    svc = lambda ip, port, proto, gid: {"ip": ip, "port": port, "protocol": proto, "cluster_group_id": gid,
                                        "local_group_id": 100 + gid, "traffic_policy_local": False}
    w6.services = [svc(A1, 80, "TCP", 1), svc(A2, 80, "TCP", 2), svc(A3, 80, "TCP", 3), svc(A1, 81, "TCP", 4),
                   svc(A1, 80, "UDP", 5), svc(A2, 81, "TCP", 6)]
    n = 257
    cols6 = workload.packets_to_v6(workload.gen_packets(wl, n, seed=58))
    #          dst  dport proto
    targets = [(A1, 80, 6), (A2, 80, 6), (A3, 80, 6), (A1, 81, 6), (A1, 80, 17), (A2, 81, 6), (A1, 80, 58), (A1, 82, 6),
               (A3, 80, 6), ("fd02:10::a60:64", 80, 6), (A3, 80, 17), None]
    for i in range(n):
        t = targets[i % len(targets)]
        if t is not None:
            cols6["dst6"][i] = np.frombuffer(ipaddress.IPv6Address(t[0]).packed, np.uint8)
            cols6["dport"][i], cols6["proto"][i] = t[1], t[2]
    return w6, cols6, n


def test_gpu_service6_edge_table():
    w6, cols6, n = _edge_workload()
    c = product6(w6)
    c.commit()
    ct = dict(cols6, ct_dst6=np.ascontiguousarray(cols6["src6"][::-1]))  # ct_dst6 given: it is the ct_ipv6_dst
    pipe = executor(w6, c)
    for batch in (cols6, ct):
        want, want_lb = svc6_model.run(pipe, batch, n)
        f = want_lb["flags"]
        assert ((f & gpc.LB_HIT) != 0).sum() > n // 2 and (f & gpc.LB_NO_ENDPOINT).any()
        assert len({bytes(x) for x in want_lb["endpoint_ip"][want_lb["group_id"] == 3]}) > 20  # the 65-Endpoint group spreads
        assert (f[np.asarray(batch["proto"]) == 58] == 0).all()  # ICMPv6 to a Service IP: no hit
        for k in (1, 63, 64, 65, 257):
            sub = {name: np.ascontiguousarray(v[:k]) for name, v in batch.items()}
            got, lb = c.classify6_host(sub, lb=True)
            _cmp(got, want[:k], sub)
            assert (lb == want_lb[:k]).all(), k


def test_gpu_service6_delta_epoch_and_service_only_commit():
    """An IPv6 delta epoch (an address add) over a committed Service image -- the journal kernels over
    the rewritten columns, the image carried over -- then a Service-only commit: both equal the
    emulation and the executor."""
    wl, w6 = svc_workload6("C1", 73)
    n = 2000
    cols = workload.gen_packets(wl, n, seed=73)
    cols6 = workload.service_packets_to_v6(cols)
    c = product6(w6, compact_after=-1)
    c.commit()

    def check():
        got, lb = c.classify6_host(cols6, lb=True)
        elb = np.zeros(n, dtype=gpc.LB6_DTYPE)
        _cmp(got, emu_svc6.classify6(c, cols6, lb=elb), cols)
        assert (lb == elb).all()
        want, want_lb = svc6_model.run(executor(w6, c), cols6, n)
        _cmp(got, want, cols)
        assert (lb == want_lb).all()
        return got

    v0 = check()
    d0 = c.image_stats()["v6_delta_builds"]
    r = next(r for r in w6.rules if r["direction"] == "In" and r.get("from") and r.get("action") in (None, "Allow"))
    src = str(ipaddress.IPv6Address(bytes(cols6["src6"][0])))
    c.add_policy_rule_address(r["flow_id"], "src", [src], r.get("priority"))
    w6.rules = copy.deepcopy(w6.rules)
    next(x for x in w6.rules if x["flow_id"] == r["flow_id"])["from"].append(src)
    c.commit()
    st = c.image_stats()
    assert st["v6_delta_builds"] == d0 + 1 and st["v6_overlay_rules"] > 0, st
    check()
    for cfg in w6.services[::4]:  # Services change, the rules do not
        c.uninstall_service_flows(cfg["ip"], cfg["port"], cfg["protocol"])
    w6.services = [s for i, s in enumerate(w6.services) if i % 4]
    c.commit()
    v2 = check()
    assert (v2 != v0).any()


def test_gpu_service6_dual_stack_on_device():
    """classify_host and classify6_host in one context with the Services of both families, each equal
    to the result of a context holding that family's Services alone."""
    wl, w6 = svc_workload6("C1np", 74, gid_offset=1000)
    dual = workload.to_ipv6(wl, dual=True)
    w6.rules = dual.rules
    wl4 = copy.copy(wl)
    wl4.rules = dual.rules
    n = 3000
    cols = workload.gen_packets(wl, n, seed=74)
    cols6 = workload.service_packets_to_v6(cols)
    both, only4, only6 = product6(w6, extra=wl4), product6(wl4), product6(w6)
    for c in (both, only4, only6):
        c.commit()
    got, lb = both.classify_host(cols, lb=True)
    want, want_lb = only4.classify_host(cols, lb=True)
    _cmp(got, want, cols)
    assert (lb == want_lb).all() and (lb["flags"] & gpc.LB_HIT).mean() > 0.3
    _cmp(got, emu.classify(both, cols), cols)
    got6, lb6 = both.classify6_host(cols6, lb=True)
    want6, want_lb6 = only6.classify6_host(cols6, lb=True)
    _cmp(got6, want6, cols)
    assert (lb6 == want_lb6).all() and (lb6["flags"] & gpc.LB_HIT).mean() > 0.3
    # IPv4 Services alone: the IPv6 path has no Service stage and reports no selection
    v, z = only4.classify6_host(cols6, lb=True)
    _cmp(v, emu.classify6(only4, cols6), cols)
    assert not z["flags"].any() and not z["endpoint_ip"].any()
