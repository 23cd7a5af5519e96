"""GPU tier: the packet source column on the device (classify.hip: the Service stage of
classify_kernel, v6_lb_kernel, the affinity passes of both families, both trace kernels) and the
short-circuit flow of external Services with externalTrafficPolicy: Local. Device == model
(tests/svc_source_model.py over the realized text) == host emulation of the same core.hpp bodies
(tests/emu_src.py), exactly: verdicts and LB results with every flag bit, and with session affinity
the live entries. Every test installs an external + Local Service, which a context without
gpc_config.packet_source rejects."""
import copy

import numpy as np
import pytest

from antrea_amd import gpc
from tests import pkt_source_cases as pc
from tests.test_emu_parity import _cmp

pytestmark = pytest.mark.gpu

A, L, SC = gpc.LB_AFFINITY, gpc.LB_LEARNED, gpc.LB_SHORT_CIRCUIT
SIZES = (1, 63, 64, 65, 257)  # around one wavefront and one block


@pytest.fixture(scope="module", autouse=True)
def _built():
    from antrea_amd.build import build
    build()
    import torch
    assert torch.cuda.is_available(), "GPU tier needs a HIP device"


def _three(name, cols, dev, side, model, now=pc.T0):
    """One batch through the device, the emulation and the model; returns the device's results."""
    got = dev(cols, now)
    pc.check(name + ": device == emulation", cols, got, side.run(cols, now))
    pc.check(name + ": device == model", cols, got, model.run(cols, now))
    return got


@pytest.mark.parametrize("affinity", [False, True], ids=["plain", "affinity"])
@pytest.mark.parametrize("family", [4, 6])
def test_gpu_default_launch_sizes(family, affinity):
    wl, w6 = pc.make_workload(5, affinity)
    w = w6 if family == 6 else wl
    c = pc.make_product(w, family, affinity)
    c.commit()
    dev, side, model = pc.device_side(c, family), pc.Emulation(c, family, affinity), pc.Model(w, c, family)
    for k, n in enumerate(SIZES):
        cols = pc.make_batch(wl, n, 20 + k, family, established=0.3 if affinity else 0.0)
        got = _three("n = %d" % n, cols, dev, side, model, pc.T0 + k)
        if affinity:
            assert pc.device_live(c, family) == side.live(pc.T0 + k) == pc.model_live(model)
    pc.coverage(cols, got[1], affinity)


@pytest.mark.parametrize("family", [4, 6])
def test_gpu_grouped_across_a_tile_boundary(family):
    """group_packets=1, n = 16384 + 65: two tiles, the column permuted with the others (IPv4) and the
    policy launches split, so the ingress launch reads what the Service stage parked. The batch draws
    its packets from 257 distinct ones, whose model results are computed once and indexed."""
    wl, w6 = pc.make_workload(5)
    w = w6 if family == 6 else wl
    c = pc.make_product(w, family, group_packets=1)
    c.commit()
    base = pc.make_batch(wl, 257, 31, family)
    want, want_lb = pc.Model(w, c, family).run(base)
    n = 16384 + 65
    idx = np.random.default_rng(32).integers(0, 257, size=n)
    cols = pc.take(base, idx)
    got = pc.device_side(c, family)(cols)
    pc.check("device == model", cols, got, (want[idx], want_lb[idx]))
    pc.check("device == emulation", cols, got, pc.Emulation(c, family).run(cols))
    pc.coverage(cols, got[1])


@pytest.mark.parametrize("family", [4, 6])
def test_gpu_after_a_rule_changing_delta_commit(family):
    """A new rule committed as a delta epoch (the journal kernels) over the committed Service image."""
    wl, w6 = pc.make_workload(5)
    w = w6 if family == 6 else wl
    c = pc.make_product(w, family, compact_after=-1)
    c.commit()
    cols = pc.make_batch(wl, 257, 41, family)
    dev, side = pc.device_side(c, family), pc.Emulation(c, family)
    _three("base", cols, dev, side, pc.Model(w, c, family))
    key = "v6_delta_builds" if family == 6 else "n_delta_builds"
    d0 = c.image_stats()[key]
    r = copy.deepcopy(next(r for r in w.rules if r["direction"] == "In" and r.get("from")))
    r["flow_id"] = max(x["flow_id"] for x in w.rules) + 1
    c.install_policy_rule_flows(copy.deepcopy(r))
    w.rules = copy.deepcopy(w.rules) + [r]
    c.commit()
    st = c.image_stats()
    assert st[key] == d0 + 1 and st["v6_overlay_rules" if family == 6 else "n_overlay_rules"] > 0, st
    got = _three("delta", cols, dev, side, pc.Model(w, c, family))
    pc.coverage(cols, got[1])


def _local_empty_service(w):
    """A short-circuit Service (not NodePort) whose Local group is empty under a Cluster group with Endpoints."""
    return next(s for s in w.services if s.get("is_external") and s.get("traffic_policy_local") and not s.get("is_nodeport")
                and not w.groups[s["local_group_id"]] and w.groups[s["cluster_group_id"]])


@pytest.mark.parametrize("family", [4, 6])
def test_gpu_host_pin_and_traces_on_an_empty_local_group(family):
    """gpc_classify_host_pin_on / gpc_classify6_host_pin over packets of every source to a Service
    whose Local group is empty: SvcReject records for exactly the non-local packets, the local ones
    served from the Cluster group; gpc_trace_on / gpc_trace6 of one local and one external packet
    equal the batch's results."""
    wl, w6 = pc.make_workload(5)
    w = w6 if family == 6 else wl
    c = pc.make_product(w, family)
    c.commit()
    s = _local_empty_service(w)
    client = "fd00:10::c0a8:109" if family == 6 else "192.168.1.9"
    cols = pc.concat(*[pc.one_packet(s, family, client, 3000 + k, src) for k, src in enumerate(pc.SOURCES * 8)])
    n = len(cols["source"])
    if family == 6:
        got, lb, recs, total = c.classify6_host_pin(cols, n, lb=True)
    else:
        got, lb, recs, total = c.classify_host_pin(cols, n, lb=True)
    pc.check("device == model", cols, (got, lb), pc.Model(w, c, family).run(cols))
    pc.check("device == emulation", cols, (got, lb), pc.Emulation(c, family).run(cols))
    local = np.isin(cols["source"], (gpc.SOURCE_GATEWAY, gpc.SOURCE_POD))
    rej = recs[recs["category"] == gpc.PIN_CAT_SVC_REJECT]
    assert total == len(recs) and sorted(rej["index"].tolist()) == np.nonzero(~local)[0].tolist()
    assert ((lb["flags"][~local] & (gpc.LB_NO_ENDPOINT | SC)) == gpc.LB_NO_ENDPOINT).all()
    assert ((lb["flags"][local] & (gpc.LB_NO_ENDPOINT | SC)) == SC).all()
    assert (lb["group_id"][local] == s["cluster_group_id"]).all() and (lb["group_id"][~local] == s["local_group_id"]).all()
    for i in (int(np.nonzero(local)[0][0]), int(np.nonzero(~local)[0][0])):
        pkt = {k: (v[i] if v.ndim > 1 else v[i].item()) for k, v in cols.items()}
        t = c.trace6(pkt) if family == 6 else c.trace(pkt)
        assert (t[0] == got[i]).all() and t[2].tobytes() == lb[i].tobytes(), (i, t[0], got[i], t[2], lb[i])


def _metrics(c):
    return {k: tuple(v) for k, v in c.network_policy_metrics().items() if any(v)}


@pytest.mark.parametrize("family", [4, 6])
def test_gpu_without_the_column_a_gated_context_is_the_ungated_one(family):
    """Without a short-circuit Service (a packet_source=0 context cannot hold one) a gated context's
    results -- the batch without the column, and with it: never loaded -- equal a packet_source=0
    context's bit for bit: verdicts, lb_out, counters."""
    wl, w6 = pc.make_workload(5, short_circuit_frac=0.0)
    w = w6 if family == 6 else wl
    bare = pc.make_batch(wl, 2000, 51, family, source=False)
    full = pc.make_batch(wl, 2000, 51, family)
    res = []
    for ps, cols in ((0, bare), (1, bare), (1, full)):
        c = pc.make_product(w, family, packet_source=ps)
        c.commit()
        fn = c.classify6_host if family == 6 else c.classify_host
        v, lb = fn(cols, count=True, lb=True)
        res.append((v, lb, _metrics(c)))
    assert res[0][2] and (res[0][1]["flags"] & gpc.LB_HIT).any()
    for v, lb, m in res[1:]:
        view = {k: x for k, x in bare.items() if x.ndim == 1}
        _cmp(v, res[0][0], view)
        assert (lb == res[0][1]).all() and m == res[0][2]
