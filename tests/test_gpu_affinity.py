"""GPU tier: session affinity of IPv4 Services on the device (classify.hip aff_sweep_kernel /
aff_learn_kernel / aff_resolve_kernel over the slot's affinity table, the policy launches over the
rewritten columns). Device == model (tests/affinity_model.py: the realized learn flows executed
serially) == host emulation of the same core.hpp bodies (tests/emu_aff.py), exactly: verdicts, LB
results with the two affinity flag bits, the live entries, gpc_affinity_stats and the per-rule
counters. Every equality test asserts overflow == 0 (tables of 2^12 slots for a few hundred keys, or
key sets that cannot overflow whatever the order: the emulation shows the same on the CPU tier) or an
overflow count the batch's order forces; the capacity and racing tests check properties instead."""
import copy
import ipaddress

import numpy as np
import pytest

from antrea_amd import gpc, workload
from tests import affinity_cases as ac
from tests import emu, emu_aff
from tests.test_emu_parity import _cmp

pytestmark = pytest.mark.gpu

A, L = gpc.LB_AFFINITY, gpc.LB_LEARNED
GOLD_CFG = {"ip": "10.96.0.100", "port": 80, "protocol": "TCP", "cluster_group_id": 100, "local_group_id": 101,
            "affinity_timeout": 100}


@pytest.fixture(scope="module", autouse=True)
def _built():
    from antrea_amd.build import build
    build()
    import torch
    assert torch.cuda.is_available(), "GPU tier needs a HIP device"


def _metrics(c):
    return {k: tuple(v) for k, v in c.network_policy_metrics().items() if any(v)}


def _device_live(c):
    """(reachable live entries as (src, dst, endpoint ip, endpoint port | flags, expires), all live)."""
    t = c.affinity_table()
    return [(int(e["src"]), int(e["dst"]), int(e["endpoint_ip"]), int(e["endpoint_port"]), int(e["expires"]))
            for e in t if e["dst"]], len(t)


def _runner(c, table):
    """The device side of a scripted step, checked against the emulation on the way: verdicts, LB
    results, live entries (by install id), stats and the per-rule counters of the step."""
    def run(name, cols, now):
        c.set_affinity_clock(now)
        c.reset_counters()
        got, lb = c.classify_host(cols, count=True, lb=True)
        _, slots = c.counters()
        arr = np.zeros((len(slots), 3), dtype=np.uint64)
        elb = np.zeros(len(lb), gpc.LB_DTYPE)
        _cmp(got, table.classify(c, cols, now, counters=arr, lb=elb), cols)
        assert (lb == elb).all(), name
        exp = {conj: tuple(int(x) for x in arr[i]) for i, conj in enumerate(slots) if conj and arr[i].any()}
        assert exp and _metrics(c) == exp, name
        stats = c.affinity_stats()
        assert stats == table.stats(now), (name, stats, table.stats(now))
        dev = sorted((int(e["src"]), int(e["install_id"]), int(e["endpoint_ip"]), int(e["endpoint_port"]), int(e["expires"]))
                     for e in c.affinity_table())
        assert dev == sorted((e[0], e[1] >> 8) + e[2:] for e in table.live(now)), name
        live, n_all = _device_live(c)
        return got, lb, live, stats, n_all
    return run


def _simple(n_services=3, n_eps=8, log2=ac.LOG2, **kw):
    """C1's rules + `n_services` affinity ClusterIP Services of `n_eps` remote Endpoints each."""
    wl = workload.config1(seed=81)
    c = gpc.Classifier(session_affinity=log2, **kw)
    c.initialize()
    c.batch_install_policy_rule_flows(copy.deepcopy(wl.rules))
    svcs = []
    for s in range(n_services):
        eps = [{"ip": "10.128.%d.%d" % (s + 1, k + 1), "port": 8000 + k, "is_local": False, "node_name": "n%d" % k}
               for k in range(n_eps)]
        cfg = dict(GOLD_CFG, ip="10.96.0.%d" % (100 + s), cluster_group_id=100 + 2 * s, local_group_id=101 + 2 * s)
        c.install_service_group(cfg["cluster_group_id"], eps, True)
        c.install_endpoint_flows("TCP", eps)
        c.install_service_flows(cfg)
        svcs.append((cfg, eps))
    wl.pods = {}
    return wl, c, svcs


def _to_services(wl, svcs, n, seed, clients, established=0.3):
    """n packets of `clients` sources to the Services (random source ports), `established` of them +est."""
    rng = np.random.default_rng(seed)
    cols = workload.gen_packets(wl, n, seed=seed)
    k = rng.integers(0, len(svcs), size=n)
    cols["src"] = (0x0a0a0000 + 5 + rng.integers(0, clients, size=n)).astype(np.uint32)
    cols["dst"] = np.array([int(ipaddress.ip_address(svcs[j][0]["ip"])) for j in k], np.uint32)
    cols["dport"] = np.full(n, 80, np.uint16)
    cols["proto"] = np.full(n, 6, np.uint8)
    cols["sport"] = rng.integers(1024, 65536, size=n).astype(np.uint16)
    cols["ct_state"] = np.where(rng.random(n) < established, ac.gpc_ct("est"), ac.gpc_ct("new")).astype(np.uint8)
    return cols


def test_gpu_contention_one_learner_per_key():
    """8 192 packets over 8 clients x 3 affinity Services in one batch: hundreds of lanes per key across
    32 blocks race for each key's slot and bid. Exactly one GPC_LB_LEARNED per key -- the key's first
    +new packet by caller index -- and every packet of the key at or after it has its Endpoint."""
    wl, c, svcs = _simple()
    c.commit()
    n = 8192
    cols = _to_services(wl, svcs, n, 82, clients=8)
    c.set_affinity_clock(500)
    got, lb = c.classify_host(cols, lb=True)
    new = (cols["ct_state"] & 1) != 0
    keys = {}
    for i in range(n):
        keys.setdefault((int(cols["src"][i]), int(cols["dst"][i])), []).append(i)
    assert len(keys) == 24
    own = np.zeros(n, gpc.LB_DTYPE)
    emu.classify(c, cols, lb=own)  # the plain Service stage: every packet's own hash choice
    for idx in keys.values():
        idx = np.array(idx)
        first = idx[new[idx]][0]
        learned = idx[(lb["flags"][idx] & L) != 0]
        assert list(learned) == [first]
        after = idx[idx >= first]
        assert (lb["endpoint_ip"][after] == own["endpoint_ip"][first]).all() and (lb["endpoint_port"][after] == own["endpoint_port"][first]).all()
        assert ((lb["flags"][after] & A) != 0).all()
        before = idx[idx < first]
        assert (lb["endpoint_ip"][before] == own["endpoint_ip"][before]).all() and ((lb["flags"][before] & (A | L)) == 0).all()
    assert any(new[np.array(idx)][0] == False for idx in keys.values()), "some key's first packet must not be +new"  # noqa: E712
    st = c.affinity_stats()
    assert st["learned"] == 24 and st["live"] == 24 and st["overflow"] == 0 and st["hits"] == int(((lb["flags"] & (A | L)) == A).sum())
    # == emulation == model
    table = emu_aff.Table(ac.LOG2)
    elb = np.zeros(n, gpc.LB_DTYPE)
    _cmp(got, table.classify(c, cols, 500, lb=elb), cols)
    assert (lb == elb).all() and st == table.stats(500)
    model = ac.Model(wl, c)
    want, want_lb = model.run(cols, 500)
    _cmp(got, want, cols)
    assert (lb == want_lb).all()
    live, n_all = _device_live(c)
    assert sorted(live) == model.pipe.live() and n_all == 24


@pytest.mark.parametrize("group", [1, -1], ids=["grouped", "ungrouped"])
def test_gpu_batch_shapes(group):
    """n = 1, 255, 256, 257, 3 000 (a bounds-checked tail, more than one block), group_packets forced
    on and off, with and without the optional columns the stage reads or rewrites, lb_out null: the
    device equals the emulation every time. The clock moves past the timeout between cases, so every
    case learns afresh."""
    wl = ac.make_workload(83)
    c = ac.make_product(wl, group_packets=group)
    c.commit()
    table = emu_aff.Table(ac.LOG2)
    base = ac.make_batch(wl, 3000, 84, clients=40, established=0.3)
    rng = np.random.default_rng(85)
    extra = {"ct_dst": base["src"][::-1].copy(), "svc_group": rng.integers(0, 50, 3000).astype(np.uint32),
             "dest": rng.integers(0, 4, 3000).astype(np.uint8)}
    now = 100
    variants = [(n, base) for n in (1, 255, 256, 257, 3000)]
    variants += [(257, dict(base, **extra)), (3000, dict(base, **extra)),
                 (3000, {k: v for k, v in base.items() if k != "ct_state"}),
                 (257, {k: v for k, v in dict(base, **extra).items() if k not in ("ct_state", "dest")})]
    seen = 0
    for n, full in variants:
        cols = {k: np.ascontiguousarray(v[:n]) for k, v in full.items()}
        now += ac.T
        c.set_affinity_clock(now)
        got, lb = c.classify_host(cols, lb=True)
        elb = np.zeros(n, gpc.LB_DTYPE)
        _cmp(got, table.classify(c, cols, now, lb=elb), cols)
        assert (lb == elb).all(), (n, sorted(cols))
        st = c.affinity_stats()
        assert st == table.stats(now) and st["overflow"] == 0, (n, st)
        seen += int(((lb["flags"] & L) != 0).sum())
    assert seen > 500
    # lb_out null: the same launches, the results just are not stored
    now += ac.T
    c.set_affinity_clock(now)
    cols = {k: np.ascontiguousarray(v[:3000]) for k, v in base.items()}
    got = c.classify_host(cols)
    _cmp(got, table.classify(c, cols, now), cols)
    assert c.affinity_stats() == table.stats(now)
    assert sorted((e[0], e[1] >> 8) + e[2:] for e in table.live(now)) == \
        sorted((int(e["src"]), int(e["install_id"]), int(e["endpoint_ip"]), int(e["endpoint_port"]), int(e["expires"]))
               for e in c.affinity_table())


@pytest.mark.parametrize("mode", ["base", "ext", "journal"])
def test_gpu_scripted_sequence(mode):
    """The CPU tier's sequence on the device (time, hard timeout, an Endpoint leaving, a reinstall, a
    NetworkPolicy-only commit). "ext" / "journal": after address churn that puts the epoch in
    point-extension mode / a rule install that puts it in journal mode -- the resolved policy
    kernels' other instantiations."""
    wl = ac.make_workload(86)
    c = ac.make_product(wl, compact_after=-1)
    c.commit()
    if mode == "ext":
        r = next(r for r in wl.rules if r["direction"] == "In" and r.get("from") and r.get("action") in (None, "Allow"))
        c.add_policy_rule_address(r["flow_id"], "src", ["10.77.0.9"], r.get("priority"))
        wl.rules = copy.deepcopy(wl.rules)
        next(x for x in wl.rules if x["flow_id"] == r["flow_id"])["from"].append("10.77.0.9")
        c.commit()
        st = c.image_stats()
        assert st["n_ext_rules"] > 0 and st["n_overlay_rules"] == 0, st
    elif mode == "journal":
        extra = dict(copy.deepcopy(wl.rules[1]), flow_id=max(r["flow_id"] for r in wl.rules) + 100)
        c.install_policy_rule_flows(copy.deepcopy(extra))
        wl.rules = copy.deepcopy(wl.rules) + [extra]
        c.commit()
        assert c.image_stats()["n_overlay_rules"] > 0
    table = emu_aff.Table(ac.LOG2)
    ac.scripted_sequence(wl, c, c.commit, _runner(c, table), n=500 if mode == "base" else 300,
                         established=0.0 if mode == "base" else 0.4, dst_known=True)
    st = c.affinity_stats()
    assert st["sweeps"] >= 5 and st["overflow"] == 0


def test_gpu_capacity_overflow_and_slot_reuse():
    """256 slots, 4 096 distinct clients of one Service: properties, not equality -- which keys
    overflow is decided by arrival order."""
    wl, c, svcs = _simple(n_services=1, n_eps=4, log2=8)
    c.commit()
    cfg, eps = svcs[0]

    def batch(first, n):
        return {"src": (0x0a800000 + first + np.arange(n)).astype(np.uint32),
                "dst": np.full(n, int(ipaddress.ip_address(cfg["ip"])), np.uint32),
                "sport": (1024 + np.arange(n) % 60000).astype(np.uint16), "dport": np.full(n, 80, np.uint16),
                "proto": np.full(n, 6, np.uint8), "out_port": np.zeros(n, np.uint32)}
    cols = batch(0, 4096)
    c.set_affinity_clock(10)
    _, lb = c.classify_host(cols, lb=True)
    st = c.affinity_stats()
    assert st["slots"] == 256 and st["overflow"] > 0 and st["live"] <= 256
    assert st["learned"] == st["live"] and st["learned"] + st["overflow"] == 4096
    ep = {(int(ipaddress.ip_address(e["ip"])), e["port"]) for e in eps}
    assert {(int(a), int(p)) for a, p in zip(lb["endpoint_ip"], lb["endpoint_port"])} <= ep
    t = c.affinity_table()
    assert len(t) == st["live"] and (t["dst"] == int(ipaddress.ip_address(cfg["ip"]))).all() and (t["expires"] == 110).all()
    held = {int(e["src"]): (int(e["endpoint_ip"]), int(e["endpoint_port"]) & 0xffff) for e in t}
    learned = (lb["flags"] & L) != 0
    assert set(held) == set(int(s) for s in cols["src"][learned])
    c.set_affinity_clock(11)
    cols2 = dict(cols, sport=(cols["sport"] + 7).astype(np.uint16))  # other hash choices
    _, lb2 = c.classify_host(cols2, lb=True)
    for i in np.nonzero(learned)[0]:  # keys that did get an entry hit it
        assert (int(lb2["endpoint_ip"][i]), int(lb2["endpoint_port"][i])) == held[int(cols["src"][i])]
    assert ((lb2["flags"][learned] & (A | L)) == A).all()
    over = c.affinity_stats()["overflow"]
    c.set_affinity_clock(110)  # past the timeout: the sweep frees every slot
    _, lb3 = c.classify_host(batch(5000, 100), lb=True)
    st = c.affinity_stats()
    assert st["overflow"] == over and st["live"] == 100 and ((lb3["flags"] & L) != 0).all() and st["sweeps"] >= 2


def test_gpu_trace_reads_the_table_and_never_learns():
    wl, c, svcs = _simple(n_services=1)
    c.commit()
    cfg, eps = svcs[0]
    pkt = {"src": 0x0a0a0005, "dst": int(ipaddress.ip_address(cfg["ip"])), "sport": 40000, "dport": 80, "proto": 6,
           "out_port": 0}
    c.set_affinity_clock(20)
    cols = {k: np.array([v], gpc.PKT_COLUMNS[k]) for k, v in pkt.items()}
    own, own6 = {}, {}
    for sp in (40000, 40001, 40002, 40003, 40004, 40005):  # traces before anything is learned: the hash choice
        v, steps, lb = c.trace(dict(pkt, sport=sp))
        own[sp] = (int(lb["endpoint_ip"]), int(lb["endpoint_port"]))
        assert not (lb["flags"] & (A | L)) and lb["flags"] & gpc.LB_HIT
        v, steps, lb = c.trace(dict(pkt, src=0x0a0a0006, sport=sp))  # (another client)
        own6[sp] = (int(lb["endpoint_ip"]), int(lb["endpoint_port"]))
    assert c.affinity_stats()["learned"] == 0 and len(set(own.values())) > 1
    got, lbb = c.classify_host(cols, lb=True)
    assert lbb["flags"][0] & L and (int(lbb["endpoint_ip"][0]), int(lbb["endpoint_port"][0])) == own[40000]
    other = next(sp for sp in own if own[sp] != own[40000])
    v, steps, lb = c.trace(dict(pkt, sport=other))  # a live entry: the learned Endpoint, whatever the hash says
    assert (int(lb["endpoint_ip"]), int(lb["endpoint_port"])) == own[40000] and (lb["flags"] & (A | L)) == A
    v2 = c.classify_host({k: np.array([x], gpc.PKT_COLUMNS[k]) for k, x in dict(pkt, sport=other).items()})
    assert (v == v2[0]).all() and len(steps) >= 1
    st = c.affinity_stats()
    assert st["learned"] == 1 and st["live"] == 1 and st["hits"] == 1  # (the second batch's hit; traces count nothing)
    v, steps, lb = c.trace(dict(pkt, src=0x0a0a0006, sport=other))  # another client: no entry, nothing created
    assert (int(lb["endpoint_ip"]), int(lb["endpoint_port"])) == own6[other] and not (lb["flags"] & (A | L))
    assert c.affinity_stats()["live"] == 1 and len(c.affinity_table()) == 1
    c.set_affinity_clock(20 + 100)  # expired
    v, steps, lb = c.trace(dict(pkt, sport=other))
    assert (int(lb["endpoint_ip"]), int(lb["endpoint_port"])) == own[other] and not (lb["flags"] & (A | L))


def test_gpu_two_streams_are_ordered_by_the_library():
    """Two batches that share keys, issued back to back on different streams with no ordering of the
    caller's: the result is that of running them in issue order."""
    import torch
    wl, c, svcs = _simple()
    c.commit()
    n = 4096
    dev = torch.device("cuda", 0)
    signed = {4: np.int32, 2: np.int16, 1: np.uint8}
    b = [_to_services(wl, svcs, n, 90 + k, clients=32, established=0.2) for k in range(2)]
    up = lambda cols: {k: torch.as_tensor(np.ascontiguousarray(a, dtype=gpc.PKT_COLUMNS[k]).view(
        signed[np.dtype(gpc.PKT_COLUMNS[k]).itemsize])).to(dev) for k, a in cols.items()}
    d = [up(x) for x in b]
    outs = [torch.zeros(16 * n, dtype=torch.uint8, device=dev) for _ in range(2)]
    lbs = [torch.zeros(16 * n, dtype=torch.uint8, device=dev) for _ in range(2)]
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    torch.cuda.synchronize(dev)
    c.set_affinity_clock(700)
    for k in range(2):
        c.classify_device(gpc.pkt_soa_device(d[k]), n, outs[k].data_ptr(), stream=streams[k].cuda_stream, lb_ptr=lbs[k].data_ptr())
    torch.cuda.synchronize(dev)
    table = emu_aff.Table(ac.LOG2)
    for k in range(2):
        elb = np.zeros(n, gpc.LB_DTYPE)
        want = table.classify(c, b[k], 700, lb=elb)
        _cmp(outs[k].cpu().numpy().view(gpc.VERDICT_DTYPE).reshape(n, 2), want, b[k])
        assert (lbs[k].cpu().numpy().view(gpc.LB_DTYPE) == elb).all(), k
    lb1 = lbs[1].cpu().numpy().view(gpc.LB_DTYPE)
    assert ((lb1["flags"] & L) != 0).sum() < 10 < ((lb1["flags"] & A) != 0).sum()  # the second batch found the first one's entries
    assert c.affinity_stats() == table.stats(700)


def test_gpu_no_affinity_service_no_affinity_launch():
    """Feature on, no affinity Service committed: the launch timing of a C1 + Services batch lists no
    aff_* kernel (and the results are those of a context without the feature); with an affinity
    Service the three kinds appear."""
    wl = workload.add_services(workload.config1(seed=51), 60, 4, seed=51, noep_frac=0.1, local_policy_frac=0.2)
    cols = workload.gen_packets(wl, 2000, seed=51)
    res = []
    for log2 in (12, 0):
        c = gpc.Classifier(session_affinity=log2)
        c.initialize()
        c.batch_install_policy_rule_flows(copy.deepcopy(wl.rules))
        workload.install_services(c, wl)
        c.commit()
        c.set_launch_timing(8)
        res.append(c.classify_host(cols, lb=True))
        kinds = set(c.launch_times())
        assert kinds and not any(k.startswith("aff_") for k in kinds), kinds
        assert c.affinity_stats()["live"] == 0
    assert (res[0][0] == res[1][0]).all() and (res[0][1] == res[1][1]).all()
    wl2 = ac.make_workload(83)
    c = ac.make_product(wl2)
    c.commit()
    c.set_launch_timing(8)
    b = ac.make_batch(wl2, 1000, 84)
    c.set_affinity_clock(5)
    c.classify_host(b)
    kinds = set(c.launch_times())
    assert {"aff_learn", "aff_resolve"} <= kinds and "aff_sweep" not in kinds, kinds  # (a new table: nothing to sweep)
    c.set_affinity_clock(6)
    c.classify_host(b)
    kinds = set(c.launch_times())
    assert {"aff_learn", "aff_resolve", "aff_sweep"} <= kinds, kinds


# ------------------------------------------------------------------ the table under hash pressure
# tests/affinity_cases.py KeySet: keys chosen with the product's hash to share buckets in a table of
# 256 slots. Exact (device == emulation == model) wherever no arrival order can overflow or the order
# is forced; properties where lanes race for a full bucket.
@pytest.fixture(scope="module")
def pressure_keys():
    wl, c, svcs = ac.make_pressure_product()
    c.commit()
    return ac.KeySet(c)


def _pressure(**kw):
    wl, c, svcs = ac.make_pressure_product(**kw)
    c.commit()
    return wl, c, svcs, emu_aff.Table(ac.P_LOG2)


def test_gpu_colliding_keys_in_one_batch(pressure_keys):
    """38 keys x 64 packets, shuffled over ten blocks: four keys with one first bucket, a key whose two
    buckets coincide and its neighbour, a chain, background pairs with identical candidates. Lanes of
    different keys race for the same slots; which key gets which is open, the results are not."""
    wl, c, svcs, table = _pressure()
    second = ac.case_collisions(wl, c, svcs, pressure_keys, table, _runner(c, table), 0, dst_known=True)
    assert len(second) >= 2 and c.affinity_stats()["overflow"] == 0


def test_gpu_live_key_behind_an_emptied_bucket(pressure_keys):
    wl, c, svcs, table = _pressure()
    ac.case_emptied_bucket(wl, c, svcs, pressure_keys, table, _runner(c, table), c.commit, 0, dst_known=True)
    assert c.affinity_stats()["overflow"] == 0


def test_gpu_full_bucket_forced_order(pressure_keys):
    wl, c, svcs, table = _pressure()
    ac.case_full_bucket_forced(wl, c, svcs, pressure_keys, _runner(c, table), 0, dst_known=True)


@pytest.mark.parametrize("per_key", [64, 1024])
def test_gpu_racing_for_a_full_bucket(pressure_keys, per_key):
    """Six keys with the same four candidate slots in one batch on an empty table (per_key = 1024: 24
    blocks): which four keys get a slot is decided by the race, so properties, not equality. Each key
    is all-or-nothing: a holder behaves as a key alone in the table would, a loser as if the Service
    had no affinity."""
    wl, c, svcs, _ = _pressure()
    keys = pressure_keys.identical
    cols = ac.key_batch(wl, svcs, keys, 231, per_key=per_key)
    index = ac.key_index(cols, svcs, keys)
    own = ac.own_choices(c, cols)
    ac.check_spread(own, index)
    new = (cols["ct_state"] & 1) != 0
    c.set_affinity_clock(ac.T0)
    _, lb = c.classify_host(cols, lb=True)
    holders = [k for k in keys if ((lb["flags"][index[k]] & L) != 0).any()]
    losers = [k for k in keys if k not in holders]
    assert len(holders) == 4
    bound = {}
    for k in holders:
        idx = index[k]
        first = ac.first_new(cols, idx)
        assert list(idx[(lb["flags"][idx] & L) != 0]) == [first]
        after, before = idx[idx >= first], idx[idx < first]
        assert (lb["endpoint_ip"][after] == own["endpoint_ip"][first]).all() and (lb["endpoint_port"][after] == own["endpoint_port"][first]).all()
        assert ((lb["flags"][after] & A) != 0).all()
        assert (lb[before] == own[before]).all() and ((lb["flags"][before] & (A | L)) == 0).all()
        bound[k] = (int(own["endpoint_ip"][first]), int(own["endpoint_port"][first]))
    for k in losers:
        assert (lb[index[k]] == own[index[k]]).all() and ((lb["flags"][index[k]] & (A | L)) == 0).all()
    lost_new = sum(int(new[index[k]].sum()) for k in losers)
    st = c.affinity_stats()
    assert lost_new > 0 and st["overflow"] == lost_new and st["learned"] == st["live"] == 4, st
    dst = {k: int(ipaddress.ip_address(svcs[k.svc][0]["ip"])) for k in keys}
    t = c.affinity_table()
    assert sorted((int(e["src"]), int(e["dst"])) for e in t) == sorted((k.src, dst[k]) for k in holders)
    # the same batch again: the holders hit, the same two keys find the bucket full again
    c.set_affinity_clock(ac.T0 + 1)
    _, lb2 = c.classify_host(cols, lb=True)
    ac.check_all_hits(lb2, {k: index[k] for k in holders}, bound)
    for k in losers:
        assert (lb2[index[k]] == own[index[k]]).all()
    st = c.affinity_stats()
    assert st["overflow"] == 2 * lost_new and st["learned"] == st["live"] == 4, st
    assert sorted((int(e["src"]), int(e["dst"])) for e in c.affinity_table()) == sorted((k.src, dst[k]) for k in holders)


def test_gpu_launch_sequence_wrap(pressure_keys):
    wl, c, svcs, table = _pressure()
    with pytest.raises(gpc.GpcError) as e:  # no table yet: its first use would restart the sequence
        c.debug_set_affinity_seq(5)
    assert e.value.code == gpc.GPC_EINVAL

    def set_seq(seq):
        c.debug_set_affinity_seq(seq)
        table.set_seq(seq)
    ac.case_sequence_wrap(wl, c, svcs, pressure_keys, table, _runner(c, table), set_seq, 0, dst_known=True)
    assert c.affinity_stats()["overflow"] == 0


def test_gpu_tables_are_per_slot(pressure_keys):
    """Two device slots on one GPU: what slot 0 learned is unknown to slot 1, which learns the same
    batch again; each slot equals an emulated table of its own."""
    wl, c, svcs, t0 = _pressure(devices=[0, 0])
    t1 = emu_aff.Table(ac.P_LOG2)
    keys = pressure_keys.shared + pressure_keys.chain + pressure_keys.degenerate
    ac.check_no_overflow(keys)
    cols = ac.key_batch(wl, svcs, keys, 241)
    index = ac.key_index(cols, svcs, keys)
    entries = lambda slot: sorted((int(e["src"]), int(e["install_id"]), int(e["endpoint_ip"]), int(e["endpoint_port"]),
                                   int(e["expires"])) for e in c.affinity_table(slot))
    emulated = lambda t, now: sorted((e[0], e[1] >> 8) + e[2:] for e in t.live(now))

    def run(slot, table, batch, now):
        c.set_affinity_clock(now)
        got, lb = c.classify_host(batch, lb=True, slot=slot)
        elb = np.zeros(len(lb), gpc.LB_DTYPE)
        _cmp(got, table.classify(c, batch, now, lb=elb), batch)
        assert (lb == elb).all(), slot
        assert c.affinity_stats(slot) == table.stats(now) and entries(slot) == emulated(table, now), slot
        return lb
    lb0 = run(0, t0, cols, ac.T0)
    bound = ac.learned_endpoints(cols, lb0, index)
    assert c.affinity_stats(1)["learned"] == 0 and len(c.affinity_table(1)) == 0
    lb1 = run(1, t1, cols, ac.T0)
    assert (lb1 == lb0).all() and ac.learned_endpoints(cols, lb1, index) == bound  # its own LEARNED packets
    assert c.affinity_stats(0)["learned"] == c.affinity_stats(1)["learned"] == len(keys)
    again = ac.key_batch(wl, svcs, keys, 242)
    ac.check_all_hits(run(0, t0, again, ac.T0 + 1), ac.key_index(again, svcs, keys), bound)
    assert c.affinity_stats(0)["learned"] == len(keys) and c.affinity_stats(0)["overflow"] == c.affinity_stats(1)["overflow"] == 0
