"""GPU tier: session affinity of IPv6 Services on the device (classify.hip aff6_sweep_kernel /
aff6_learn_kernel / aff6_resolve_kernel over the slot's IPv6 affinity table, then the code pass and
the policy launches over the rewritten columns). Device == model (tests/affinity6_model.py: the
realized learn flows executed serially) == host emulation of the same core.hpp bodies
(tests/emu_aff6.py), exactly: verdicts, LB results with the two affinity flag bits, the live entries,
gpc_affinity_stats6 and the per-rule counters. Equality tests use tables or key sets that cannot
overflow whatever the order (checked on the CPU with the product's own hash) or an outcome the
batch's order forces; the racing tests check properties instead. Shapes are small: C1, a few thousand
packets. (An IPv6 epoch is a base or a journal epoch: it has no extension-only mode.)"""
import copy
import ipaddress

import numpy as np
import pytest

from antrea_amd import gpc, workload
from tests import affinity6_cases as a6
from tests import affinity_cases as ac
from tests import emu, emu_aff, emu_aff6
from tests.test_emu_parity import _cmp

pytestmark = pytest.mark.gpu

A, L = gpc.LB_AFFINITY, gpc.LB_LEARNED


@pytest.fixture(scope="module", autouse=True)
def _built():
    from antrea_amd.build import build
    build()
    import torch
    assert torch.cuda.is_available(), "GPU tier needs a HIP device"


def _metrics(c):
    return {k: tuple(v) for k, v in c.network_policy_metrics().items() if any(v)}


def _entries(c, slot=0):
    """The device's live entries as (client, install id, destination, Endpoint, port | flags, expires)."""
    i = lambda b: int.from_bytes(bytes(b), "big")
    return sorted((i(e["src"]), int(e["install_id"]), i(e["dst"]), i(e["endpoint_ip"]), int(e["endpoint_port"]), int(e["expires"]))
                  for e in c.affinity_table6(slot))


def _emulated(table, now):
    return sorted((e[0], e[1] >> 8) + e[2:] for e in table.live(now))


def _upload(cols, dev):
    import torch
    signed = {4: np.int32, 2: np.int16, 1: np.uint8}
    return {k: torch.as_tensor(np.ascontiguousarray(a, dtype=gpc.PKT_COLUMNS[k]).view(
        signed[np.dtype(gpc.PKT_COLUMNS[k]).itemsize])).to(dev) for k, a in cols.items()}


def _dev6(c, cols, slot=0, count=False):
    """gpc_classify6_lb_on over device columns on the null stream: (verdicts (n, 2), lb (n,) LB6_DTYPE)."""
    import torch
    dev = torch.device("cuda", 0)
    n = len(cols["dport"])
    d = _upload(cols, dev)
    out = torch.zeros(16 * n, dtype=torch.uint8, device=dev)
    lb = torch.zeros(32 * n, dtype=torch.uint8, device=dev)
    c.classify6_lb_device(gpc.pkt_soa_device(d), n, out.data_ptr(), lb.data_ptr(), count=count, slot=slot)
    torch.cuda.synchronize(dev)
    return out.cpu().numpy().view(gpc.VERDICT_DTYPE).reshape(n, 2), lb.cpu().numpy().view(gpc.LB6_DTYPE)


def _runner(c, table):
    """The device side of a scripted step, checked against the emulation on the way: verdicts, LB
    results, live entries (by install id), stats and the per-rule counters of the step."""
    def run(name, cols, now):
        c.set_affinity_clock(now)
        c.reset_counters()
        got, lb = c.classify6_host(cols, count=True, lb=True)
        _, slots = c.counters()
        arr = np.zeros((len(slots), 3), dtype=np.uint64)
        elb = np.zeros(len(lb), gpc.LB6_DTYPE)
        want = table.classify6(c, cols, now, counters=arr, lb=elb)
        assert (got == want).all(), (name, np.nonzero((got != want).any(axis=1))[0][:5])
        assert (lb == elb).all(), name
        exp = {conj: tuple(int(x) for x in arr[i]) for i, conj in enumerate(slots) if conj and arr[i].any()}
        assert exp and _metrics(c) == exp, name
        stats = c.affinity_stats6()
        assert stats == table.stats(now), (name, stats, table.stats(now))
        dev = _entries(c)
        assert sorted(e[:2] + e[3:] for e in dev) == _emulated(table, now), name
        return got, lb, [(e[0],) + e[2:] for e in dev if e[2]], stats, len(dev)
    return run


@pytest.mark.parametrize("group", [1, -1], ids=["grouped", "ungrouped"])
@pytest.mark.parametrize("mode", ["base", "journal"])
def test_gpu_scripted_sequence(mode, group):
    """The CPU tier's sequence on the device (time, hard timeout, an Endpoint leaving, a reinstall, a
    NetworkPolicy-only commit), over a base epoch and over an IPv6 delta epoch (the journal
    instantiation of the resolved policy kernels), with packet grouping forced on and off."""
    wl, w6 = a6.make_workload(86)
    c = a6.make_product(w6, compact_after=-1, group_packets=group)
    c.commit()
    if mode == "journal":
        r = next(r for r in w6.rules if r["direction"] == "In" and r.get("from") and r.get("action") in (None, "Allow"))
        src = "fd00:10::c0a8:4d07"
        c.add_policy_rule_address(r["flow_id"], "src", [src], r.get("priority"))
        w6.rules = copy.deepcopy(w6.rules)
        next(x for x in w6.rules if x["flow_id"] == r["flow_id"])["from"].append(src)
        c.commit()
        assert c.image_stats()["v6_overlay_rules"] > 0
    table = emu_aff6.Table6(a6.LOG2)
    a6.scripted_sequence(wl, w6, c, c.commit, _runner(c, table), n=500 if mode == "base" else 300,
                         established=0.0 if mode == "base" else 0.4, dst_known=True)
    st = c.affinity_stats6()
    assert st["sweeps"] >= 5 and st["overflow"] == 0 and c.affinity_stats()["slots"] == 0


@pytest.mark.parametrize("per_key", [64, 1024])
def test_gpu_contention_one_key(pressure_keys, per_key):
    """One key carried by 64 and by 1024 packets of one batch (one wavefront; four blocks): exactly one
    GPC_LB_LEARNED, the key's first +new packet by caller index; every packet at or after it has its
    Endpoint, the ones before it their own choice. Identical to the emulation and the model."""
    wl, rules, c, svcs = a6.make_pressure_product()
    c.commit()
    key = pressure_keys.spread(0, 1)[0]
    batch = a6.key_batch(wl, svcs, [key], 251, per_key=per_key, established=0.5)
    cols = batch[1]
    cols["ct_state"][:3] = ac.gpc_ct("est")  # the first packets are not +new
    table = emu_aff6.Table6(a6.P_LOG2)
    lb, st, live = a6.Steps(rules, c, _runner(c, table), dst_known=True)("one key", batch, a6.T0)
    own = a6.own_choices(c, cols)
    first = a6.first_new(cols, np.arange(per_key))
    assert first >= 3 and list(np.nonzero(lb["flags"] & L)[0]) == [first]
    assert all(a6.ep_of(lb, i) == a6.ep_of(own, first) for i in range(first, per_key)) and ((lb["flags"][first:] & A) != 0).all()
    assert (lb[:first] == own[:first]).all()
    assert st["learned"] == st["live"] == 1 and st["hits"] == per_key - first - 1 and st["overflow"] == 0


def test_gpu_contention_many_keys_racing_into_a_small_table():
    """400 clients x 3 Services x 8 packets in one shuffled batch against 256 slots: lanes of 1 200 keys
    race for the slots. Which keys get one is decided by the race, so properties: a key is
    all-or-nothing -- a holder has exactly one learner, its first +new packet, and its Endpoint from
    there on; a loser's packets carry no flag and their own choices; the counters add up."""
    eps = lambda s: [{"ip": "fd00:10:128:%d::%x" % (s + 1, k), "port": 8000 + k, "is_local": False, "node_name": "n%d" % k}
                     for k in range(8)]
    c = gpc.Classifier(ipv4=True, ipv6=True, session_affinity6=8)
    c.initialize()
    wl = workload.config1(seed=81)
    c.batch_install_policy_rule_flows(copy.deepcopy(workload.to_ipv6(wl).rules))
    svc_ips = []
    for s in range(3):
        cfg = {"ip": "fd00:10:96::%x" % (0x100 + s), "port": 80, "protocol": "TCP", "cluster_group_id": 100 + 2 * s,
               "local_group_id": 101 + 2 * s, "affinity_timeout": 100}
        c.install_service_group(cfg["cluster_group_id"], eps(s), True)
        c.install_endpoint_flows("TCP", eps(s), 6)
        c.install_service_flows(cfg)
        svc_ips.append(a6.ip6(cfg["ip"]))
    c.commit()
    rng = np.random.default_rng(252)
    n_keys, per = 1200, 8
    n = n_keys * per
    k = rng.permutation(np.repeat(np.arange(n_keys), per))
    cols = workload.packets_to_v6(workload.gen_packets(wl, n, seed=252))
    cols["src6"] = np.array([a6.b16(a6.ip6("2001:db8:c::") + (j // 3)) for j in range(n_keys)], np.uint8)[k]
    cols["dst6"] = np.array([a6.b16(svc_ips[j % 3]) for j in range(n_keys)], np.uint8)[k]
    cols["dport"], cols["proto"] = np.full(n, 80, np.uint16), np.full(n, 6, np.uint8)
    cols["sport"] = rng.integers(1024, 65536, size=n).astype(np.uint16)
    cols["ct_state"] = np.where(rng.random(n) < 0.3, ac.gpc_ct("est"), ac.gpc_ct("new")).astype(np.uint8)
    own = a6.own_choices(c, cols)
    c.set_affinity_clock(50)
    _, lb = c.classify6_host(cols, lb=True)
    new = (cols["ct_state"] & 1) != 0
    holders = lost_new = hits = 0
    for j in range(n_keys):
        idx = np.nonzero(k == j)[0]
        if not new[idx].any():
            assert (lb[idx] == own[idx]).all()
            continue
        first = idx[new[idx]][0]
        learned = idx[(lb["flags"][idx] & L) != 0]
        if len(learned):
            assert list(learned) == [first]
            after, before = idx[idx >= first], idx[idx < first]
            assert all(a6.ep_of(lb, i) == a6.ep_of(own, first) for i in after) and ((lb["flags"][after] & A) != 0).all()
            assert (lb[before] == own[before]).all()
            holders += 1
            hits += len(after) - 1
        else:
            assert (lb[idx] == own[idx]).all() and ((lb["flags"][idx] & (A | L)) == 0).all()
            lost_new += int(new[idx].sum())
    st = c.affinity_stats6()
    assert 150 < holders <= 256 and lost_new > 1000
    assert st == {"slots": 256, "live": holders, "learned": holders, "hits": hits, "overflow": lost_new, "sweeps": 0}
    ent = _entries(c)
    assert len(ent) == holders == len({(e[0], e[2]) for e in ent})


# ------------------------------------------------------------------ the table under hash pressure
@pytest.fixture(scope="module")
def pressure_keys():
    wl, rules, c, svcs = a6.make_pressure_product()
    c.commit()
    return a6.KeySet(c)


def _pressure(bits=None, **kw):
    wl, rules, c, svcs = a6.make_pressure_product(bits=bits, **kw)
    c.commit()
    return wl, rules, c, svcs, emu_aff6.Table6(a6.P_LOG2, bits=bits or 64)


def test_gpu_colliding_keys_in_one_batch(pressure_keys):
    wl, rules, c, svcs, table = _pressure()
    a6.case_collisions(wl, rules, c, svcs, pressure_keys, _runner(c, table), 0, dst_known=True)


def test_gpu_live_key_behind_an_emptied_bucket(pressure_keys):
    wl, rules, c, svcs, table = _pressure()
    a6.case_emptied_bucket(wl, rules, c, svcs, pressure_keys, _runner(c, table), 0, dst_known=True)
    assert c.affinity_stats6()["overflow"] == 0


def test_gpu_full_bucket_forced_order(pressure_keys):
    wl, rules, c, svcs, table = _pressure()
    a6.case_full_bucket_forced(wl, rules, c, svcs, pressure_keys, _runner(c, table), 0)


def test_gpu_digest_collisions():
    """The claim digest narrowed to 8 bits by gpc_debug_set_affinity6_digest_bits: two clients of one
    Service with one digest never share an entry (tests/affinity6_cases.py case_digest_collisions)."""
    wl, rules, c, svcs, table = _pressure(bits=8)
    a6.case_digest_collisions(wl, rules, c, svcs, a6.KeySet(c, bits=8), _runner(c, table), 0)
    with pytest.raises(gpc.GpcError) as e:  # the table exists: claims of another width may be in it
        c.debug_set_affinity6_digest_bits(64)
    assert e.value.code == gpc.GPC_EINVAL


def test_gpu_launch_sequence_wrap(pressure_keys):
    wl, rules, c, svcs, table = _pressure()
    with pytest.raises(gpc.GpcError) as e:  # no table yet: its first use would restart the sequence
        c.debug_set_affinity_seq6(5)
    assert e.value.code == gpc.GPC_EINVAL

    def set_seq(seq):
        c.debug_set_affinity_seq6(seq)
        table.set_seq(seq)
    a6.case_sequence_wrap(wl, rules, c, svcs, pressure_keys, _runner(c, table), set_seq, 0, dst_known=True)
    assert c.affinity_stats6()["overflow"] == 0 and table.seq == 2


def test_gpu_two_streams_are_ordered_by_the_library(pressure_keys):
    """Two batches that share keys, issued back to back on different streams with no ordering of the
    caller's: the result is that of running them in issue order."""
    import torch
    wl, rules, c, svcs, table = _pressure()
    keys = pressure_keys.spread(0, 30)
    dev = torch.device("cuda", 0)
    b = [a6.key_batch(wl, svcs, keys, 260 + j, established=0.2)[1] for j in range(2)]
    n = len(b[0]["dport"])
    d = [_upload(x, dev) for x in b]
    outs = [torch.zeros(16 * n, dtype=torch.uint8, device=dev) for _ in range(2)]
    lbs = [torch.zeros(32 * n, dtype=torch.uint8, device=dev) for _ in range(2)]
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    torch.cuda.synchronize(dev)
    c.set_affinity_clock(700)
    for j in range(2):
        c.classify6_lb_device(gpc.pkt_soa_device(d[j]), n, outs[j].data_ptr(), lbs[j].data_ptr(), stream=streams[j].cuda_stream)
    torch.cuda.synchronize(dev)
    for j in range(2):
        elb = np.zeros(n, gpc.LB6_DTYPE)
        want = table.classify6(c, b[j], 700, lb=elb)
        assert (outs[j].cpu().numpy().view(gpc.VERDICT_DTYPE).reshape(n, 2) == want).all(), j
        assert (lbs[j].cpu().numpy().view(gpc.LB6_DTYPE) == elb).all(), j
    lb1 = lbs[1].cpu().numpy().view(gpc.LB6_DTYPE)
    assert ((lb1["flags"] & L) != 0).sum() == 0 and ((lb1["flags"] & A) != 0).all()  # the second batch found the first one's entries
    assert c.affinity_stats6() == table.stats(700)


def test_gpu_tables_are_per_slot(pressure_keys):
    """Two device slots on one GPU: what slot 0 learned is unknown to slot 1, which learns the same
    batch again; each slot equals an emulated table of its own."""
    wl, rules, c, svcs, t0 = _pressure(devices=[0, 0])
    t1 = emu_aff6.Table6(a6.P_LOG2)
    keys = pressure_keys.shared + pressure_keys.degenerate
    ac.check_no_overflow(keys)
    cols = a6.key_batch(wl, svcs, keys, 241)[1]
    index = a6.key_index(cols, svcs, keys)

    def run(slot, table, batch, now):
        c.set_affinity_clock(now)
        got, lb = _dev6(c, batch, slot=slot)
        elb = np.zeros(len(lb), gpc.LB6_DTYPE)
        assert (got == table.classify6(c, batch, now, lb=elb)).all() and (lb == elb).all(), slot
        assert c.affinity_stats6(slot) == table.stats(now), slot
        assert sorted(e[:2] + e[3:] for e in _entries(c, slot)) == _emulated(table, now), slot
        return lb
    lb0 = run(0, t0, cols, a6.T0)
    bound = a6.learned_endpoints(cols, lb0, index)
    assert c.affinity_stats6(1)["learned"] == 0 and len(c.affinity_table6(1)) == 0
    lb1 = run(1, t1, cols, a6.T0)
    assert (lb1 == lb0).all() and a6.learned_endpoints(cols, lb1, index) == bound  # its own LEARNED packets
    again = a6.key_batch(wl, svcs, keys, 242)[1]
    a6.check_all_hits(run(0, t0, again, a6.T0 + 1), a6.key_index(again, svcs, keys), bound)
    assert c.affinity_stats6(0)["learned"] == c.affinity_stats6(1)["learned"] == len(keys)


def test_gpu_replay_clears_the_table_and_restarts_the_counters(pressure_keys):
    wl, rules, c, svcs, table = _pressure()
    keys = pressure_keys.spread(1, 20)
    cols = a6.key_batch(wl, svcs, keys, 271)[1]
    run = _runner(c, table)
    run("before", cols, a6.T0)
    assert c.affinity_stats6()["live"] == 20
    c.replay()
    assert c.affinity_stats6() == {"slots": 256, "live": 0, "learned": 0, "hits": 0, "overflow": 0, "sweeps": 0}
    assert len(c.affinity_table6()) == 0
    fresh = emu_aff6.Table6(a6.P_LOG2)
    got, lb, live, st, n_all = _runner(c, fresh)("after", cols, a6.T0 + 1)
    assert st["learned"] == 20 and ((lb["flags"] & L) != 0).sum() == 20  # everything is learned again


def test_gpu_no_affinity_service_no_aff6_launch():
    """The table configured, no IPv6 affinity Service committed: the launch timing lists no aff6_*
    kernel but v6_lb, and the outputs are those of a context without the field; with an affinity
    Service aff6_learn / aff6_resolve take v6_lb's place, aff6_sweep once the clock has moved."""
    from tests.test_service6 import product6, svc_workload6
    wl, w6 = svc_workload6("C1np", 72)
    cols6 = workload.service_packets_to_v6(workload.gen_packets(wl, 2000, seed=72))
    res = []
    for log2 in (12, 0):
        c = product6(w6, session_affinity6=log2)
        c.commit()
        c.set_launch_timing(8)
        res.append(c.classify6_host(cols6, lb=True))
        kinds = set(c.launch_times())
        assert "v6_lb" in kinds and "v6_codes" in kinds and not any(k.startswith("aff") for k in kinds), kinds
        assert c.affinity_stats6()["live"] == 0 and len(c.affinity_table6()) == 0
    assert (res[0][0] == res[1][0]).all() and (res[0][1] == res[1][1]).all()
    assert (res[0][1]["flags"] & gpc.LB_HIT).mean() > 0.3
    wl2, w62 = a6.make_workload(83)
    c = a6.make_product(w62)
    c.commit()
    c.set_launch_timing(8)
    b = a6.make_batch(wl2, 1000, 84)[1]
    c.set_affinity_clock(5)
    c.classify6_host(b)
    kinds = set(c.launch_times())
    assert {"aff6_learn", "aff6_resolve", "v6_codes"} <= kinds and not {"aff6_sweep", "v6_lb"} & kinds, kinds
    c.set_affinity_clock(6)
    c.classify6_host(b)
    kinds = set(c.launch_times())
    assert {"aff6_learn", "aff6_resolve", "aff6_sweep"} <= kinds and not any(k.startswith("aff_") for k in kinds), kinds


def test_gpu_dual_stack_tables_do_not_see_each_other():
    """One context, one slot, both tables: an IPv4 affinity batch and the same packets as an IPv6
    affinity batch. Each family equals its own emulated table; neither table holds the other's entries."""
    wl, w6 = a6.make_workload(87)
    w6.groups = {g + 1000: e for g, e in w6.groups.items()}
    w6.affinity_groups = {g + 1000 for g in w6.affinity_groups}
    w6.services = [dict(s, cluster_group_id=s["cluster_group_id"] + 1000, local_group_id=s["local_group_id"] + 1000)
                   for s in w6.services]
    dual = workload.to_ipv6(wl, dual=True)
    wl4 = copy.copy(wl)
    wl4.rules = w6.rules = dual.rules
    c = gpc.Classifier(ipv4=True, ipv6=True, session_affinity=10, session_affinity6=11)
    c.initialize()
    c.batch_install_policy_rule_flows(copy.deepcopy(dual.rules))
    workload.install_services(c, w6)
    workload.install_services(c, wl4)
    c.commit()
    cols, cols6 = a6.make_batch(wl, 600, 88, established=0.3)
    t4, t6 = emu_aff.Table(10), emu_aff6.Table6(11)
    for now in (100, 101):
        c.set_affinity_clock(now)
        got, lb = c.classify_host(cols, lb=True)
        elb = np.zeros(600, gpc.LB_DTYPE)
        _cmp(got, t4.classify(c, cols, now, lb=elb), cols)
        assert (lb == elb).all() and c.affinity_stats() == t4.stats(now)
        got6, lb6 = c.classify6_host(cols6, lb=True)
        elb6 = np.zeros(600, gpc.LB6_DTYPE)
        assert (got6 == t6.classify6(c, cols6, now, lb=elb6)).all() and (lb6 == elb6).all()
        assert c.affinity_stats6() == t6.stats(now) and c.affinity_stats() == t4.stats(now)
    s4, s6 = c.affinity_stats(), c.affinity_stats6()
    assert s4["slots"] == 1024 and s6["slots"] == 2048 and s4["live"] > 20 and s6["live"] > 20
    assert len(c.affinity_table()) == s4["live"] and len(c.affinity_table6()) == s6["live"]
    ids4, ids6 = emu_aff.install_ids(c), emu_aff6.install_ids(c)
    assert ids4 and ids6 and not ids4 & ids6  # one sequence of install ids over both families
    assert {int(e["install_id"]) for e in c.affinity_table()} <= ids4
    assert {int(e["install_id"]) for e in c.affinity_table6()} <= ids6
