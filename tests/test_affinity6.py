"""Session affinity of IPv6 Services (gpc_config.session_affinity6), CPU tier: the learn flow's text
against the reference's goldens (client_test.go "Service ClusterIP,IPv6,SessionAffinity" and "Service
NodePort,IPv6,SessionAffinity", transcribed in tests/golden/service_flows_affinity_v6.json), the
ABI's argument checks, the IPv6 Service image, and the host emulation of the learn / resolve / sweep
bodies of core.hpp (tests/emu_aff6.py) against the model that executes the realized learn flows
serially (tests/affinity6_model.py) and, under the /96 embedding, against the IPv4 emulation."""
import ctypes as C

import numpy as np
import pytest

from antrea_amd import gpc, workload
from tests import affinity6_cases as a6
from tests import affinity_cases as ac
from tests import emu, emu_aff, emu_aff6
from tests.util import load_golden

GOLD = load_golden("service_flows_affinity_v6.json")
GOLD4 = load_golden("service_flows_affinity.json")


@pytest.mark.parametrize("case", GOLD["service_flows"], ids=[c["name"] for c in GOLD["service_flows"]])
def test_affinity6_service_flows_golden(case):
    c = gpc.Classifier(ipv6=True, session_affinity6=12)
    c.install_service_flows(case["config"])
    assert c.dump_flows() == case["expected"]
    cfg = case["config"]
    c.uninstall_service_flows(cfg["ip"], cfg["port"], cfg["protocol"])
    assert c.dump_flows() == []


@pytest.mark.parametrize("log2", [7, 27, -1, 1])
def test_table_size_out_of_range_fails_create(log2):
    with pytest.raises(gpc.GpcError) as e:
        gpc.Classifier(ipv6=True, session_affinity6=log2)
    assert e.value.code == gpc.GPC_EINVAL


@pytest.mark.parametrize("log2", [8, 26])
def test_table_size_bounds_accepted(log2):
    c = gpc.Classifier(ipv6=True, session_affinity6=log2)
    assert c.affinity_stats6()["slots"] == 1 << log2 and c.affinity_stats()["slots"] == 0  # (nothing is allocated yet)
    assert len(c.affinity_table6()) == 0


def test_the_two_fields_gate_their_own_family():
    cfg4, cfg6 = GOLD4["service_flows"][0]["config"], GOLD["service_flows"][0]["config"]
    for kw, ok4, ok6 in ((dict(session_affinity6=12), False, True), (dict(session_affinity=12), True, False),
                         (dict(session_affinity=12, session_affinity6=9), True, True), ({}, False, False)):
        for cfg, ok in ((cfg4, ok4), (cfg6, ok6)):
            c = gpc.Classifier(ipv6=True, **kw)
            if ok:
                c.install_service_flows(cfg)
                assert sum("priority=190" in f for f in c.dump_flows()) == 1
            else:
                with pytest.raises(gpc.GpcError) as e:
                    c.install_service_flows(cfg)
                assert e.value.code == gpc.GPC_EINVAL and c.dump_flows() == []
                c.install_service_flows(dict(cfg, affinity_timeout=0))  # the same Service without affinity is fine


def test_test_hooks_check_their_arguments():
    c = gpc.Classifier(ipv6=True, session_affinity6=8)
    for bits in (0, 65):
        assert c.lib.gpc_debug_set_affinity6_digest_bits(c.h, 0, bits) == -gpc.GPC_EINVAL
    assert c.lib.gpc_debug_set_affinity6_digest_bits(c.h, 1, 8) == -gpc.GPC_EINVAL
    assert c.lib.gpc_debug_set_affinity6_digest_bits(c.h, 0, 8) == 0
    assert c.lib.gpc_debug_set_affinity_seq6(c.h, 0, 5) == -gpc.GPC_EINVAL  # no table yet
    off = gpc.Classifier(ipv6=True, session_affinity=8)
    assert off.lib.gpc_debug_set_affinity6_digest_bits(off.h, 0, 8) == -gpc.GPC_EINVAL
    assert off.lib.gpc_debug_set_affinity_seq6(off.h, 0, 5) == -gpc.GPC_EINVAL
    assert off.affinity_stats6()["slots"] == 0


def _image(c, six):
    b, n = C.POINTER(C.c_uint32)(), C.c_size_t()
    fn = c.lib.gpc_debug_service_image6 if six else c.lib.gpc_debug_service_image
    assert fn(c.h, C.byref(b), C.byref(n)) == 0
    return np.ctypeslib.as_array(b, shape=(n.value,)).copy() if n.value else np.zeros(0, np.uint32)


@pytest.mark.parametrize("name,seed", [("C1", 51), ("C1np", 54)])
def test_images_without_v6_affinity_service_are_byte_identical(name, seed):
    """An IPv6 Service image without an affinity Service is the same with the field on and off (the
    affinity words exist only in an image that holds an affinity Service), and the field never touches
    the IPv4 image -- here one with IPv4 affinity Services, in a dual-stack context."""
    from tests.test_service6 import product6, svc_workload6
    blobs = []
    for log2 in (0, 12):
        wl, w6 = svc_workload6(name, seed, gid_offset=1000)
        wl4 = ac.make_workload(seed)
        c = product6(w6, extra=wl4, session_affinity=10, session_affinity6=log2)
        emu.commit_host(c)
        blobs.append((_image(c, True), _image(c, False)))
    assert len(blobs[0][0]) > 100 and np.array_equal(blobs[0][0], blobs[1][0])
    assert len(blobs[0][1]) > 100 and np.array_equal(blobs[0][1], blobs[1][1])
    assert not emu_aff6.load().emu_aff6_image(blobs[1][0].ctypes.data) and emu_aff.load().emu_aff_image(blobs[1][1].ctypes.data)


def test_group_with_affinity_buckets_needs_a_learn_flow():
    """Both commit-time errors stay: a group whose buckets resubmit to ServiceLB under a ServiceLB flow
    without a learn flow, and an affinity Service whose group bypasses the learn flow."""
    eps = [{"ip": "fec0:10:10::100", "port": 8080, "is_local": False, "node_name": "n1"}]
    cfg = dict(GOLD["service_flows"][0]["config"])
    for svc_aff, grp_aff in ((False, True), (True, False)):
        c = gpc.Classifier(ipv6=True, session_affinity6=12)
        c.initialize()
        c.install_service_group(cfg["cluster_group_id"], eps, grp_aff)
        c.install_service_flows(dict(cfg, affinity_timeout=100 if svc_aff else 0))
        assert c.lib.gpc_commit(c.h) == -gpc.GPC_EINVAL
    c = gpc.Classifier(ipv6=True, session_affinity6=12)
    c.initialize()
    c.install_service_group(cfg["cluster_group_id"], eps, True)
    c.install_service_flows(cfg)
    emu.commit_host(c)
    assert emu_aff6.load().emu_aff6_image(c.debug_service_image6())
    assert [(i, g, t) for i, g, t in emu_aff6.affinity_services(c)] == [(1, 100, 100)]


def test_services_to_ipv6_carries_affinity_over():
    wl = ac.make_workload(71)
    w6 = workload.services_to_ipv6(wl)
    assert w6.affinity_groups == wl.affinity_groups and len(w6.affinity_groups) > 10
    assert [s.get("affinity_timeout") for s in w6.services] == [s.get("affinity_timeout") for s in wl.services]
    plain = workload.add_services(workload.config1(seed=51), 60, 4, seed=51)
    assert not hasattr(workload.services_to_ipv6(plain), "affinity_groups")


def _emu_runner(clf, table):
    def run(name, cols, now):
        lb = np.zeros(len(cols["dport"]), gpc.LB6_DTYPE)
        v = table.classify6(clf, cols, now, lb=lb)
        live = table.live(now)
        ids = emu_aff6.install_ids(clf)
        return v, lb, [e for e in live if (e[1] >> 8) in ids], table.stats(now), len(live)
    return run


@pytest.mark.parametrize("established", [0.0, 0.5], ids=["all_new", "first_packets_not_new"])
def test_emulation_equals_model_over_the_scripted_sequence(established):
    wl, w6 = a6.make_workload(71)
    clf = a6.make_product(w6, compact_after=-1)
    table = emu_aff6.Table6(a6.LOG2)
    a6.scripted_sequence(wl, w6, clf, lambda: emu.commit_host(clf), _emu_runner(clf, table), established=established)
    st = table.stats(a6.T0 + a6.T + 3)
    assert st["sweeps"] >= 5 and st["hits"] > st["learned"] > 0 and st["overflow"] == 0


def test_metamorphic_vs_the_ipv4_emulation():
    """The /96 embedding of the affinity workload: batch by batch the IPv6 emulation gives the IPv4
    emulation's verdicts, Endpoint choices, flags, counters and live-entry set, addresses embedded --
    the bucket hash over the folded addresses is the IPv4 hash there."""
    wl, w6 = a6.make_workload(72)
    c4 = ac.make_product(wl, compact_after=-1)
    c6 = a6.make_product(w6, compact_after=-1)
    emu.commit_host(c4), emu.commit_host(c6)
    t4, t6 = emu_aff.Table(a6.LOG2), emu_aff6.Table6(a6.LOG2)
    n = 500
    e = lambda a: workload.v6_embed(int(a))
    seen_learn = seen_hit = 0
    for k, now in enumerate((a6.T0, a6.T0 + 1, a6.T0 + 50, a6.T0 + a6.T, a6.T0 + a6.T + 1)):
        cols, cols6 = a6.make_batch(wl, n, 7 + k // 2, established=0.3, embedded_only=True)  # (batches repeat: hits)
        lb4, lb6 = np.zeros(n, gpc.LB_DTYPE), np.zeros(n, gpc.LB6_DTYPE)
        v4, v6 = t4.classify(c4, cols, now, lb=lb4), t6.classify6(c6, cols6, now, lb=lb6)
        assert (v4 == v6).all(), now
        for f in ("endpoint_port", "flags", "group_id", "out_port"):
            assert (lb6[f] == lb4[f]).all(), (now, f)
        sel = lb4["endpoint_ip"] != 0
        assert (lb6["endpoint_ip"][sel] == workload.v6_bytes(lb4["endpoint_ip"][sel])).all() and (lb6["endpoint_ip"][~sel] == 0).all()
        assert t4.stats(now) == t6.stats(now)
        live4 = sorted((e(s), e(ip), port, exp) for s, _, ip, port, exp in t4.live(now))
        assert live4 == sorted((s, ip, port, exp) for s, _, ip, port, exp in t6.live(now)) and live4
        seen_learn += int(((lb4["flags"] & gpc.LB_LEARNED) != 0).sum())
        seen_hit += int(((lb4["flags"] & a6.FLAGS) == gpc.LB_AFFINITY).sum())
    assert seen_learn > 60 and seen_hit > 100  # (the batches exercise both branches)
    assert emu_aff6.fold(str(__import__("ipaddress").IPv6Address(e(0x0a000001)))) ^ emu_aff6.fold(
        str(__import__("ipaddress").IPv6Address(e(0x0a000002)))) == 0x0a000001 ^ 0x0a000002


def _one_service(log2=8, bits=None):
    eps = [{"ip": "fec0:10:10::%x" % (0x100 + k), "port": 8080, "is_local": False, "node_name": "n1"} for k in range(8)]
    cfg = dict(GOLD["service_flows"][0]["config"])
    c = gpc.Classifier(ipv6=True, session_affinity6=log2)
    c.initialize()
    c.install_service_group(cfg["cluster_group_id"], eps, True)
    c.install_endpoint_flows("TCP", eps, 6)
    c.install_service_flows(cfg)
    if bits:
        c.debug_set_affinity6_digest_bits(bits)
    emu.commit_host(c)
    return c, cfg


def _client_batch(cfg, clients, per, seed, state="new"):
    n = len(clients) * per
    k = np.repeat(np.arange(len(clients)), per)
    rng = np.random.default_rng(seed)
    cols = {"src6": np.array([a6.b16(a6.ip6(a)) for a in clients], np.uint8)[k],
            "dst6": np.tile(a6.b16(a6.ip6(cfg["ip"])), (n, 1)), "sport": rng.integers(1024, 65536, size=n).astype(np.uint16),
            "dport": np.full(n, 80, np.uint16), "proto": np.full(n, 6, np.uint8), "out_port": np.zeros(n, np.uint32),
            "ct_state": np.full(n, ac.gpc_ct(state), np.uint8)}
    perm = rng.permutation(n)
    return {f: np.ascontiguousarray(v[perm]) for f, v in cols.items()}, k[perm]


def test_keys_beyond_the_embedding_are_distinct():
    """Clients that differ only in their upper 96 bits, and clients with equal fold6 (the bucket hash
    cannot tell them apart: the digest must), are distinct keys: one entry and one LEARNED packet each,
    every client bound to the choice of its own first packet."""
    c, cfg = _one_service()
    low = "::aabb:ccdd"
    upper = ["2001:db8:%x%s" % (k + 1, low) for k in range(6)]
    base = a6.ip6("2001:db8:77::1")
    same_fold = [str(__import__("ipaddress").IPv6Address(base ^ (x << 96) ^ (x << 32))) for x in (0, 0x1111, 0x2222, 0xabcdef)]
    assert len({emu_aff6.fold(a) for a in same_fold}) == 1
    clients = upper + same_fold
    cols, who = _client_batch(cfg, clients, 20, 5)
    own = a6.own_choices(c, cols)
    table = emu_aff6.Table6(8)
    lb = np.zeros(len(who), gpc.LB6_DTYPE)
    table.classify6(c, cols, 10, lb=lb)
    st = table.stats(10)
    assert st == {"slots": 256, "live": len(clients), "learned": len(clients), "hits": len(who) - len(clients), "overflow": 0,
                  "sweeps": 0}
    assert sorted(e[0] for e in table.live(10)) == sorted(a6.ip6(a) for a in clients)
    eps = set()
    for j in range(len(clients)):
        idx = np.nonzero(who == j)[0]
        assert [int(f) & a6.FLAGS for f in lb["flags"][idx]] == [a6.FLAGS] + [gpc.LB_AFFINITY] * (len(idx) - 1)
        assert all(a6.ep_of(lb, i) == a6.ep_of(own, idx[0]) for i in idx)
        eps.add(a6.ep_of(own, idx[0]))
    assert len(eps) >= 4, "the clients' first choices must differ, or shared entries would not show"
    # +est packets alone hit; past the timeout the entries are gone and nothing is learned from +est
    cols2, who2 = _client_batch(cfg, clients, 5, 6, state="est")
    lb2 = np.zeros(len(who2), gpc.LB6_DTYPE)
    table.classify6(c, cols2, 109, lb=lb2)
    assert ((lb2["flags"] & a6.FLAGS) == gpc.LB_AFFINITY).all()
    table.classify6(c, cols2, 110, lb=lb2)
    assert ((lb2["flags"] & a6.FLAGS) == 0).all() and table.live(110) == [] and (lb2 == a6.own_choices(c, cols2)).all()


def test_small_table_overflows_and_reuses_swept_slots():
    c, cfg = _one_service()
    clients = ["2001:db8:5::%x" % (k + 1) for k in range(2000)]
    cols, who = _client_batch(cfg, clients, 1, 8)
    table = emu_aff6.Table6(8)
    lb = np.zeros(2000, gpc.LB6_DTYPE)
    table.classify6(c, cols, 10, lb=lb)
    st = table.stats(10)
    assert st["overflow"] > 0 and st["live"] <= 256 and st["learned"] == st["live"] and st["learned"] + st["overflow"] == 2000
    learned = (lb["flags"] & gpc.LB_LEARNED) != 0
    cols2 = dict(cols, sport=(cols["sport"] + 7).astype(np.uint16))
    lb2 = np.zeros(2000, gpc.LB6_DTYPE)
    table.classify6(c, cols2, 11, lb=lb2)
    assert (lb2[["endpoint_ip", "endpoint_port"]][learned] == lb[["endpoint_ip", "endpoint_port"]][learned]).all()
    assert ((lb2["flags"][learned] & a6.FLAGS) == gpc.LB_AFFINITY).all()
    over = table.stats(11)["overflow"]
    # 40 new clients that share no bucket (checked with the product's hash: they cannot overflow)
    pool = ["2001:db8:6::%x" % (k + 1) for k in range(600)]
    _, cand = emu_aff6.candidates(emu_aff6.affinity_services(c)[0][0], pool, 8)
    fresh, used = [], set()
    for a, cs in zip(pool, cand):
        b = {int(cs[0]) >> 1, int(cs[2]) >> 1}
        if len(fresh) < 40 and not b & used:
            used |= b
            fresh.append(a)
    assert len(fresh) == 40
    cols3, _ = _client_batch(cfg, fresh, 1, 9)
    table.classify6(c, cols3, 110, lb=np.zeros(40, gpc.LB6_DTYPE))
    st = table.stats(110)
    assert st["overflow"] == over and st["live"] == 40


# ------------------------------------------------------------------ the table under hash pressure
# Emulation == model for three shuffles of every batch; shuffle 2 runs the learn pass with stale
# finds (emu_aff6.cpp AffOpsStale).
ORDERS = [0, 1, 2]


@pytest.fixture(scope="module")
def pressure_keys():
    wl, rules, clf, svcs = a6.make_pressure_product()
    emu.commit_host(clf)
    return a6.KeySet(clf)


def _pressure(order, bits=64):
    wl, rules, clf, svcs = a6.make_pressure_product()
    emu.commit_host(clf)
    return wl, rules, clf, svcs, emu_aff6.Table6(a6.P_LOG2, stale_find=order == 2, bits=bits)


def test_candidates_are_the_products_hash(pressure_keys):
    ks = pressure_keys
    assert ks.install[0] != ks.install[1] and all(ks.install)
    wl, rules, clf, svcs, table = _pressure(0)
    keys = ks.spread(1, 40)
    table.classify6(clf, a6.key_batch(wl, svcs, keys, 3, per_key=2, established=0.0)[1], 10)
    assert all(a6.slot_of(table.tab, k) == [k.c[0]] for k in keys)  # nothing in the way: the first candidate
    assert len({k.c[0] for k in ks.shared}) == 1 and len({k.c[2] for k in ks.shared}) == 4
    d, e = ks.degenerate
    assert d.c[:2] == d.c[2:] and e.c[:2] == d.c[:2] and e.c[2] != e.c[0]
    assert len(ac.neighbours(ks.shared[0], ks.exact_keys())) == 3 and len(ac.neighbours(ks.identical[0], ks.identical)) == 5


@pytest.mark.parametrize("order", ORDERS)
def test_colliding_keys_in_one_batch(pressure_keys, order):
    wl, rules, clf, svcs, table = _pressure(order)
    a6.case_collisions(wl, rules, clf, svcs, pressure_keys, _emu_runner(clf, table), order, tab=lambda: table.tab)


@pytest.mark.parametrize("order", ORDERS)
def test_live_key_behind_an_emptied_bucket(pressure_keys, order):
    wl, rules, clf, svcs, table = _pressure(order)
    a6.case_emptied_bucket(wl, rules, clf, svcs, pressure_keys, _emu_runner(clf, table), order, tab=lambda: table.tab)


@pytest.mark.parametrize("order", ORDERS)
def test_full_bucket_forced_order(pressure_keys, order):
    wl, rules, clf, svcs, table = _pressure(order)
    a6.case_full_bucket_forced(wl, rules, clf, svcs, pressure_keys, _emu_runner(clf, table), order)


@pytest.mark.parametrize("order", ORDERS)
def test_launch_sequence_wrap(pressure_keys, order):
    wl, rules, clf, svcs, table = _pressure(order)
    a6.case_sequence_wrap(wl, rules, clf, svcs, pressure_keys, _emu_runner(clf, table), table.set_seq, order)
    assert table.seq == 2


@pytest.mark.parametrize("order", ORDERS)
def test_digest_collisions(order):
    wl, rules, clf, svcs, table = _pressure(order, bits=8)
    a6.case_digest_collisions(wl, rules, clf, svcs, a6.KeySet(clf, bits=8), _emu_runner(clf, table), order)
