"""Session affinity of IPv4 Services (sessionAffinity: ClientIP), CPU tier: the learn flow's text
against the reference's goldens (client_test.go "Service ClusterIP,SessionAffinity" and "Service
NodePort,SessionAffinity", transcribed in tests/golden/service_flows_affinity.json), the ABI's
argument checks, the Service image, and the host emulation of the learn / resolve / sweep bodies of
core.hpp (tests/emu_aff.py) against the model that executes the realized learn flows serially
(tests/affinity_model.py)."""
import copy
import ctypes as C

import numpy as np
import pytest

from antrea_amd import gpc, workload
from tests import affinity_cases as ac
from tests import emu, emu_aff
from tests.util import load_golden

GOLD = load_golden("service_flows_affinity.json")


@pytest.mark.parametrize("case", GOLD["service_flows"], ids=[c["name"] for c in GOLD["service_flows"]])
def test_affinity_service_flows_golden(case):
    c = gpc.Classifier(session_affinity=12)
    c.install_service_flows(case["config"])
    assert c.dump_flows() == case["expected"]
    cfg = case["config"]
    c.uninstall_service_flows(cfg["ip"], cfg["port"], cfg["protocol"])
    assert c.dump_flows() == []


def test_affinity_config_rejected_with_the_feature_off():
    with pytest.raises(gpc.GpcError) as e:
        gpc.Classifier(session_affinity=0).install_service_flows(GOLD["service_flows"][0]["config"])
    assert e.value.code == gpc.GPC_EINVAL


@pytest.mark.parametrize("log2", [7, 27, -1, 1])
def test_table_size_out_of_range_fails_create(log2):
    with pytest.raises(gpc.GpcError) as e:
        gpc.Classifier(session_affinity=log2)
    assert e.value.code == gpc.GPC_EINVAL


@pytest.mark.parametrize("log2", [8, 26])
def test_table_size_bounds_accepted(log2):
    assert gpc.Classifier(session_affinity=log2).affinity_stats()["slots"] == 1 << log2  # (nothing is allocated yet)


def test_family6_affinity_config_rejected_with_the_feature_on():
    c = gpc.Classifier(ipv6=True, session_affinity=12)
    cfg = dict(GOLD["service_flows"][0]["config"], ip="fec0:10:96::100")
    with pytest.raises(gpc.GpcError) as e:
        c.install_service_flows(cfg)
    assert e.value.code == gpc.GPC_EINVAL
    c.install_service_flows(dict(cfg, affinity_timeout=0))  # the same Service without affinity is fine


def test_clock_is_monotonic():
    c = gpc.Classifier(session_affinity=12)
    c.set_affinity_clock(100)
    c.set_affinity_clock(100)
    c.set_affinity_clock(250)
    with pytest.raises(gpc.GpcError) as e:
        c.set_affinity_clock(249)
    assert e.value.code == gpc.GPC_EINVAL
    c.set_affinity_clock(250)


def _service_image(c):
    b = C.POINTER(C.c_uint32)()
    n = C.c_size_t()
    assert c.lib.gpc_debug_service_image(c.h, C.byref(b), C.byref(n)) == 0
    return np.ctypeslib.as_array(b, shape=(n.value,)).copy()


@pytest.mark.parametrize("name,seed", [("C1", 51), ("C1np", 54)])
def test_image_without_affinity_service_is_byte_identical(name, seed):
    """The existing Service workloads (tests/test_service.py) build the same image with the feature
    on and off: the affinity words exist only in an image that holds an affinity Service."""
    blobs = []
    for log2 in (0, 12):
        wl = workload.config1(seed=seed)
        wl = workload.add_services(wl, 60, 4, seed=seed, noep_frac=0.1, local_policy_frac=0.2,
                                   nodeport_frac=0.4 if name.endswith("np") else 0.0)
        c = gpc.Classifier(session_affinity=log2)
        c.initialize()
        workload.install_services(c, wl)
        emu.commit_host(c)
        blobs.append(_service_image(c))
    assert len(blobs[0]) > 100 and np.array_equal(blobs[0], blobs[1])


@pytest.mark.parametrize("seed", [51, 52, 53, 54, 61, 63, workload.RULE_SEED + 4])
def test_affinity_frac_draws_from_its_own_generator(seed):
    """add_services(affinity_frac=0) is the generator it always was: the affinity choices come from a
    separate stream, so turning them on changes nothing else of the workload (Services, groups,
    Endpoint flows, the packets' Service table) for the seeds the fixtures and tests use."""
    kw = dict(noep_frac=0.1, local_policy_frac=0.2, nodeport_frac=0.4)
    a = workload.add_services(workload.config1(seed=seed), 60, 4, seed=seed, **kw)
    z = workload.add_services(workload.config1(seed=seed), 60, 4, seed=seed, affinity_frac=0.0, **kw)
    b = workload.add_services(workload.config1(seed=seed), 60, 4, seed=seed, affinity_frac=0.4, affinity_timeout=30, **kw)
    assert a.services == z.services and not z.affinity_groups
    assert not any("affinity_timeout" in s for s in a.services)
    on = [s for s in b.services if s.get("affinity_timeout")]
    assert 10 < len(on) < 40 and all(s["affinity_timeout"] == 30 for s in on)
    assert [{k: v for k, v in s.items() if k != "affinity_timeout"} for s in b.services] == a.services
    assert a.groups == b.groups and a.endpoint_flows == b.endpoint_flows
    assert all(np.array_equal(a.svc_meta[k], b.svc_meta[k]) for k in a.svc_meta)
    assert len(b.affinity_groups) == len(on)


def test_group_with_affinity_buckets_needs_a_learn_flow():
    """A group whose buckets resubmit to ServiceLB under a ServiceLB flow without a learn flow is still
    an error at commit; so is an affinity Service whose group bypasses the learn flow."""
    eps = [{"ip": "10.10.0.100", "port": 8080, "is_local": False, "node_name": "n1"}]
    cfg = dict(GOLD["service_flows"][0]["config"])
    for svc_aff, grp_aff in ((False, True), (True, False)):
        c = gpc.Classifier(session_affinity=12)
        c.initialize()
        c.install_service_group(cfg["cluster_group_id"], eps, grp_aff)
        c.install_service_flows(dict(cfg, affinity_timeout=100 if svc_aff else 0))
        assert c.lib.gpc_commit(c.h) == -gpc.GPC_EINVAL
    c = gpc.Classifier(session_affinity=12)
    c.initialize()
    c.install_service_group(cfg["cluster_group_id"], eps, True)
    c.install_service_flows(cfg)
    emu.commit_host(c)
    assert emu_aff.load().emu_aff_image(c.debug_service_image())


def _emu_runner(clf, table):
    def run(name, cols, now):
        lb = np.zeros(len(cols["src"]), gpc.LB_DTYPE)
        v = table.classify(clf, cols, now, lb=lb)
        live = table.live(now)
        ids = emu_aff.install_ids(clf)
        return v, lb, [e for e in live if (e[1] >> 8) in ids], table.stats(now), len(live)
    return run


@pytest.mark.parametrize("established", [0.0, 0.5], ids=["all_new", "first_packets_not_new"])
def test_emulation_equals_model_over_the_scripted_sequence(established):
    """established = 0.5: half of the packets are +est, so many keys' first packets are not +new:
    they keep their own choice and learn nothing, the first +new packet of the key decides for the
    packets after it."""
    wl = ac.make_workload(71)
    clf = ac.make_product(wl, compact_after=-1)
    table = emu_aff.Table(ac.LOG2)
    ac.scripted_sequence(wl, clf, lambda: emu.commit_host(clf), _emu_runner(clf, table), established=established)
    st = table.stats(ac.T0 + ac.T + 3)
    assert st["sweeps"] >= 5 and st["hits"] > st["learned"] > 0


def test_earlier_non_new_packets_keep_their_own_choice():
    """One key, five packets with different source ports: est, est, new, est, new. The third decides:
    packets 3-5 take its Endpoint (only the third is LEARNED), packets 1-2 their own hash choice."""
    import ipaddress
    eps = [{"ip": "10.10.0.%d" % (100 + k), "port": 8080, "is_local": False, "node_name": "n1"} for k in range(8)]
    cfg = dict(GOLD["service_flows"][0]["config"])
    c = gpc.Classifier(session_affinity=8)
    c.initialize()
    c.install_service_group(cfg["cluster_group_id"], eps, True)
    c.install_endpoint_flows("TCP", eps)
    c.install_service_flows(cfg)
    emu.commit_host(c)
    n = 5
    cols = {"src": np.full(n, int(ipaddress.ip_address("10.10.0.5")), np.uint32),
            "dst": np.full(n, int(ipaddress.ip_address(cfg["ip"])), np.uint32),
            "sport": np.array([40001, 40002, 40003, 40004, 40005], np.uint16), "dport": np.full(n, 80, np.uint16),
            "proto": np.full(n, 6, np.uint8), "out_port": np.zeros(n, np.uint32),
            "ct_state": np.array([ac.gpc_ct(k) for k in ("est", "est", "new", "est", "new")], np.uint8)}
    own = np.zeros(n, gpc.LB_DTYPE)
    emu.classify(c, cols, lb=own)  # the plain Service stage: every packet's own hash choice
    assert len(set(own["endpoint_ip"])) > 2, "the ports must spread over the Endpoints"
    table = emu_aff.Table(8)
    lb = np.zeros(n, gpc.LB_DTYPE)
    table.classify(c, cols, 50, lb=lb)
    a, l = gpc.LB_AFFINITY, gpc.LB_LEARNED
    assert [int(f) & (a | l) for f in lb["flags"]] == [0, 0, a | l, a, a]
    assert list(lb["endpoint_ip"][:2]) == list(own["endpoint_ip"][:2])
    assert (lb["endpoint_ip"][2:] == own["endpoint_ip"][2]).all()
    assert table.stats(50) == {"slots": 256, "live": 1, "learned": 1, "hits": 2, "overflow": 0, "sweeps": 0}
    # a later batch of established packets alone hits the entry; past the timeout it is gone
    cols["ct_state"][:] = ac.gpc_ct("est")
    table.classify(c, cols, 149, lb=lb)
    assert (lb["endpoint_ip"] == own["endpoint_ip"][2]).all() and ((lb["flags"] & (a | l)) == a).all()
    table.classify(c, cols, 150, lb=lb)
    assert list(lb["endpoint_ip"]) == list(own["endpoint_ip"]) and ((lb["flags"] & (a | l)) == 0).all()
    assert table.live(150) == [] and table.stats(150)["live"] == 0


def test_small_table_overflows_and_reuses_swept_slots():
    """256 slots, 2 000 clients of one Service: keys that find no free slot are not learned and take
    their hash choice; keys that did get an entry hit it in the next batch; after the timeout the
    sweep has freed the slots and 100 new clients learn without a new overflow."""
    import ipaddress
    eps = [{"ip": "10.10.0.%d" % (100 + k), "port": 8080, "is_local": False, "node_name": "n1"} for k in range(4)]
    cfg = dict(GOLD["service_flows"][0]["config"])
    c = gpc.Classifier(session_affinity=8)
    c.initialize()
    c.install_service_group(cfg["cluster_group_id"], eps, True)
    c.install_service_flows(cfg)
    emu.commit_host(c)

    def batch(first, n):
        return {"src": (0x0a800000 + first + np.arange(n)).astype(np.uint32),
                "dst": np.full(n, int(ipaddress.ip_address(cfg["ip"])), np.uint32),
                "sport": (1024 + np.arange(n) % 60000).astype(np.uint16), "dport": np.full(n, 80, np.uint16),
                "proto": np.full(n, 6, np.uint8), "out_port": np.zeros(n, np.uint32)}
    table = emu_aff.Table(8)
    cols = batch(0, 2000)
    lb = np.zeros(2000, gpc.LB_DTYPE)
    table.classify(c, cols, 10, lb=lb)
    st = table.stats(10)
    assert st["overflow"] > 0 and st["live"] <= 256 and st["learned"] == st["live"] and st["learned"] + st["overflow"] == 2000
    ep_ips = {int(ipaddress.ip_address(e["ip"])) for e in eps}
    assert set(int(x) for x in lb["endpoint_ip"]) <= ep_ips
    learned = (lb["flags"] & gpc.LB_LEARNED) != 0
    lb2 = np.zeros(2000, gpc.LB_DTYPE)
    cols2 = dict(cols, sport=(cols["sport"] + 7).astype(np.uint16))  # other hash choices
    table.classify(c, cols2, 11, lb=lb2)
    assert (lb2["endpoint_ip"][learned] == lb["endpoint_ip"][learned]).all()
    assert ((lb2["flags"][learned] & (gpc.LB_AFFINITY | gpc.LB_LEARNED)) == gpc.LB_AFFINITY).all()
    over = table.stats(11)["overflow"]
    table.classify(c, batch(5000, 100), 10 + 100, lb=np.zeros(100, gpc.LB_DTYPE))
    st = table.stats(110)
    assert st["overflow"] == over and st["live"] == 100


# ------------------------------------------------------------------ the table under hash pressure
# (tests/affinity_cases.py KeySet: keys that share buckets in a table of 256 slots.) Emulation ==
# model for three shuffles of every batch: which slot a key lands in depends on the order, the results
# must not. Shuffle 2 runs the learn pass with stale finds (emu_aff.cpp AffOpsStale). The per-rule
# counters are the device's against the emulation's in the GPU tier; the model has none.
ORDERS = [0, 1, 2]


@pytest.fixture(scope="module")
def pressure_keys():
    wl, clf, svcs = ac.make_pressure_product()
    emu.commit_host(clf)
    return ac.KeySet(clf)


def _pressure(order):
    wl, clf, svcs = ac.make_pressure_product()
    emu.commit_host(clf)
    table = emu_aff.Table(ac.P_LOG2, stale_find=order == 2)
    return wl, clf, svcs, table


def test_candidates_are_the_products_hash(pressure_keys):
    """emu_aff.candidates against the slots the emulated learn pass really uses, and the clusters'
    shapes."""
    ks = pressure_keys
    assert ks.install[0] != ks.install[1] and all(ks.install)
    assert (emu_aff.candidates(ks.install[1], ac.P_NETS[1] + 77, ac.P_LOG2) == ks.cand[1][77]).all()
    wl, clf, svcs, table = _pressure(0)
    keys = ks.spread(1, 40)
    table.classify(clf, ac.key_batch(wl, svcs, keys, 3, per_key=2, established=0.0), 10)
    assert all(ks.slot_of(table, k) == [k.c[0]] for k in keys)  # nothing in the way: the first candidate
    a1, a2, b1, b2 = ks.shared
    assert len({k.c[0] for k in ks.shared}) == 1 and len({k.c[2] for k in ks.shared}) == 4
    assert [k.svc for k in ks.shared] == [0, 0, 1, 1] and [k.svc for k in ks.identical] == [0, 0, 1, 1, 1, 1]
    d, e = ks.degenerate
    assert d.c[:2] == d.c[2:] and e.c[:2] == d.c[:2] and e.c[2] != e.c[0]
    assert sum(1 for k in ks.exact_keys() if k.c[0] == d.c[0]) == 2
    f, g = ks.chain
    assert f.c[2:] == g.c[:2] and len({f.c[0], f.c[2], g.c[2]}) == 3
    assert len(ks.background) == 30 and all(len(ac.neighbours(k, ks.exact_keys())) == 1 for k in ks.background)
    assert len(ac.neighbours(a1, ks.exact_keys())) == 3 and len(ac.neighbours(ks.identical[0], ks.identical)) == 5


@pytest.mark.parametrize("order", ORDERS)
def test_colliding_keys_in_one_batch(pressure_keys, order):
    wl, clf, svcs, table = _pressure(order)
    second = ac.case_collisions(wl, clf, svcs, pressure_keys, table, _emu_runner(clf, table), order)
    assert set(second) & set(pressure_keys.shared)


@pytest.mark.parametrize("order", ORDERS)
def test_live_key_behind_an_emptied_bucket(pressure_keys, order):
    wl, clf, svcs, table = _pressure(order)
    ac.case_emptied_bucket(wl, clf, svcs, pressure_keys, table, _emu_runner(clf, table), lambda: emu.commit_host(clf), order)


@pytest.mark.parametrize("order", ORDERS)
def test_full_bucket_forced_order(pressure_keys, order):
    wl, clf, svcs, table = _pressure(order)
    ac.case_full_bucket_forced(wl, clf, svcs, pressure_keys, _emu_runner(clf, table), order)


@pytest.mark.parametrize("order", ORDERS)
def test_launch_sequence_wrap(pressure_keys, order):
    wl, clf, svcs, table = _pressure(order)
    ac.case_sequence_wrap(wl, clf, svcs, pressure_keys, table, _emu_runner(clf, table), table.set_seq, order)


def test_set_affinity_seq_needs_a_table():
    """gpc_debug_set_affinity_seq: a bad slot, the feature off, or no table yet (nothing classified on
    the slot: the table's first use restarts the sequence) is GPC_EINVAL."""
    for log2, slot in ((8, 0), (8, 1), (0, 0)):
        c = gpc.Classifier(session_affinity=log2)
        assert c.lib.gpc_debug_set_affinity_seq(c.h, slot, 0xfffffffc) == -gpc.GPC_EINVAL
    assert c.lib.gpc_debug_set_affinity_seq(None, 0, 1) == -gpc.GPC_EINVAL
