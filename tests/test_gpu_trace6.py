"""GPU tier: gpc_trace6 on the device (classify.hip trace6_kernel: the IPv6 Service stage, the LPM
coding of the address columns and the traced walk in one launch) and gpc_trace_on.

Per packet of the native batch of tests/v6_cases.py the device trace is compared with the oracle's own
walk of the same flows (tests/trace6_util.py), its verdict pair with the data path's
(gpc_classify6_host_lb), every address record's code with the host run of the device's LPM
instantiation (emu.v6_codes "one") and its translated prefix with the longest prefix of the flow text
that holds the address; GPC_T6_OVERFLOW marks exactly the addresses in a prefix a delta commit
interned. Behind IPv6 Services the LB result and the DNAT show in the records; with session affinity
the trace reads the slot's table and leaves it, and its counters, as they were."""
import copy
import ctypes as C
import ipaddress

import numpy as np
import pytest

from antrea_amd import gpc, workload
from tests import affinity6_cases as a6
from tests import emu, trace6_util as tu, v6_cases as vc

pytestmark = pytest.mark.gpu

N = 200
A, L = gpc.LB_AFFINITY, gpc.LB_LEARNED
P, O, D = gpc.T6_PRESENT, gpc.T6_OVERFLOW, gpc.T6_DNAT


@pytest.fixture(scope="module", autouse=True)
def _built():
    from antrea_amd.build import build
    build()
    import torch
    assert torch.cuda.is_available(), "GPU tier needs a HIP device"


_STATE = {}


def _path(path):
    """Per path, built once: workload, classifier, the first N packets of the native batch (with and
    without the ct address columns), the oracle; the oracle's traces are computed once per column set."""
    if path not in _STATE:
        w6 = vc.workload_of(path, tu.SEED)
        c = vc.make_classifier(path, w6, lambda k: k.commit())
        cols, opt, info = vc.native_packets(w6, tu.SEED)
        cols = vc.head(cols, N)
        ct = dict(cols, ct_src6=np.ascontiguousarray(opt["ct_src6"][:N]), ct_dst6=np.ascontiguousarray(opt["ct_dst6"][:N]))
        _STATE[path] = {"w6": w6, "c": c, "plain": cols, "ct": ct, "oracle": tu.Oracle(path, w6)}
    return _STATE[path]


def _want(s, key):
    if "want_" + key not in s:
        s["want_" + key] = tu.oracle_traces(s["oracle"], s["c"], s[key], N)
    return s["want_" + key]


def _pkt(cols, i):
    return {k: v[i] for k, v in cols.items()}


def _check_records(s, path, cols, rw, i, addrs, codes, seen):
    """The four address records of packet i: rw = the columns as the policy stages see them, codes =
    {column: emu.v6_codes "one" of that column}."""
    for k, name in enumerate(tu.ADDR_COLUMNS):
        r = addrs[k]
        if name not in rw:
            assert r == {"prefix": None, "code": 0, "flags": 0}, (path, i, name, r)
            continue
        a = tu.addr_int(rw[name][i])
        assert r["flags"] & P and r["code"] == int(codes[name][i]), (path, i, name, r, int(codes[name][i]))
        tu.check_prefix(r["prefix"], a, s["oracle"], path != "delta", (path, i, name))
        # interned by a delta commit: a prefix of the final flow text that the base epoch's lacks
        late = r["prefix"] is not None and r["prefix"] not in s["oracle"].base_nets
        assert bool(r["flags"] & O) == late, (path, i, name, r)
        if late:
            seen.add(r["prefix"].prefixlen)


@pytest.mark.parametrize("columns", ["plain", "ct"])
@pytest.mark.parametrize("path", ["base", "delta", "grouped"])
def test_device_trace6_vs_oracle_and_flow_text_lpm(path, columns):
    s = _path(path)
    c, cols, want = s["c"], s[columns], _want(s, columns)
    data = c.classify6_host(cols)
    codes = {k: emu.v6_codes(c, cols[k])[0] for k in tu.ADDR_COLUMNS if k in cols}
    late = set()
    for i in range(N):
        verdicts, steps, lb, addrs = c.trace6(_pkt(cols, i))
        tu.same_trace(verdicts, steps, want[i], (path, columns, i))
        assert (verdicts == data[i]).all(), (path, i, verdicts, data[i])
        assert lb.tobytes() == bytes(32)
        _check_records(s, path, cols, cols, i, addrs, codes, late)
    # the lengths whose OVERFLOW bit was seen are those the flow text alone expects: the prefixes of
    # the final text that the base epoch's lacks and that hold one of the traced addresses -- none on a
    # full build; on the delta path one of every length the delta commits brought once the ct columns
    # are traced too (of these 200 packets, src6 / dst6 alone reach the new /24 and /64)
    expect = set()
    for k in codes:
        nets = (s["oracle"].lpm(tu.addr_int(a)) for a in cols[k])
        expect |= {p.prefixlen for p in nets if p is not None and p not in s["oracle"].base_nets}
    assert late == expect, (late, expect)
    if path != "delta":
        assert not expect
    elif columns == "ct":
        assert set(vc.NEW_LENGTHS) | {64} <= expect, expect
    else:
        assert {24, 64} <= expect, expect


def test_device_trace6_behind_ipv6_services():
    s = _path("svc6")
    c, cols, want = s["c"], s["plain"], _want(s, "plain")
    rw, want_lb, noep = tu.policy_columns(c, cols)  # host run of the Service stage: which packet is of which kind
    dnat = (want_lb["flags"] & gpc.LB_DNAT) != 0
    assert dnat.any() and noep.any() and (want_lb["flags"] == 0).any()
    data, data_lb = c.classify6_host(cols, lb=True)
    codes = {k: emu.v6_codes(c, rw[k])[0] for k in tu.ADDR_COLUMNS if k in rw}
    for i in range(N):
        verdicts, steps, lb, addrs = c.trace6(_pkt(cols, i))
        assert lb.tobytes() == data_lb[i].tobytes() and (verdicts == data[i]).all(), (i, lb, data_lb[i], verdicts, data[i])
        tu.same_trace(verdicts, steps, want[i], ("svc6", i))
        if noep[i]:
            assert verdicts[0]["action"] == gpc.ACT_NAMES.index("REJECT") and verdicts[0]["table"] == gpc.VTABLE_ENDPOINT_DNAT
            assert steps == [] and all(r == {"prefix": None, "code": 0, "flags": 0} for r in addrs), (i, addrs)
            continue
        _check_records(s, "svc6", cols, rw, i, addrs, codes, set())
        assert bool(addrs[1]["flags"] & D) == bool(dnat[i]) and not any(addrs[k]["flags"] & D for k in (0, 2, 3))
        if dnat[i]:  # addrs[1]: the Endpoint; addrs[3]: the Service IP
            assert (rw["dst6"][i] == lb["endpoint_ip"]).all() and (rw["ct_dst6"][i] == cols["dst6"][i]).all()
            assert (rw["dst6"][i] != cols["dst6"][i]).any()


def test_trace6_reads_the_affinity_table_and_never_learns():
    wl, rules, c, svcs = a6.make_pressure_product()
    c.commit()
    cfg, eps = svcs[0]
    client, other_client = a6.b16(a6.P_NETS[0] + 5), a6.b16(a6.P_NETS[0] + 6)
    pkt = {"src6": client, "dst6": a6.b16(a6.ip6(cfg["ip"])), "sport": 40000, "dport": 80, "proto": 6, "out_port": 0}
    ep = lambda lb: (bytes(lb["endpoint_ip"]), int(lb["endpoint_port"]))
    ports = (40000, 40001, 40002, 40003, 40004, 40005)
    c.set_affinity_clock(20)

    def hash_choices():
        own, own6 = {}, {}
        for sp in ports:
            v, steps, lb, addrs = c.trace6(dict(pkt, sport=sp))
            own[sp] = ep(lb)
            assert not (lb["flags"] & (A | L)) and lb["flags"] & gpc.LB_HIT and addrs[1]["flags"] & D
            v, steps, lb, addrs = c.trace6(dict(pkt, src6=other_client, sport=sp))
            own6[sp] = ep(lb)
        return own, own6

    own, own6 = hash_choices()  # before the slot has a table
    assert c.affinity_stats6()["learned"] == 0 and len(set(own.values())) > 1
    miss = {k: np.array([v], gpc.PKT_COLUMNS[k]) for k, v in dict(pkt, dst6=a6.b16(a6.ip6("2001:db8:ffff::9"))).items()}
    _, lbm = c.classify6_host(miss, lb=True)  # a batch that hits no Service: the table exists, empty
    assert lbm["flags"][0] == 0
    before = c.affinity_stats6()
    assert hash_choices() == (own, own6)  # read-only over the empty table: the same choices, nothing created
    assert c.affinity_stats6() == before and before["learned"] == 0 and len(c.affinity_table6()) == 0
    cols = {k: np.array([v], gpc.PKT_COLUMNS[k]) for k, v in pkt.items()}
    got, lbb = c.classify6_host(cols, lb=True)
    assert lbb["flags"][0] & L and ep(lbb[0]) == own[40000]
    other = next(sp for sp in ports if own[sp] != own[40000])
    stats, table = c.affinity_stats6(), c.affinity_table6()
    v, steps, lb, addrs = c.trace6(dict(pkt, sport=other))  # a live entry: the learned Endpoint, whatever the hash says
    assert ep(lb) == own[40000] and (lb["flags"] & (A | L)) == A and len(steps) >= 1
    v, steps, lb, addrs = c.trace6(dict(pkt, src6=other_client, sport=other))  # another client: no entry, nothing created
    assert ep(lb) == own6[other] and not (lb["flags"] & (A | L))
    assert c.affinity_stats6() == stats and c.affinity_table6().tobytes() == table.tobytes()
    assert stats["learned"] == 1 and stats["live"] == 1 and stats["hits"] == 0 and len(table) == 1
    v2, lb2 = c.classify6_host({k: np.array([x], gpc.PKT_COLUMNS[k]) for k, x in dict(pkt, sport=other).items()}, lb=True)
    v, steps, lb, addrs = c.trace6(dict(pkt, sport=other))
    assert (v == v2[0]).all() and ep(lb) == ep(lb2[0]) == own[40000]  # the data path agrees (and counts its hit)
    assert c.affinity_stats6()["hits"] == 1
    c.set_affinity_clock(20 + a6.P_TIMEOUTS[0])  # expired
    v, steps, lb, addrs = c.trace6(dict(pkt, sport=other))
    assert ep(lb) == own[other] and not (lb["flags"] & (A | L))


def _simple4(**kw):
    """C1's rules + one IPv4 affinity ClusterIP Service of 8 remote Endpoints."""
    wl = workload.config1(seed=81)
    c = gpc.Classifier(session_affinity=a6.LOG2, **kw)
    c.initialize()
    c.batch_install_policy_rule_flows(copy.deepcopy(wl.rules))
    eps = [{"ip": "10.128.1.%d" % (k + 1), "port": 8000 + k, "is_local": False, "node_name": "n%d" % k} for k in range(8)]
    cfg = {"ip": "10.96.0.100", "port": 80, "protocol": "TCP", "cluster_group_id": 100, "local_group_id": 101,
           "affinity_timeout": 100}
    c.install_service_group(cfg["cluster_group_id"], eps, True)
    c.install_endpoint_flows("TCP", eps)
    c.install_service_flows(cfg)
    return c, cfg


def test_trace_on_shows_the_slots_own_affinity_table():
    c, cfg = _simple4(devices=[0, 0])
    c.commit()
    c.set_affinity_clock(20)
    pkt = {"src": 0x0a0a0005, "dst": int(ipaddress.ip_address(cfg["ip"])), "sport": 40000, "dport": 80, "proto": 6, "out_port": 0}
    ep = lambda lb: (int(lb["endpoint_ip"]), int(lb["endpoint_port"]))
    own = {sp: ep(c.trace(dict(pkt, sport=sp))[2]) for sp in range(40000, 40006)}
    other = next(sp for sp in own if own[sp] != own[40000])
    cols = {k: np.array([v], gpc.PKT_COLUMNS[k]) for k, v in pkt.items()}
    _, lbb = c.classify_host(cols, lb=True, slot=1)  # slot 1 learns the client's Endpoint
    assert lbb["flags"][0] & L and ep(lbb[0]) == own[40000]
    v1, steps1, lb1 = c.trace(dict(pkt, sport=other), slot=1)
    assert ep(lb1) == own[40000] and (lb1["flags"] & (A | L)) == A
    v0, steps0, lb0 = c.trace(dict(pkt, sport=other), slot=0)
    assert ep(lb0) == own[other] and not (lb0["flags"] & (A | L))
    assert c.affinity_stats(0)["learned"] == 0 and c.affinity_stats(1)["learned"] == 1
    # gpc_trace == gpc_trace_on(..., 0)
    soa, keep, _ = gpc.pkt_soa_host({k: np.array([v], gpc.PKT_COLUMNS[k]) for k, v in dict(pkt, sport=other).items()})
    out, lb = np.zeros(2, gpc.VERDICT_DTYPE), np.zeros(1, gpc.LB_DTYPE)
    steps, ns = (gpc.gpc_trace_step * 8)(), C.c_size_t()
    assert c.lib.gpc_trace(c.h, C.byref(soa), out.ctypes.data, lb.ctypes.data, steps, 8, C.byref(ns)) == 0
    assert (out == v0).all() and lb[0] == lb0 and ns.value == len(steps0)
    assert [steps[i].table for i in range(ns.value)] == [st["table"] for st in steps0]
    with pytest.raises(gpc.GpcError) as e:
        c.trace(pkt, slot=2)
    assert e.value.code == gpc.GPC_EINVAL


def _einval(fn):
    with pytest.raises(gpc.GpcError) as e:
        fn()
    assert e.value.code == gpc.GPC_EINVAL


def test_trace6_errors_and_step_capacity():
    s = _path("base")
    c, cols = s["c"], s["plain"]
    pkt = _pkt(cols, 0)
    v4 = gpc.Classifier()  # a context without IPv6
    v4.initialize()
    v4.batch_install_policy_rule_flows(copy.deepcopy(workload.config1(seed=7).rules))
    v4.commit()
    _einval(lambda: v4.trace6(pkt))
    fresh = gpc.Classifier(ipv4=False, ipv6=True)  # before the first commit
    fresh.initialize()
    _einval(lambda: fresh.trace6(pkt))
    _einval(lambda: c.trace6(pkt, slot=2))
    _einval(lambda: c.trace6({k: v for k, v in pkt.items() if k != "dst6"}))
    # a six-step walk into one step of room: -GPC_ERANGE, the step count and the first step reported
    want = _want(s, "plain")
    i = next(i for i in range(N) if len(want[i][1]) == 6)
    soa, keep, _ = gpc.pkt_soa_host({k: np.array([v], gpc.PKT_COLUMNS[k]) for k, v in _pkt(cols, i).items()})
    out, steps, ns = np.zeros(2, gpc.VERDICT_DTYPE), (gpc.gpc_trace_step * 1)(), C.c_size_t()
    rc = c.lib.gpc_trace6(c.h, 0, C.byref(soa), out.ctypes.data, None, None, steps, 1, C.byref(ns))
    assert rc == -gpc.GPC_ERANGE and ns.value == 6 and steps[0].table == want[i][1][0][0]
    assert (out == c.classify6_host({k: v[i:i + 1] for k, v in cols.items()})[0]).all()
