"""GPU tier: the packet-in queue built on the device (packetin.hip behind the classify launches)
against the oracle-only model (tests/packet_in_model.py) and the host emulation (tests/emu_pin.py),
byte for byte. Every device buffer -- verdicts, LB results, records, count, scratch -- is 0xA5-filled
with guard bytes behind it: nothing may be written behind min(total, cap) records, behind the count
word or behind gpc_pin_scratch_bytes(n) of scratch. The cases are tests/packet_in_cases.py."""
import copy
import ctypes as C

import numpy as np
import pytest

from antrea_amd import gpc
from tests import emu, emu_pin, emu_svc6
from tests import packet_in_cases as cases
from tests import packet_in_model as model

pytestmark = pytest.mark.gpu

FILL, GUARD = 0xA5, 64
T, N = cases.T, cases.N


@pytest.fixture(scope="module", autouse=True)
def _built():
    from antrea_amd.build import build
    build()
    import torch
    assert torch.cuda.is_available(), "GPU tier needs a HIP device"


def _to_device(cols, n):
    import torch
    dev = torch.device("cuda", 0)
    signed = {4: np.int32, 2: np.int16, 1: np.uint8}  # the same bits in torch dtypes
    out = {}
    for k, a in cols.items():
        a = np.ascontiguousarray(a[:n], dtype=gpc.PKT_COLUMNS[k])
        out[k] = torch.as_tensor(a.view(signed[a.dtype.itemsize])).to(dev)
    return out


def _buf(nbytes):
    import torch
    return torch.full((nbytes + GUARD,), FILL, dtype=torch.uint8, device=torch.device("cuda", 0))


def _host(t, nbytes, what):
    h = t.cpu().numpy()
    assert (h[nbytes:] == FILL).all(), "guard bytes behind the %s written" % what
    return h[:nbytes]


def _plain(c, cols, n, v6=False, lb=False, count=False, slot=0):
    """gpc_classify*_on without a queue: (verdicts (n, 2), LB result bytes or None)."""
    import torch
    d = _to_device(cols, n)
    lbsz = 32 if v6 else 16
    out, lbo = _buf(16 * n), _buf(lbsz * n) if lb else None
    if v6:
        c.classify6_lb_device(gpc.pkt_soa_device(d), n, out.data_ptr(), lbo.data_ptr() if lb else 0, count=count, slot=slot)
    else:
        c.classify_device(gpc.pkt_soa_device(d), n, out.data_ptr(), count=count, lb_ptr=lbo.data_ptr() if lb else 0, slot=slot)
    torch.cuda.synchronize()
    return _host(out, 16 * n, "verdicts").view(gpc.VERDICT_DTYPE).reshape(n, 2).copy(), \
        (_host(lbo, lbsz * n, "LB results").copy() if lb else None)


def _queue(c, cols, n, cap, v6=False, lb=False, count=False, slot=0, null_records=False):
    """gpc_classify*_pin_on: (verdicts (n, 2), LB result bytes or None, records, total). The records
    are the first min(total, cap); every byte behind them, of the cap entries and of the guard, must
    still hold the fill."""
    import torch
    d = _to_device(cols, n)
    lbsz = 32 if v6 else 16
    out, lbo = _buf(16 * n), _buf(lbsz * n) if lb else None
    recs, cnt = _buf(16 * cap), _buf(8)
    sb = c.pin_scratch_bytes(n)
    scratch = _buf(sb)
    q = gpc.gpc_pin_queue(records=None if null_records else recs.data_ptr(), cap=cap, count=cnt.data_ptr(),
                          scratch=scratch.data_ptr(), scratch_bytes=sb)
    call = c.classify6_pin_device if v6 else c.classify_pin_device
    call(gpc.pkt_soa_device(d), n, out.data_ptr(), q, count=count, lb_ptr=lbo.data_ptr() if lb else 0, slot=slot)
    torch.cuda.synchronize()
    total = int(_host(cnt, 8, "count").view(np.uint64)[0])
    _host(scratch, sb, "scratch")
    h = recs.cpu().numpy()
    k = min(total, cap)
    assert (h[16 * k:] == FILL).all(), "bytes behind min(total, cap) records written"
    return _host(out, 16 * n, "verdicts").view(gpc.VERDICT_DTYPE).reshape(n, 2).copy(), \
        (_host(lbo, lbsz * n, "LB results").copy() if lb else None), h[:16 * k].view(gpc.PACKET_IN_DTYPE).copy(), total


_STATE = {}


def _state(variant="plain", v6=False, **kw):
    """Built once per (variant, family, options): committed classifier, oracle, the whole batch and its
    expected verdicts."""
    key = (variant, v6, tuple(sorted(kw.items())))
    if key not in _STATE:
        c, wl = cases.make_product(variant, v6, **kw)
        c.commit()
        orc = cases.Oracle(wl, variant, v6, c)
        cols4 = cases.make_batch()
        cols = cases.to_v6(cols4) if v6 else cols4
        okey = (variant, v6, "expect")
        if okey not in _STATE:  # (the oracle's walk does not depend on the launch options)
            _STATE[okey] = orc.expect(cols)[0]
        _STATE[key] = {"c": c, "wl": wl, "orc": orc, "cols": cols, "v": _STATE[okey], "v6": v6, "variant": variant}
    return _STATE[key]


def _slice(s, n):
    """(columns, expected verdicts, expected records) of the size case n."""
    lo = 64 if n <= 65 else 0
    cols = {k: np.ascontiguousarray(a[lo:lo + n]) for k, a in s["cols"].items()}
    v = s["v"][lo:lo + n]
    return cols, v, model.records(v, s["orc"].ops)


def _emulated(s, cols):
    v = (emu_svc6.classify6 if s["v6"] else emu.classify)(s["c"], cols)
    return v, emu_pin.collect(s["c"], v)


def _check(s, n, cap=None, **kw):
    cols, v, want = _slice(s, n)
    cap = 2 * n if cap is None else cap
    got_v, _, got, total = _queue(s["c"], cols, n, cap, v6=s["v6"], **kw)
    ev, (erecs, etotal) = _emulated(s, cols)
    assert got_v.tobytes() == ev.tobytes() == np.ascontiguousarray(v).tobytes()
    assert total == etotal == len(want), (total, etotal, len(want))
    k = min(total, cap)
    assert got.tobytes() == erecs[:k].tobytes() == want[:k].tobytes()
    assert (got["reserved"] == 0).all()
    return got, total


@pytest.mark.parametrize("n", cases.SIZES)
def test_batch_sizes(n):
    """One packet, a partial wave, a full wave, one lane past it; one packet short of a tile, a tile,
    one past it; three tiles and five packets."""
    s = _state()
    got, total = _check(s, n)
    assert total > 0
    if n == N:
        cases.check_conditions("plain", s["v"], got)


@pytest.mark.parametrize("cap", ["null", "total", "total-1", "one"])
def test_caps(cap):
    s = _state()
    total = len(_slice(s, N)[2])
    assert total > 2
    if cap == "null":
        got, t = _check(s, N, cap=0, null_records=True)
        assert len(got) == 0 and t == total
    else:
        k = {"total": total, "total-1": total - 1, "one": 1}[cap]
        got, t = _check(s, N, cap=k)
        assert len(got) == k and t == total


@pytest.mark.parametrize("variant", ["deny_tracking", "quiet"])
def test_variants(variant):
    s = _state(variant)
    got, total = _check(s, N)
    cases.check_conditions(variant, s["v"], got)
    if variant == "quiet":
        assert total == 0 and s["c"].debug_pin_image() == (None, 0)


@pytest.mark.parametrize("n", [65, T + 1, N])
def test_grouped_path(n):
    """group_packets = 1: the batch is classified in grouped order and un-permuted; the collection
    runs behind that, over verdicts in caller order."""
    s = _state(group_packets=1)
    _check(s, n)
    before = s["c"].launch_times()
    s["c"].set_launch_timing(4)
    try:
        _check(s, n)
        kinds = s["c"].launch_times()
    finally:
        s["c"].set_launch_timing(0)
    assert "group_tiles" in kinds and "pin_scatter" in kinds, (before, kinds)


def _late_rule(fid, net, logging=True):
    return {"direction": "Out", "table": "AntreaPolicyEgressRule", "action": "Drop", "flow_id": fid,
            "policy_type": "AntreaClusterNetworkPolicy", "policy_namespace": "", "policy_name": "pin-late",
            "policy_uid": "uid-pin-late", "name": "rule-%d" % fid, "tier_priority": 50, "priority": 63000 + fid % 100,
            "service": None, "enable_logging": logging, "from": ["10.0.0.1"], "to": [{"ipnet": "%d.0.0.0/16" % net}]}


def test_delta_epoch_compact_replay():
    """A logged rule added by a delta commit (journal mode) is collected; the queue is the same after
    gpc_compact and after gpc_replay; uninstalling the rule empties its records again."""
    c, wl = cases.make_product("plain", compact_after=-1)
    c.commit()
    orc = cases.Oracle(wl, "plain")
    cols = cases.make_batch(T + 70)
    hit = np.arange(3, T + 70, 7)
    cols["src"][hit] = cases.POD(0)
    cols["dst"][hit] = (70 << 24) | (hit & 0xFFFF)
    s = {"c": c, "orc": orc, "cols": cols, "v6": False}
    n = len(cols["src"])

    def run(tag):
        s["v"] = model.verdicts(orc.pipe, cols)
        got, total = _check(s, n)
        return got

    base = run("base")
    assert not (base["conj_id"] == 160).any()
    late = _late_rule(160, 70)
    c.install_policy_rule_flows(copy.deepcopy(late))
    orc.install(late)
    c.commit()
    orc.refresh()
    st = c.image_stats()
    assert st["n_overlay_rules"] > 0 and st["n_delta_builds"] >= 1
    delta = run("delta")
    mine = delta[delta["conj_id"] == 160]
    assert len(mine) == len(hit) and (mine["operations"] == 1).all() and (mine["disposition"] == 1).all()
    c.compact()
    assert c.image_stats()["n_overlay_rules"] == 0
    assert run("compact").tobytes() == delta.tobytes()
    c.replay()
    assert run("replay").tobytes() == delta.tobytes()
    for side in (c, orc.fnp):
        side.uninstall_policy_rule_flows(160)
    c.commit()
    orc.refresh()
    assert run("uninstalled").tobytes() == base.tobytes()


@pytest.mark.parametrize("n", [65, N])
def test_ipv6(n):
    """gpc_classify6_pin_on over the IPv6 embedding, the IPv6 Service without Endpoints included."""
    s = _state("plain", True)
    got, total = _check(s, n, lb=True)
    if n == N:
        assert (got["category"] == gpc.PIN_CAT_SVC_REJECT).any() and (got["category"] == gpc.PIN_CAT_DNS).any()
        v4 = _state()
        assert got.tobytes() == _slice(v4, N)[2].tobytes(), "the embedding keeps the queue"
    else:  # the host wrapper
        cols, v, want = _slice(s, n)
        hv, hlb, hrecs, total = s["c"].classify6_host_pin(cols, cap=2 * n, lb=True)
        assert total == len(want) and hrecs.tobytes() == want.tobytes() and hv.tobytes() == np.ascontiguousarray(v).tobytes()


def test_second_slot():
    """Slot 1 of a two-slot context on one device: its own copy of the packet-in image."""
    c, wl = cases.make_product("plain", devices=[0, 0])
    c.commit()
    s = dict(_state(), c=c)
    a, ta = _check(s, T + 1, slot=1)
    b, tb = _check(s, T + 1, slot=0)
    assert ta == tb and a.tobytes() == b.tobytes()


def test_other_outputs_unchanged_and_launch_kinds():
    """Verdicts, LB results and per-rule counters of a call with a queue equal those of gpc_classify_on on
    the same batch; the pin_* launch kinds appear for calls with a queue only."""
    s = _state()
    c, cols = s["c"], s["cols"]
    c.set_launch_timing(8)
    try:
        c.launch_times()
        c.reset_counters()
        v0, lb0 = _plain(c, cols, N, lb=True, count=True)
        m0 = {k: tuple(v) for k, v in c.network_policy_metrics().items() if any(v)}
        k0 = c.launch_times()
        c.reset_counters()
        v1, lb1, recs, total = _queue(c, cols, N, 2 * N, lb=True, count=True)
        m1 = {k: tuple(v) for k, v in c.network_policy_metrics().items() if any(v)}
        k1 = c.launch_times()
    finally:
        c.set_launch_timing(0)
    assert v0.tobytes() == v1.tobytes() and lb0.tobytes() == lb1.tobytes()
    assert m0 == m1 and len(m0) > 5
    pin = {"pin_count", "pin_scan", "pin_scatter"}
    assert not pin & set(k0) and pin <= set(k1), (k0, k1)
    assert set(k1) - pin == set(k0) and all(k1[k]["launches"] == 1 for k in pin)
    assert all(k1[k]["launches"] == k0[k]["launches"] for k in k0)


def test_arguments():
    import torch
    s = _state()
    c = s["c"]
    n = 130
    cols, v, want = _slice(s, n)
    d = _to_device(cols, n)
    soa = gpc.pkt_soa_device(d)
    out, recs, cnt = _buf(16 * n), _buf(16 * 8), _buf(8)
    sb = c.pin_scratch_bytes(n)
    scratch = _buf(sb + 16)
    good = dict(records=recs.data_ptr(), cap=8, count=cnt.data_ptr(), scratch=scratch.data_ptr(), scratch_bytes=sb)
    bad = [dict(good, scratch_bytes=sb - 1), dict(good, scratch=None), dict(good, scratch=scratch.data_ptr() + 8),
           dict(good, records=recs.data_ptr() + 4), dict(good, records=None), dict(good, count=None),
           dict(good, count=cnt.data_ptr() + 4)]
    for kw in bad:
        rc = c.lib.gpc_classify_pin_on(c.h, 0, C.byref(soa), n, out.data_ptr(), None, C.byref(gpc.gpc_pin_queue(**kw)), 0, None)
        assert rc == -gpc.GPC_EINVAL, kw
    assert c.lib.gpc_classify_pin_on(c.h, 0, C.byref(soa), n, out.data_ptr(), None, None, 0, None) == -gpc.GPC_EINVAL
    torch.cuda.synchronize()
    for t, nb in ((out, 16 * n), (recs, 16 * 8), (cnt, 8), (scratch, sb + 16)):
        assert (t.cpu().numpy() == FILL).all(), "a rejected call wrote something"
    # n == 0: the count alone, no scratch needed
    q = gpc.gpc_pin_queue(records=None, cap=0, count=cnt.data_ptr(), scratch=None, scratch_bytes=0)
    c.classify_pin_device(soa, 0, out.data_ptr(), q)
    torch.cuda.synchronize()
    assert int(_host(cnt, 8, "count").view(np.uint64)[0]) == 0
    assert (out.cpu().numpy() == FILL).all()
    # the host wrapper, short and full
    hv, hrecs, total = c.classify_host_pin(cols, cap=3)
    assert total == len(want) > 3 and hrecs.tobytes() == want[:3].tobytes()
    hv, hrecs, total = c.classify_host_pin(cols, cap=2 * n)
    assert hrecs.tobytes() == want.tobytes() and hv.tobytes() == np.ascontiguousarray(v).tobytes()
