"""Packet-in queue, host tier: core.hpp pin_records (tests/csrc/emu_pin.cpp) over the emulated verdicts
and the packet-in image the library built, against the oracle-only model (tests/packet_in_model.py);
and the packet-in image as the control plane moves."""
import copy
import ctypes as C

import numpy as np
import pytest

from antrea_amd import gpc
from tests import emu, emu_pin, emu_svc6
from tests import packet_in_cases as cases
from tests.test_emu_parity import _cmp

_cache = {}


def _case(variant, v6=False):
    """(classifier committed on the host, oracle, IPv4 columns, columns as classified, expected verdicts, records)."""
    key = (variant, v6)
    if key not in _cache:
        c, wl = cases.make_product(variant, v6)
        emu.commit_host(c)
        orc = cases.Oracle(wl, variant, v6, c)
        cols4 = cases.make_batch()
        cols = cases.to_v6(cols4) if v6 else cols4
        v, recs = orc.expect(cols)
        _cache[key] = (c, orc, cols4, cols, v, recs)
    return _cache[key]


def _same(got, want):
    assert got.dtype == want.dtype == gpc.PACKET_IN_DTYPE
    assert len(got) == len(want), (len(got), len(want))
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (bad[:5], got[bad[:3]], want[bad[:3]])


def test_abi_shapes():
    assert gpc.PACKET_IN_DTYPE.itemsize == 16 and C.sizeof(gpc.gpc_pin_queue) == 40
    assert emu_pin.load().emu_pin_tile() == gpc.PIN_TILE
    assert gpc.load().gpc_abi_version() == 6
    b = C.c_size_t()
    lib = gpc.load()
    for n in (0, 1, 64, 65, gpc.PIN_TILE, gpc.PIN_TILE + 1, 1 << 24):
        assert lib.gpc_pin_scratch_bytes(n, C.byref(b)) == 0
        waves, tiles = (n + 63) // 64, (n + gpc.PIN_TILE - 1) // gpc.PIN_TILE
        assert b.value >= 16 * waves + 8 * tiles and b.value % 16 == 0 and b.value <= 16 * waves + 8 * tiles + 8
    assert lib.gpc_pin_scratch_bytes((1 << 32) - 255, C.byref(b)) == -gpc.GPC_EINVAL


@pytest.mark.parametrize("variant", cases.VARIANTS)
def test_case_conditions(variant):
    c, orc, cols4, cols, v, recs = _case(variant)
    cases.check_conditions(variant, v, recs)


@pytest.mark.parametrize("variant", cases.VARIANTS)
def test_records_emu_vs_model(variant):
    c, orc, cols4, cols, v, recs = _case(variant)
    got_v = emu.classify(c, cols)
    _cmp(got_v, v, cols)
    assert emu_pin.image_map(c) == orc.ops
    if variant == "quiet":
        assert c.debug_pin_image() == (None, 0)
    got, total = emu_pin.collect(c, got_v)
    assert total == len(recs)
    _same(got, recs)
    for cap in (0, 1, total - 1):  # a short queue keeps the leading records and still counts them all
        if cap < 0:
            continue
        part, t = emu_pin.collect(c, got_v, cap)
        assert t == total
        _same(part, recs[:cap])


def test_records_emu_vs_model_v6():
    """The same rules, Services and packets embedded in IPv6 (the IPv6 Service without Endpoints included)."""
    c, orc, cols4, cols, v, recs = _case("plain", True)
    v4, recs4 = _case("plain")[4:6]
    assert (v == v4).all() and (recs == recs4).all(), "the embedding keeps verdicts and records"
    cases.check_conditions("plain", v, recs)
    got_v = emu_svc6.classify6(c, cols)
    _cmp(got_v, v, cols)
    assert emu_pin.image_map(c) == orc.ops
    got, total = emu_pin.collect(c, got_v)
    assert total == len(recs)
    _same(got, recs)


def _logged(fid, net):
    return {"direction": "Out", "table": "AntreaPolicyEgressRule", "action": "Drop", "flow_id": fid,
            "policy_type": "AntreaClusterNetworkPolicy", "policy_namespace": "", "policy_name": "pin-late",
            "policy_uid": "uid-pin-late", "name": "rule-%d" % fid, "tier_priority": 50, "priority": 63000 + fid % 100,
            "service": None, "enable_logging": True, "from": ["10.0.0.1"], "to": [{"ipnet": "%d.0.0.0/16" % net}]}


def test_image_follows_the_control_plane():
    c, wl = cases.make_product("plain")
    orc = cases.Oracle(wl, "plain")
    assert c.debug_pin_image() == (None, 0)  # nothing committed yet
    emu.commit_host(c)
    assert emu_pin.image_map(c) == orc.ops and len(orc.ops) >= 9
    full = c.image_stats()["n_full_builds"]
    # a delta commit that adds a logged rule
    late = _logged(150, 70)
    for side in (c, orc.fnp):
        side.install_policy_rule_flows(copy.deepcopy(late))
    emu.commit_host(c)
    assert c.image_stats()["n_full_builds"] == full and c.image_stats()["n_delta_builds"] >= 1
    want = cases.model.ops_map(orc.fnp)
    assert want[150] == 1 and emu_pin.image_map(c) == want
    # a commit that touches no packet-in flow: the blob is not rebuilt
    ptr, words = emu_pin.image_bytes(c)
    plain = dict(_logged(151, 71), enable_logging=False)
    for side in (c, orc.fnp):
        side.install_policy_rule_flows(copy.deepcopy(plain))
    c.add_policy_rule_address(151, "dst", [{"ipnet": "72.0.0.0/16"}], plain["priority"])
    emu.commit_host(c)
    ptr2, words2 = emu_pin.image_bytes(c)
    assert ptr2 == ptr and (words2 == words).all()
    emu.commit_host(c)  # nothing pending at all
    assert emu_pin.image_bytes(c)[0] == ptr
    # uninstall: the id is gone
    for side in (c, orc.fnp):
        side.uninstall_policy_rule_flows(150)
    emu.commit_host(c)
    want = cases.model.ops_map(orc.fnp)
    assert 150 not in want and emu_pin.image_map(c) == want
    # reinstall with logging flipped, both ways
    for fid, logging in ((151, True), (cases.FID["e_drop_log"], False)):
        r = next(x for x in wl.rules + [plain] if x["flow_id"] == fid)
        for side in (c, orc.fnp):
            side.uninstall_policy_rule_flows(fid)
            side.install_policy_rule_flows(dict(copy.deepcopy(r), enable_logging=logging))
    emu.commit_host(c)
    want = cases.model.ops_map(orc.fnp)
    assert want.get(151) == 1 and cases.FID["e_drop_log"] not in want and emu_pin.image_map(c) == want
    # compaction keeps it
    before = emu_pin.image_bytes(c)
    emu.commit_host(c, full=True)
    after = emu_pin.image_bytes(c)
    assert after[0] == before[0] and (after[1] == before[1]).all() and emu_pin.image_map(c) == want


def test_image_goes_away_with_its_last_flow():
    c = gpc.Classifier()
    c.initialize()
    c.install_policy_rule_flows(_logged(150, 70))
    emu.commit_host(c)
    assert emu_pin.image_map(c) == {150: 1}
    c.uninstall_policy_rule_flows(150)
    emu.commit_host(c)
    assert c.debug_pin_image() == (None, 0)


def test_load_flows_rebuilds_the_same_image():
    c, wl = cases.make_product("deny_tracking")
    emu.commit_host(c)
    want = emu_pin.image_map(c)
    assert want and any(o == 2 for o in want.values())
    blob = emu_pin.image_bytes(c)[1]
    c2 = gpc.Classifier(enable_deny_tracking=True)
    c2.load_flows(c.dump_flows())
    emu.commit_host(c2)
    assert emu_pin.image_map(c2) == want
    assert (emu_pin.image_bytes(c2)[1] == blob).all()
    cols = cases.make_batch(512)
    v = emu.classify(c2, {k: a for k, a in cols.items()})
    got, total = emu_pin.collect(c2, v)
    ref, _ = emu_pin.collect(c, emu.classify(c, cols))
    ref = ref[ref["category"] != gpc.PIN_CAT_SVC_REJECT]  # (flow text carries no groups: c2 has no Services)
    assert total == len(ref) > 0
    _same(got, ref)


def test_many_ids_hash():
    """A few thousand ids through the image builder: every id found with its value, no other id found."""
    c = gpc.Classifier()
    c.initialize()
    rules = [dict(_logged(1000 + i, 70), priority=20000 + i, enable_logging=bool(i % 3), action="Drop" if i % 2 else "Reject",
                  to=[{"ipnet": "%d.%d.0.0/16" % (70 + i // 250, i % 250)}]) for i in range(3000)]
    c.batch_install_policy_rule_flows(rules)
    emu.commit_host(c)
    want = {r["flow_id"]: (1 if r["enable_logging"] else 0) + (4 if r["action"] == "Reject" else 0) for r in rules}
    want = {k: o for k, o in want.items() if o}
    assert emu_pin.image_map(c) == want
    img, _ = c.debug_pin_image()
    lib = emu_pin.load()
    assert all(lib.emu_pin_lookup(img, k) == 0 for k in list(range(1, 1000)) + [r["flow_id"] for r in rules if r["flow_id"] not in want])
