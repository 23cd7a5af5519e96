"""CPU tier: the host-set combination index (image.cpp build_composite, core.hpp kBandCombo) and the
other layouts build_composite can choose, at the small scale of tests/combo_cases.py.

The host emulation of the kernel body over the image the product built is compared with the C
restatement of the OVS classifier over the oracle compiler's flows: every packet's verdict pair and
the per-rule {packets, bytes, sessions}. What was built is read back through emu.composite_layout /
emu.combo_ids, so every test also states that the format under test is present.

Verified to fail: with the `hi`-byte half of entry_pass's `cok` dropped, and with the `key == 0u`
skip of the combination sub-index dropped, test_base[dense] fails (each tried on a scratch copy)."""
import copy
import os

import numpy as np
import pytest

from antrea_amd import gpc, workload
from oracle import ovs_cls
from tests import combo_cases as cc
from tests import emu

COMBO = emu.BAND_COMBO


def _image(clf):
    """The committed host image: its header (the sub-indexes' formats live there) and its words."""
    snap = emu.snapshot(clf)
    return snap["hdr"].tobytes() + snap["blob"].tobytes()


def _dir_block_loads(clf, cols):
    """64-B lines of bucket directories (core.hpp dir_list) the emulation reads for cols, summed over
    the packets: the emulation's line statistics are kept per source line of the read."""
    with open(os.path.join(emu.ROOT, "antrea_amd", "csrc", "core.hpp")) as f:
        line = 1 + next(i for i, text in enumerate(f) if "GPC_TOUCH(d, 16);" in text)
    emu.site_lines(reset=True)
    emu.classify(clf, cols)
    return emu.site_lines(reset=True).get(line & 2047, 0)


def _check_conditions(name, cond):
    """The conditions on the cases (tests/combo_cases.py conditions): on the oracle's verdicts alone."""
    assert {cc.NO_MATCH, cc.ALLOW, cc.DROP} <= cond["actions"], cond
    for d in ("In", "Out"):
        k = cond[d]
        assert k["decided"] >= 200, (d, k["decided"])
        assert k["shapes"] == set(cc.SHAPES), (d, k["shapes"])
        assert k["id0_in_pool"] > 0, d  # pool addresses in no group: the sub-index is skipped
        if name == "dense":
            assert k["max_id"] >= 256, (d, k["max_id"])  # an id that needs the `hi` byte decides a packet
        else:
            assert set(range(8)) <= k["ids"], (d, k["ids"])


@pytest.mark.parametrize("name", ["tiny", "dense"])
def test_base(name, monkeypatch):
    """Verdicts and counters of the combination image equal the oracle's and those of a twin built
    under GPC_NO_COMBO=1; the images differ and only the first has the combination band, on the
    source axis of the ingress table and the destination axis of the egress table. `dense` reaches
    the format at the production threshold, `tiny` with the threshold forced to 1."""
    ref = cc.reference(name)
    c, cols = ref["case"], ref["cols"]
    assert (c.env == {}) == (name == "dense")
    monkeypatch.delenv("GPC_COMBO_MIN_ENTRIES", raising=False)
    clf = cc.classifier(c, monkeypatch)
    twin = cc.classifier(c, monkeypatch, env={"GPC_NO_COMBO": "1"})
    for d in ("In", "Out"):
        assert COMBO in cc.bands(clf, d) and 4 not in cc.bands(clf, d), cc.bands(clf, d)
        assert COMBO not in cc.bands(twin, d) and 4 in cc.bands(twin, d), cc.bands(twin, d)
        assert {2, 3} <= set(cc.bands(clf, d))  # the /24 and the /28 keep their own bands
    assert _image(clf) != _image(twin)
    _check_conditions(name, cc.conditions(c, clf, cols, ref["want"]))
    got, counted = cc.emulate(clf, cols)
    cc.same(got, ref["want"], cols, "combination image against the oracle")
    assert counted == ref["metrics"]
    # combination 0 is skipped, not probed. Ingress packets whose source lies in the pool but in no
    # group: no entry is scanned, and the only bucket-directory blocks read are those of the ingress
    # table's other sub-indexes (format 1: one block each per packet; the egress table's format 2 reads
    # none, their source being no Pod of a rule)
    free = (ref["info"]["cat"] == cc.FREE) & np.array([c.direction[int(f)] == "In" for f in ref["info"]["aim"]])
    assert free.sum() >= 50 and not emu.pkt_scan(len(got))[free].any()
    subs = emu.composite_layout(clf)[cc.TABLE["In"]]
    assert {s["fmt"] for s in subs} == {1}
    plain = {k: cols[k][free] for k in ("src", "dst", "sport", "dport", "proto", "out_port")}  # +new, no bypass
    assert _dir_block_loads(clf, plain) == int(free.sum()) * (len(subs) - 1)
    # every entry of the combination lists passes with its own id alone: not with bit 8 flipped (the
    # `hi` byte), not with bit 0 flipped, not with 0
    for d in ("In", "Out"):
        k = emu.combo_entry_check(clf, cc.TABLE[d])
        assert k["entries"] > 0 and k["pass_own_id"] == k["entries"], k
        assert k["pass_bit8_flipped"] == k["pass_bit0_flipped"] == k["pass_id0"] == 0, k
        assert (k["id_above_255"] > 0) == (name == "dense"), k
    got, counted = cc.emulate(twin, cols)
    cc.same(got, ref["want"], cols, "GPC_NO_COMBO twin against the oracle")
    assert counted == ref["metrics"]
    if name == "tiny":  # without the override the 40-host groups stay under the production threshold
        assert COMBO not in cc.bands(cc.classifier(c, monkeypatch, env={"GPC_COMBO_MIN_ENTRIES": "65536"}), "In")


# ----------------------------------------------------------------------------------------- layouts
VARIANTS = [{"GPC_CBAND_MERGE": "0"}, {"GPC_CBAND_MERGE": "1"}, {"GPC_CBAND_MERGE": "3"},
            {"GPC_COMPOSITE_DIR": "0"}, {"GPC_COMPOSITE_DIR": "1"}, {"GPC_COMPOSITE_DIR": "2"},
            {"GPC_COMPOSITE_EXTRA_BITS": "0"}, {"GPC_COMPOSITE_EXTRA_BITS": "3"},
            {"GPC_NO_EXACT_X": "1"}, {"GPC_NO_EXACT_MULTI": "1"}, {"GPC_NO_PRESENCE": "1", "GPC_COMPOSITE_DIR": "0"},
            {"GPC_COMPOSITE": "0"}]


def _small_c3():
    """(rules, columns, oracle verdicts, oracle metrics) of a 2 000-rule C3. C3's services are one
    port or one range each; every 97th rule takes two more single ports, so that multi-interval
    exact entries (GPC_NO_EXACT_MULTI) occur."""
    wl = workload.config3(n_policies_per_dir=20, rules_per_policy=50)
    for r in wl.rules[::97]:
        s = r["service"][0]
        r["service"] = [{"protocol": s["protocol"], "port": min(65535, s["port"] + k)} for k in (0, 2, 4)]
    cols = workload.gen_packets(wl, 3000, seed=31)
    rng = np.random.default_rng(31)
    cols["ct_state"] = rng.choice([0x21, 0x21, 0x21, 0x20, 0x22], 3000).astype(np.uint8)
    cols["dest"] = rng.choice([0, 0, 0, 0, 1, 2, 3], 3000).astype(np.uint8)
    want, metrics = cc.Oracle(wl.rules).run(cols)
    return wl.rules, cols, want, metrics


def _layout_ids(v):
    return ",".join("%s=%s" % (k[4:], x) for k, x in v.items())


@pytest.mark.parametrize("name", ["dense", "C3s"])
def test_layout_variants(name, monkeypatch):
    """Every layout build_composite can be steered to (the IPv4 counterpart of
    tests/test_ipv6.py test_lpm_layout_variants): each equals the oracle in verdicts and counters --
    so all give byte-equal verdicts --, and each image differs from the default's. One classifier per
    rule set: a compaction rebuilds its image under the variant's variables, which the builder reads
    at every build. GPC_NO_PRESENCE only bears on format 0, so it is set together with it and its
    image must differ from format 0's own."""
    if name == "dense":
        ref = cc.reference(name)
        rules, cols, want, metrics = ref["case"].wl.rules, ref["cols"], ref["want"], ref["metrics"]
    else:
        rules, cols, want, metrics = _small_c3()
    clf = gpc.Classifier()
    clf.initialize()
    clf.batch_install_policy_rule_flows(copy.deepcopy(rules))
    emu.commit_host(clf)
    default = _image(clf)
    layout0 = emu.composite_layout(clf)
    tables = [t for t in cc.TABLE.values()]
    assert all(layout0[t] for t in tables)
    got, counted = cc.emulate(clf, cols)
    cc.same(got, want, cols, "default")
    assert counted == metrics
    images = {}
    for v in VARIANTS:
        with monkeypatch.context() as m:
            for k, x in v.items():
                m.setenv(k, x)
            builds = clf.image_stats()["n_full_builds"]
            emu.commit_host(clf, full=True)
            assert clf.image_stats()["n_full_builds"] == builds + 1
        key = _layout_ids(v)
        images[key] = _image(clf)
        assert images[key] != default, key
        layout = emu.composite_layout(clf)
        got, counted = cc.emulate(clf, cols)
        cc.same(got, want, cols, key)
        assert counted == metrics, key
        subs = [s for t in tables for s in layout[t]]
        if "GPC_COMPOSITE" in v:
            assert not subs
            continue
        if "GPC_COMPOSITE_DIR" in v:
            assert {s["fmt"] for s in subs} == {int(v["GPC_COMPOSITE_DIR"])}, key
        if v.get("GPC_CBAND_MERGE") == "0" and name == "C3s":  # every band keyed at band 0's granularity
            assert {s["band"] for s in subs} == {0}, layout
        if v.get("GPC_CBAND_MERGE") == "3" and name == "C3s":  # host addresses keyed with the /25 .. /31
            assert 4 not in {s["band"] for s in subs} and 3 in {s["band"] for s in subs}, layout
        if "GPC_COMPOSITE_EXTRA_BITS" in v:
            d = int(v["GPC_COMPOSITE_EXTRA_BITS"]) - 2
            assert [s["bits"] for t in tables for s in layout[t]] != [s["bits"] for t in tables for s in layout0[t]]
            assert all(s["bits"] - s0["bits"] in (d, 0) for t in tables for s, s0 in zip(layout[t], layout0[t]))
        if v.get("GPC_COMPOSITE_EXTRA_BITS") == "0":  # overflow buckets: a pointer entry plus six inert ones
            assert max(s["longest"] for s in subs) >= emu.DIR_COUNT_MAX, layout
        if name == "dense" and "GPC_CBAND_MERGE" not in v:
            assert all(COMBO in [s["band"] for s in layout[t]] for t in tables), key
    assert images["NO_PRESENCE=1,COMPOSITE_DIR=0"] != images["COMPOSITE_DIR=0"] or name == "dense"
    assert len(set(images.values())) >= len(images) - 2  # (the directory format a table has anyway repeats the default's for it)


# ------------------------------------------------------------------------------------ delta epochs
@pytest.mark.parametrize("env", [{}, {"GPC_EXT_PLAIN": "1"}, {"GPC_NO_EXTENSIONS": "1"}], ids=["default", "ext-plain", "no-extensions"])
def test_delta_epochs_over_combination_base(env, monkeypatch):
    """tests/combo_cases.py delta_script over the committed `dense` base, one delta epoch per step
    (compact_after=-1): after every step the delta classifier's verdicts and per-rule counters equal
    the oracle compiler's replay and a twin that rebuilds its whole image (the twin has no
    extensions, so the default run's twin serves the other two runs through the oracle's equality).
    Then a compaction: the combination band is back, the verdicts are unchanged."""
    ref = cc.reference("dense")
    c, cols = ref["case"], ref["cols"]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    a = cc.classifier(c, monkeypatch, compact_after=-1)
    b = cc.classifier(c, monkeypatch, compact_after=-1) if not env else None
    z = c.delta
    prev = ref["want"]
    n_ext = 0
    for label, ops, want, metrics in cc.delta_reference("dense"):
        cc.apply(a, ops)
        emu.commit_host(a)
        got, counted = cc.emulate(a, cols)
        cc.same(got, want, cols, "%s: delta epoch against the oracle's replay" % label)
        assert counted == metrics, label
        if b is not None:
            cc.apply(b, ops)
            emu.commit_host(b, full=True)
            full, counted = cc.emulate(b, cols)
            cc.same(got, full, cols, "%s: delta epoch against the full rebuild" % label)
            assert counted == metrics, label
            assert b.image_stats()["n_overlay_rules"] == 0
        assert (want != prev).any(), "%s moves no verdict of the batch" % label
        st = a.image_stats()
        assert st["n_full_builds"] == 1, st
        for d in ("In", "Out"):  # the base image still holds its combination lists
            assert COMBO in cc.bands(a, d)
        if label.startswith("add") and "GPC_NO_EXTENSIONS" not in env:  # point extensions, no journaled rule
            assert st["n_ext_values"] > n_ext and st["n_ext_rules"] == 2 and st["n_overlay_rules"] == 0, (label, st)
            n_ext = st["n_ext_values"]
        if label == "del base_member":  # a journal version of the rule plus a tombstone of its base record
            assert st["n_overlay_rules"] >= 2 and st["n_tombstones"] >= 2, st
            for d, col, stage in (("In", "src", 1), ("Out", "dst", 0)):
                m = (cols[col] == z[d]["base_member"]) & (ref["info"]["aim"] == z[d]["shared"])
                assert (prev[m][:, stage]["conj_id"] == z[d]["shared"]).any(), d  # (a condition on the case)
                assert not (got[m][:, stage]["conj_id"] == z[d]["shared"]).any(), d  # the host lost this rule ...
                m = (cols[col] == z[d]["base_member"]) & (ref["info"]["aim"] == z[d]["ext"])
                assert (got[m] == prev[m]).all() and m.any(), d  # ... and only this one of its group
        prev = want
    emu.commit_host(a, full=True)
    st = a.image_stats()
    assert st["n_full_builds"] == 2 and st["n_overlay_rules"] == 0 and st["n_tombstones"] == 0, st
    for d in ("In", "Out"):
        assert COMBO in cc.bands(a, d)
    got, counted = cc.emulate(a, cols)
    cc.same(got, prev, cols, "after the compaction")
    assert counted == metrics


# ------------------------------------------------------------------------------------------- trace
def trace_rows(ref, n):
    """n packets of the batch: decided by a group rule in ingress, in egress, and the head."""
    want = ref["want"]
    c = ref["case"]
    rows = []
    for d, stage in (("In", 1), ("Out", 0)):
        rules = c.group_rules(d)
        rows += list(np.nonzero(np.isin(want[:, stage]["conj_id"], rules))[0][:2 * n // 5])
    rows += [i for i in range(len(want)) if i not in rows][:n - len(rows)]
    return np.array(sorted(rows))


def test_trace_over_combination_base(monkeypatch):
    """emu.trace (the walk of gpc_trace) of 50 packets on the `dense` base: table sequence, decisions
    and final verdicts equal the oracle's own walk of the flows."""
    from tests.test_trace import _check
    ref = cc.reference("dense")
    clf = cc.classifier(ref["case"], monkeypatch)
    pipe = ovs_cls.Pipeline(ref["flows"], ref["tiers"])
    rows = trace_rows(ref, 50)
    cols = {k: v[rows] for k, v in ref["cols"].items()}
    kinds = _check(pipe, clf, cols, emu.trace, 50)
    assert {1, 2, 3} <= kinds, kinds
