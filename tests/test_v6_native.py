"""IPv6 classification of native prefixes (tests/v6_cases.py), CPU tier: prefixes of every length class
anywhere in the address space -- below 32 bits, on and next to the 32-bit word boundaries, a nested
chain, /128s that differ in one word only -- in rules of small C3, packets aimed at their first,
last, an inner and the first outer address. The host emulation of the kernel body over the
product's IPv6 image equals the Python oracle, on the base epoch and after delta epochs that bring
new prefix lengths, with and without ct address columns, and in a dual-stack context; and the LPM
instantiation the device runs (one address per search, descriptors from a copy) gives the code of
the instantiation the emulation runs, address by address.

What the cases are worth is asserted on the oracle's verdicts alone (v6_cases.sensitivity): for
every length some (inside, just outside) pair of packets is decided differently, and the chain's
packets are decided by at least three different conjunctions. With seed 3 the oracle decides 166 of
the 640 packets otherwise than it would without the native prefixes.

Faults this file was tried against (each put into the emulation's copy of core.hpp / emu.cpp alone,
the image builder left as it is), and the tests that fail then:
  * v6_codes taking word 0 of every address for the embedding's: test_native_emu_vs_oracle,
    test_native_ct_columns_emu_vs_oracle, test_dual_stack_native;
  * v6_key one bit short at lengths 32 and 64: the same three (of the older tests, both faults are
    seen only where addresses leave fd00:10::/96: the multi48 cases, whose region tables key on /48
    and /64, the eight sources of test_new_prefix_lengths_are_incremental, tests/test_affinity6.py);
  * v6_codes<1> skipping the probe of the delta epochs' new lengths after the search:
    test_device_lpm_instantiation_equals_the_emulations[delta] alone, and no older test (the
    emulation classifies through <2>, so its verdicts stay right -- the device's would not);
  * emu_classify6 reading ct_dst6 for ct_src: test_native_ct_columns_emu_vs_oracle[*-both],
    test_dual_stack_native, and no older test."""
import copy

import numpy as np
import pytest

from antrea_amd import gpc, workload
from tests import emu, v6_cases as vc
from tests.test_ipv6 import _oracle6
from tests.test_ipv6_delta import _oracle_after

SEED = 3
N = vc.N_BATCH
_STATE = {}


def _state(path):
    """Per path, built once: workload, classifier, batch; _want: the oracle's verdicts without and
    with the ct address columns, computed once (left unchanged by every test)."""
    if path not in _STATE:
        w6 = vc.workload_of(path, SEED)
        c = vc.make_classifier(path, w6, emu.commit_host)
        cols, opt, info = vc.native_packets(w6, SEED)
        ct = dict(cols, ct_src6=opt["ct_src6"], ct_dst6=opt["ct_dst6"])
        _STATE[path] = {"w6": w6, "c": c, "cols": cols, "opt": opt, "info": info, "ct": ct, "path": path}
    return _STATE[path]


def _want(s, key="want"):
    if key not in s:
        s[key] = vc.oracle6(s["w6"].rules, s["ct" if key == "want_ct" else "cols"], N, vc.log_of(s["path"], s["w6"]))
    return s[key]


def test_cases_depend_on_the_native_prefixes():
    """The condition on the reference: per length an (inside, just outside) pair the oracle decides
    differently, at least three deciding conjunctions along the chain, ct cases on both sides that
    decide, and both /128s of the word-0 and of the word-3 pair."""
    s = _state("base")
    differ, decided = vc.sensitivity(_want(s), s["info"])
    for plen in vc.LENGTHS:
        assert differ[("len", plen)] >= 1, (plen, differ)
    for plen in vc.CHAIN:
        assert differ[("chain", plen)] == 1, (plen, differ)
    assert differ[("word0", 128)] == 2 and differ[("word3", 128)] == 2, differ
    assert len(decided) >= 3, decided
    ct_differ, _ = vc.sensitivity(_want(s, "want_ct"), s["info"], ct=True)
    sides = {c.side for c in s["info"]["cases"] if c.ct and ct_differ[(c.group, c.prefix.prefixlen)]}
    assert sides == {"from", "to"} and sum(ct_differ.values()) >= 4, ct_differ
    assert (_want(s, "want_ct") != _want(s)).any(axis=1).sum() >= 8  # the ct columns change verdicts
    # the same oracle as the other IPv6 tests' (which pass no ct columns on)
    assert _oracle6(s["w6"].rules, vc.head(s["cols"], 60), 60, ipv4=False).tobytes() == _want(s)[:60].tobytes()


def test_delta_cases_hit_the_added_prefixes():
    s, b = _state("delta"), _state("base")
    differ, _ = vc.sensitivity(_want(s), s["info"])
    for plen in vc.NEW_LENGTHS + (64,):
        assert differ[("new", plen)] >= 1, (plen, differ)
    assert not any(g == "new" for g, _ in vc.sensitivity(_want(b), b["info"])[0])  # (not before the log)
    assert differ[("chain", 60)] == 0 and vc.sensitivity(_want(b), b["info"])[0][("chain", 60)] == 1  # the deleted member
    sub = vc.head(s["cols"], 60)
    assert _oracle_after(s["w6"].rules, s["w6"].log, sub, 60, False).tobytes() == _want(s)[:60].tobytes()


@pytest.mark.parametrize("path", ["base", "delta"])
def test_native_emu_vs_oracle(path):
    s = _state(path)
    got = vc.emulation(s["c"], s["cols"])
    vc.cmp6(got, _want(s), s["cols"])
    assert {1, 2, 3} <= set(np.unique(got["action"]).tolist())


@pytest.mark.parametrize("present", ["ct_src6", "ct_dst6", "both"])
@pytest.mark.parametrize("path", ["base", "delta"])
def test_native_ct_columns_emu_vs_oracle(path, present):
    s = _state(path)
    names = ("ct_src6", "ct_dst6") if present == "both" else (present,)
    cols = dict(s["cols"], **{k: s["opt"][k] for k in names})
    want = _want(s, "want_ct") if present == "both" else vc.oracle6(s["w6"].rules, cols, N, vc.log_of(path, s["w6"]))
    vc.cmp6(vc.emulation(s["c"], cols), want, cols)
    assert (want != _want(s)).any(axis=1).sum() >= 4


@pytest.mark.parametrize("path", vc.PATHS)
def test_device_lpm_instantiation_equals_the_emulations(path):
    """v6_codes<1> over a copy of the descriptors (classify.hip v6_code_kernel) == v6_codes<2> over
    the image's (tests/csrc/emu.cpp emu_classify6), for every address of the native batch."""
    s = _state(path)
    addrs = np.concatenate([s["cols"]["src6"], s["cols"]["dst6"], s["opt"]["ct_src6"], s["opt"]["ct_dst6"]])
    one, pair = emu.v6_codes(s["c"], addrs)
    assert (one == pair[:, 0]).all() and (np.roll(one, -1) == pair[:, 1]).all()
    assert len(np.unique(one)) > 60


VARIANTS = {"default": {}, "one_tag": {"GPC_V6_MAX_TAGS": "1"}, "leaf0": {"GPC_V6_LEAF_LENS": "0"}, "leaf8": {"GPC_V6_LEAF_LENS": "8"}}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_native_under_region_tables(variant, monkeypatch):
    """The native prefixes under the four /48s of the multi48 embedding, where the LPM has region
    tables and sub-region tables (core.hpp V6Lpm): prefixes end inside, on and below the tables'
    levels, shorter ones hold whole regions. Every layout variant == the oracle, by both
    instantiations of the search, and the lookups do descend the tables."""
    if "regions" not in _STATE:
        w6, _ = vc.native_workload(SEED, embed="multi48")
        cols, opt, info = vc.native_packets(w6, SEED)
        ct = dict(cols, ct_src6=opt["ct_src6"], ct_dst6=opt["ct_dst6"])
        want = vc.oracle6(w6.rules, ct, N)
        differ, decided = vc.sensitivity(vc.oracle6(w6.rules, cols, N), info)
        assert all(differ[("len", plen)] for plen in vc.LENGTHS) and all(differ[("chain", plen)] for plen in vc.CHAIN), differ
        _STATE["regions"] = (w6, ct, want)
    w6, ct, want = _STATE["regions"]
    for k, v in VARIANTS[variant].items():
        monkeypatch.setenv(k, v)
    c = vc.make_classifier("base", w6, emu.commit_host)
    emu.stats(reset=True)
    vc.cmp6(vc.emulation(c, ct), want, ct)
    assert emu.stats()[14] > 0  # sub-region tables descended
    one, pair = emu.v6_codes(c, np.concatenate([ct["src6"], ct["dst6"], ct["ct_src6"], ct["ct_dst6"]]))
    assert (one == pair[:, 0]).all() and (np.roll(one, -1) == pair[:, 1]).all()


def test_dual_stack_native():
    """The IPv4 peers stay in every list: the IPv6 verdicts are those of the IPv6-only context, and
    the context's IPv4 verdicts are those of the same dual-stack rules without native prefixes."""
    s = _state("base")
    wl = workload.config3(seed=SEED, n_policies_per_dir=6, rules_per_policy=8)
    dual, _ = vc.native_workload(SEED, dual=True)
    assert [c for c in dual.cases] == [c for c in s["w6"].cases]
    assert any(isinstance(a, dict) and "." in a.get("ipnet", "") for r in dual.rules for a in r.get("from") or [])
    c = vc.make_classifier("base", dual, emu.commit_host, ipv4=True)
    for cols, want in ((s["cols"], _want(s)), (s["ct"], _want(s, "want_ct"))):
        vc.cmp6(vc.emulation(c, cols), want, cols)
    plain = gpc.Classifier(ipv4=True, ipv6=True)
    plain.initialize()
    plain.batch_install_policy_rule_flows(copy.deepcopy(workload.to_ipv6(wl, dual=True).rules))
    emu.commit_host(plain)
    cols4 = workload.gen_packets(wl, 3000, seed=SEED)
    got4 = emu.classify(c, cols4)
    vc.cmp6(got4, emu.classify(plain, cols4), cols4)
    assert (got4["action"] == 2).any() and (got4["action"] == 3).any()
