"""gpc_trace6, CPU tier (tests/trace6_util.py): the trace of an IPv6 packet composed on the host from
the pieces the device kernel calls -- the Service stage (lb_stage6), the LPM coding (v6_codes<1>) and
the traced walk over the codes -- equals the oracle's own walk of the same flows, table by table, over
the whole native batch of tests/v6_cases.py on the base epoch, after delta epochs and behind IPv6
Services; and the host translation of an LPM code back to its prefix
(gpc_debug_v6_prefix_of_code, what gpc_trace6 reports per address column) equals the longest prefix
of the flow text that holds the address.

What the cases are worth is asserted on the references alone: the oracle's traces hold misses, allows,
drops and passes, walks of 1, 4 and 6 tables and every rule table; the addresses fall into prefixes of
at least 25 lengths, the word boundaries and "none" among them, and on the delta path into a prefix of
every length the delta commits brought."""
import collections

import numpy as np
import pytest

from antrea_amd import gpc
from tests import emu, trace6_util as tu, v6_cases as vc

N = vc.N_BATCH
_STATE = {}


def _state(path):
    """Per path, built once: workload, classifier (host commits), the native batch, the oracle."""
    if path not in _STATE:
        w6 = vc.workload_of(path, tu.SEED)
        c = vc.make_classifier(path, w6, emu.commit_host)
        cols, opt, info = vc.native_packets(w6, tu.SEED)
        _STATE[path] = {"w6": w6, "c": c, "cols": cols, "opt": opt, "oracle": tu.Oracle(path, w6)}
    return _STATE[path]


def _want(s):
    if "want" not in s:
        s["want"] = tu.oracle_traces(s["oracle"], s["c"], s["cols"], N)
    return s["want"]


@pytest.mark.parametrize("path", ["base", "delta", "svc6"])
def test_emulated_trace6_equals_the_oracle_trace(path):
    s = _state(path)
    want = _want(s)
    got = tu.emu_trace6(s["c"], s["cols"], N)
    for i in range(N):
        tu.same_trace(got[i][0], got[i][1], want[i], (path, i))
    if path == "svc6":  # the batch meets every kind of Service-stage outcome
        flags = np.array([g[2]["flags"] for g in got])
        assert ((flags & gpc.LB_DNAT) != 0).any() and ((flags & gpc.LB_NO_ENDPOINT) != 0).any() and (flags == 0).any()
        assert all(not w[1] for w, g in zip(want, got) if g[2]["flags"] & gpc.LB_NO_ENDPOINT)


def test_the_oracle_traces_cover_the_walk():
    want = _want(_state("base"))
    decisions = collections.Counter(st[1] for _, steps in want for st in steps)
    walks = collections.Counter(len(steps) for _, steps in want)
    tables = {st[0] for _, steps in want for st in steps}
    assert {1, 2, 3, 7} <= set(decisions), decisions     # miss, allow, drop, pass
    assert {1, 4, 6} <= set(walks), walks
    assert tables == {1, 2, 3, 4, 5, 6}


def _addresses(s):
    return np.concatenate([s["cols"]["src6"], s["cols"]["dst6"], s["opt"]["ct_src6"], s["opt"]["ct_dst6"]])


@pytest.mark.parametrize("path", ["base", "delta"])
def test_code_translation_equals_the_flow_text_lpm(path):
    s = _state(path)
    addrs = _addresses(s)
    codes = emu.v6_codes(s["c"], addrs)[0]
    prefix_of = {int(code): s["c"].v6_prefix_of_code(int(code)) for code in np.unique(codes)}
    for i, a in enumerate(addrs):
        tu.check_prefix(prefix_of[int(codes[i])], tu.addr_int(a), s["oracle"], path == "base", (path, i))
    assert len({p for p in prefix_of.values() if p is not None}) > 40


def test_the_addresses_cover_the_prefix_lengths():
    s = _state("base")
    lens = tu.length_classes(s["oracle"], _addresses(s))
    assert len(lens) >= 25 and {0, 1, 32, 33, 64, 65, 96, 97, 127, 128} <= set(lens), sorted(lens)
    d = _state("delta")
    dl = tu.length_classes(d["oracle"], _addresses(d))
    assert set(vc.NEW_LENGTHS) <= set(dl), sorted(dl)
    assert not set(vc.NEW_LENGTHS) & {n.prefixlen for n in d["oracle"].base_nets}  # brought by the delta commits


def test_unowned_codes_and_missing_image_are_einval():
    """Of 256 random codes every one the tree owns translates to a prefix of the flow text; the tree
    holds a few hundred nodes, so (almost) none of 256 codes drawn from 2^32 is owned."""
    s = _state("base")
    rng = np.random.default_rng(11)
    unowned = 0
    for code in rng.integers(1, 1 << 32, 256):
        try:
            p = s["c"].v6_prefix_of_code(int(code))
            assert p in s["oracle"].nets, (hex(int(code)), p)
        except gpc.GpcError as e:
            assert e.code == gpc.GPC_EINVAL
            unowned += 1
    assert unowned >= 250
    assert s["c"].v6_prefix_of_code(0) is None  # under no prefix of the rule set
    fresh = gpc.Classifier(ipv4=False, ipv6=True)
    fresh.initialize()
    with pytest.raises(gpc.GpcError) as e:  # before an IPv6 image exists
        fresh.v6_prefix_of_code(0)
    assert e.value.code == gpc.GPC_EINVAL
    v4 = gpc.Classifier()
    v4.initialize()
    emu.commit_host(v4)
    with pytest.raises(gpc.GpcError) as e:  # IPv6 disabled: never one
        v4.v6_prefix_of_code(0)
    assert e.value.code == gpc.GPC_EINVAL
