"""GPU tier: the classify kernels' tail after its reordering -- the packet length loaded with the
other columns and parked in the lane's LDS column (in the one-launch kernels in the upper half of
the word that holds the ingress-bypass result), the result stores issued before the counter adds.

Paths: the base kernel, the extension-mode kernel, the grouped path and a Service kernel (the
classifiers of tests/test_gpu_fused_chain.py, C1 with its extra counted egress Drop rule), a journal
epoch (a rule installed after the first commit) and one IPv6 classifier through classify6_device.
Every device run is compared with the host emulation of the same epoch: verdict pairs (and LB
results) byte for byte, per-rule {packets, bytes, sessions} exactly; on the base path also with the
oracle's walk of the flows and its Metric-table counters (it models ct_state, dest, ct_mark, len)."""
import copy

import numpy as np
import pytest

from antrea_amd import gpc
from oracle import parity
from tests import test_gpu_fused_chain as fc
from tests import test_gpu_v6_chain as v6
from tests import v6_cases as vc
from tests.test_emu_parity import _cmp, oracle_verdicts

pytestmark = pytest.mark.gpu

PATHS = fc.PATHS + ("journal",)
SIZES = (1, 63, 64, 65, 129)
LENS = (0, 1, 65535)  # no bytes add; the smallest; the top bit of the parked half-word set
HAIRPIN = 0x40
NEW, NOT_NEW, EST = 0x21, 0x20, 0x22


@pytest.fixture(scope="module", autouse=True)
def _built():
    from antrea_amd.build import build
    build()
    import torch
    assert torch.cuda.is_available(), "GPU tier needs a HIP device"


def _commit(c):
    c.commit()


def _device4(s, cols, n, count):
    """Device verdicts [and LB results] of cols[:n] and the nonzero per-rule metrics after the run."""
    c = s["c"]
    c.reset_counters()
    got = fc._device(c, cols, n, count=count, lb=s["lb"])
    return got, {k: tuple(v) for k, v in c.network_policy_metrics().items() if any(v)}


def _device6(s, cols, n, count):
    c = s["c"]
    c.reset_counters()
    got = v6._device(c, cols, n, count=count)
    return got, {k: tuple(v) for k, v in c.network_policy_metrics().items() if any(v)}


_STATE = {}


def _journal_classifier(wl):
    """C1 committed, then one more rule installed and committed as a delta epoch (journal mode)."""
    c = gpc.Classifier(compact_after=-1)
    c.initialize()
    c.batch_install_policy_rule_flows(copy.deepcopy(wl.rules))
    _commit(c)
    extra = dict(copy.deepcopy(wl.rules[1]), flow_id=max(r["flow_id"] for r in wl.rules) + 100)
    c.install_policy_rule_flows(copy.deepcopy(extra))
    _commit(c)
    assert c.image_stats()["n_overlay_rules"] > 0
    return c


def _path(path):
    """Per path, built once: classifier, the 64-packet counter batch of the fused-chain tests with
    the packet counted in both stages moved to row 0, and the rows of its cases."""
    if path not in _STATE:
        wl = fc.workload_of(path)
        c = _journal_classifier(wl) if path == "journal" else fc.make_classifier(path, wl, _commit)
        cols, cases = fc.counter_batch(c, wl)
        assert set(cases) == {"both", "egress_dropped", "ingress_only", "bypass", "uncounted"}, cases
        order = np.array([cases["both"]] + [i for i in range(64) if i != cases["both"]])
        cols = {k: a[order].copy() for k, a in cols.items()}
        cases = {k: int(np.nonzero(order == i)[0][0]) for k, i in cases.items()}
        _STATE[path] = {"path": path, "wl": wl, "c": c, "cols": cols, "cases": cases, "lb": path == "svc", "run": _device4}
    return _STATE[path]


def _emulate(s, cols, n, count):
    """Emulated verdicts [and LB results] and nonzero per-rule counters of cols[:n]."""
    c = s["c"]
    _, slots = c.counters()
    arr = np.zeros((max(1, len(slots)), 3), np.uint64)
    if s["path"] == "v6":
        want = v6._emu(c, cols, n, counters=arr if count else None)
    else:
        want = fc._emu(c, cols, n, lb=s["lb"], counters=arr if count else None)
    return want, {int(conj): tuple(int(x) for x in arr[i]) for i, conj in enumerate(slots) if conj and arr[i].any()}


def _check(s, cols, n, count=True):
    """One device run over cols[:n] against the emulation: records byte for byte, counters exactly;
    on the base path also against the oracle's verdicts and its Metric-table counters. Returns (verdict pairs, {conj: (packets, bytes, sessions)})."""
    got, dev = s["run"](s, cols, n, count)
    want, exp = _emulate(s, cols, n, count)
    if s["lb"]:
        assert got[1].tobytes() == want[1].tobytes()
        got, want = got[0], want[0]
    if s["path"] == "v6":
        v6._same_bytes(got, want, cols)
    else:
        fc._same_bytes(got, want, cols)
    assert dev == exp
    if s["path"] == "base":  # the oracle models every column of these batches (ct_state, dest, ct_mark, len)
        sub = {k: a[:n] for k, a in cols.items()}
        want, pipe = oracle_verdicts(s["wl"].rules, sub, n)
        _cmp(got, want, sub)
        if count:
            assert {k: tuple(v) for k, v in parity.oracle_metrics(pipe).items() if any(v)} == exp
    return got, exp


def _tile(cols, n):
    reps = -(-n // len(next(iter(cols.values()))))
    return {k: np.concatenate([a] * reps)[:n].copy() for k, a in cols.items()}


def _copies(cols, row, n=64):
    return {k: np.repeat(a[row:row + 1], n, axis=0) for k, a in cols.items()}


def _edge_batch(s):
    """The counter batch with len cycling over LENS, and three uncounted rows replaced by copies of the
    packet counted in both stages that take the ingress bypass: dest = gateway (len 65,535 and 0)
    and dest = gateway with the hairpin ct_mark (both bypasses: bit 8 of the parked word beside the
    packed length). Returns (cols, rows of the three)."""
    cols = {k: a.copy() for k, a in s["cols"].items()}
    cases = s["cases"]
    free = [i for i in range(64) if i not in cases.values()][:3]
    for k, a in cols.items():
        a[free] = a[0]
    cols["len"] = np.array([LENS[i % 3] for i in range(64)], np.uint16)
    cols["len"][0] = 65535
    cols["len"][cases["egress_dropped"]] = 1
    cols["len"][cases["ingress_only"]] = 65535
    cols["dest"][free] = 1
    cols["ct_mark"][free] = [0, 0, HAIRPIN]
    cols["len"][free] = [65535, 0, 65535]
    return cols, free


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("path", PATHS)
def test_partial_waves(path, n):
    """1, 63, 64, 65 and 129 packets with counters on and a len column at its edge values (lane 0 of
    every wave is counted in both stages): the records and the counters are the emulation's, and
    nothing is written behind the 16 n bytes (the guard check of the device helper)."""
    s = _path(path)
    cols, _ = _edge_batch(s)
    _, exp = _check(s, _tile(cols, n), n)
    assert exp and sum(v[1] for v in exp.values()) >= 65535


@pytest.mark.parametrize("path", PATHS)
def test_len_edges_and_bypass_flags(path):
    """len 0 / 1 / 65,535 in a present column, with packets counted in egress that take the plain
    ingress bypass and both bypasses: bytes counters and bypass flags exact."""
    s = _path(path)
    cols, (plain, plain0, both) = _edge_batch(s)
    got, exp = _check(s, cols, 64)
    for i in (plain, plain0, both):  # egress as the packet of row 0, the ingress bypass taken
        assert got[i, 0].tobytes() == got[0, 0].tobytes() and int(got[i, 1]["action"]) == 6 and int(got[i, 1]["conj_id"]) == 0
    assert int(got[plain, 1]["flags"]) == 0 == int(got[plain0, 1]["flags"]) and int(got[both, 1]["flags"]) == 2
    # row 0 and its three copies alone, on the device: the egress rule counts 4 packets, 3 x 65,535 bytes
    e = int(got[0, 0]["conj_id"])
    _, alone = _check(s, {k: a[[0, plain, plain0, both]] for k, a in cols.items()}, 4)
    assert alone[e][:2] == (4, 3 * 65535)


@pytest.mark.parametrize("path", PATHS)
def test_absent_len_and_counting_off(path):
    """Without a len column the bytes counters stay zero; with count=False and a len column present
    every counter stays zero and the verdicts are those of the counted run."""
    s = _path(path)
    cols, _ = _edge_batch(s)
    nolen = {k: a for k, a in cols.items() if k != "len"}
    got, exp = _check(s, nolen, 64)
    assert exp and all(v[1] == 0 for v in exp.values())
    off, none = _check(s, cols, 64, count=False)
    assert none == {} and off.tobytes() == got.tobytes()
    on, exp_len = _check(s, cols, 64)
    assert on.tobytes() == got.tobytes() and {k: (v[0], v[2]) for k, v in exp_len.items()} == {k: (v[0], v[2]) for k, v in exp.items()}


@pytest.mark.parametrize("case", ["both", "ingress_only"])
@pytest.mark.parametrize("path", PATHS)
def test_same_slots_in_every_lane(path, case):
    """64 copies of one packet counted in both stages (every lane adds to the same two slots), and of
    one counted in ingress only, len 65,535."""
    s = _path(path)
    cols = _copies(s["cols"], s["cases"][case])
    cols["len"][:] = 65535
    got, exp = _check(s, cols, 64)
    stages = (0, 1) if case == "both" else (1,)
    assert set(exp) == {int(got[0, j]["conj_id"]) for j in stages}
    assert sum(v[0] for v in exp.values()) == 64 * len(stages) and sum(v[1] for v in exp.values()) == 64 * 65535 * len(stages)


@pytest.mark.parametrize("path", PATHS)
def test_non_session_adds(path):
    """Connections that are not new (+trk without +new: the packets of an established connection
    that reach the policy tables; +est itself skips them) mixed with new ones in one wave on counted
    Allow rules: the third word is added for the lanes that are no sessions only."""
    s = _path(path)
    cols = {k: a.copy() for k, a in s["cols"].items()}
    both = _copies(s["cols"], 0, 32)
    for k in cols:
        cols[k][::2] = both[k]  # every other lane: the packet counted in both stages
    cols["ct_state"][:] = np.where(np.arange(64) % 4 < 2, NEW, NOT_NEW).astype(np.uint8)  # lanes 0, 4, ...: new; 2, 6, ...: not
    cols["ct_state"][1::8] = EST  # and a few lanes that skip the policy tables
    got, exp = _check(s, cols, 64)
    allow = {int(got[0, j]["conj_id"]) for j in (0, 1) if int(got[0, j]["action"]) == 2}
    assert allow, "the packet counted in both stages hits no Allow rule"
    for conj in allow:
        assert exp[conj][0] >= 32 and 16 <= exp[conj][0] - exp[conj][2]  # the 16 copies that are not new are no sessions


# ------------------------------------------------------------------------------------------ IPv6
def _path6():
    if "v6" not in _STATE:
        w6 = vc.workload_of("base", v6.SEED)
        c = vc.make_classifier("base", w6, _commit)
        native, _, _ = vc.native_packets(w6, v6.SEED)
        cols, rows = vc.counter_batch(w6, native)
        order = np.array([rows["both"]] + [i for i in range(64) if i != rows["both"]])
        cols = {k: a[order].copy() for k, a in cols.items()}
        cols["len"] = np.array([LENS[(i + 2) % 3] for i in range(64)], np.uint16)  # row 0: 65,535
        _STATE["v6"] = {"path": "v6", "w6": w6, "c": c, "cols": cols, "lb": False, "run": _device6}
    return _STATE["v6"]


@pytest.mark.parametrize("n", SIZES)
def test_ipv6_batch(n):
    """The IPv6 device path (code columns, then the same policy kernels): partial waves with counters
    on and len at its edge values."""
    s = _path6()
    _, exp = _check(s, _tile(s["cols"], n), n)
    k = s["w6"].counted
    assert {k["egress"], k["ingress"]} <= set(exp) and exp[k["egress"]][1] >= 65535
