"""GPU tier: the one-launch kernels (both policy stages per lane) after the reordering of their
memory chain -- header reads through the constant address space, one round of column loads, the
egress half parked in LDS and one 16-B store per packet after both stages' counter adds.

Every check runs on four paths: the base kernel, the extension-mode kernel (one
AddPolicyRuleAddress committed as a delta epoch), the grouped path (group_packets=1) and a Service
kernel (C1 with Services, LB results requested). The device is compared with the host emulation of
the same epoch (verdicts, LB results, counters) and, where the oracle models the columns (none,
ct_state / dest / ct_mark), with the oracle's walk of the flows."""
import copy

import numpy as np
import pytest

from antrea_amd import gpc, workload
from tests import emu
from tests.test_emu_parity import _cmp, oracle_verdicts

pytestmark = pytest.mark.gpu

PATHS = ("base", "ext", "grouped", "svc")
OPTIONAL = ("ct_src", "ct_dst", "in_port", "svc_group", "tun_id", "ct_state", "dest", "ct_mark", "len")
N_POOL = 6000  # packets the 64-packet counter batch is picked from
GUARD = 64
FILL = 0xA5


@pytest.fixture(scope="module", autouse=True)
def _built():
    from antrea_amd.build import build
    build()
    import torch
    assert torch.cuda.is_available(), "GPU tier needs a HIP device"


def workload_of(path):
    """C1 (for the Service path with Services) plus one counted AntreaClusterNetworkPolicy egress Drop
    rule over the first K8s egress rule's Pods, first peer and service, so that packets exist which
    are counted in egress and dropped there (C1's own drops are uncounted isolation drops)."""
    if path == "svc":
        from tests.test_service import _svc_workload
        wl = _svc_workload("C1", 61)
    else:
        wl = workload.config1(seed=5)
    r = next(r for r in wl.rules if r["direction"] == "Out" and r.get("from") and r.get("to") and r.get("service"))
    wl.rules.append({"direction": "Out", "table": "AntreaPolicyEgressRule", "action": "Drop",
                     "flow_id": max(x["flow_id"] for x in wl.rules) + 1, "policy_type": "AntreaClusterNetworkPolicy",
                     "policy_namespace": "", "policy_name": "fused-chain-drop", "policy_uid": "uid-fused-chain-drop",
                     "name": "rule-0", "tier_priority": 50, "priority": 54953, "service": copy.deepcopy(r["service"][:1]),
                     "from": copy.deepcopy(r["from"]), "to": copy.deepcopy(r["to"][:1])})
    return wl


def make_classifier(path, wl, commit):
    """The path's classifier with its rule set committed through `commit`."""
    c = gpc.Classifier(group_packets=1 if path == "grouped" else 0)
    c.initialize()
    c.batch_install_policy_rule_flows(copy.deepcopy(wl.rules))
    if path == "svc":
        workload.install_services(c, wl)
    commit(c)
    if path == "ext":  # one added address: a point extension over the base (no journal walk)
        r = next(r for r in wl.rules if r.get("from"))
        c.add_policy_rule_address(r["flow_id"], "src", ["10.250.250.250"], r.get("priority"))
        commit(c)
    return c


def optional_columns(cols, seed):
    """Random values for every optional column (values the rule sets and the bypasses react to)."""
    n = len(cols["src"])
    rng = np.random.default_rng(seed)
    o = {}
    o["ct_src"] = cols["src"][rng.permutation(n)].astype(np.uint32)
    o["ct_dst"] = cols["dst"][rng.permutation(n)].astype(np.uint32)
    o["in_port"] = cols["out_port"][rng.permutation(n)].astype(np.uint32)
    o["svc_group"] = rng.integers(0, 4, n).astype(np.uint32)
    o["tun_id"] = rng.integers(0, 3, n).astype(np.uint32)
    u = rng.random(n)  # +new+trk / +trk (-new: no session) / +est+trk
    o["ct_state"] = np.where(u < 0.6, 0x21, np.where(u < 0.85, 0x20, 0x22)).astype(np.uint8)
    o["dest"] = rng.choice([0, 0, 1, 2, 3], n).astype(np.uint8)
    o["ct_mark"] = np.where(rng.random(n) < 0.25, 0x40, rng.choice([0, 0x10, 0x20], n)).astype(np.uint8)
    o["len"] = rng.integers(1, 65536, n).astype(np.uint16)
    return o


def default_columns(cols):
    """Every optional column present with the value its absence stands for (len: no verdict effect)."""
    n = len(cols["src"])
    return {"ct_src": cols["src"].astype(np.uint32), "ct_dst": cols["dst"].astype(np.uint32),
            "in_port": np.zeros(n, np.uint32), "svc_group": np.zeros(n, np.uint32), "tun_id": np.zeros(n, np.uint32),
            "ct_state": np.full(n, 0x21, np.uint8), "dest": np.zeros(n, np.uint8), "ct_mark": np.zeros(n, np.uint8),
            "len": np.full(n, 100, np.uint16)}


def counted_stages(c, cols, i, v):
    """(egress counted, ingress counted) of packet i, from the emulation of the packet alone."""
    _, slots = c.counters()
    arr = np.zeros((max(1, len(slots)), 3), np.uint64)
    emu.classify(c, {k: a[i:i + 1] for k, a in cols.items()}, counters=arr)
    hit = [slots[s] for s in np.nonzero(arr[:, 0])[0] for _ in range(int(arr[s, 0]))]
    if len(hit) == 2:
        return True, True
    if not hit:
        return False, False
    e = hit[0] == int(v[i, 0]["conj_id"]) and int(v[i, 0]["action"]) in (2, 3, 4)
    if e and hit[0] == int(v[i, 1]["conj_id"]) and int(v[i, 1]["action"]) in (2, 3, 4):
        return None, None  # one conjunction decides both stages: ambiguous, not picked
    return e, not e


def counter_batch(c, wl, seed=5):
    """A 64-packet batch (with ct_state, dest, ct_mark and len columns) that holds a packet counted
    in both stages, one counted in egress only and dropped there, one counted in ingress only, one
    that takes the ingress bypass (dest = gateway) and one that is not counted at all; the rest are
    the pool's first packets. Returns (cols, {case: row})."""
    pool = workload.gen_packets(wl, N_POOL, seed=seed)
    rng = np.random.default_rng(seed)
    u = rng.random(N_POOL)
    pool["ct_state"] = np.where(u < 0.7, 0x21, np.where(u < 0.9, 0x20, 0x22)).astype(np.uint8)
    pool["dest"] = np.where(rng.random(N_POOL) < 0.15, 1, 0).astype(np.uint8)
    pool["ct_mark"] = np.zeros(N_POOL, np.uint8)
    pool["len"] = rng.integers(1, 1500, N_POOL).astype(np.uint16)
    v = emu.classify(c, pool)
    ea, ga = v[:, 0]["action"], v[:, 1]["action"]
    allow_deny = lambda a: (a == 2) | (a == 3) | (a == 4)
    shape = {"both": allow_deny(ea) & allow_deny(ga), "egress_dropped": ((ea == 3) | (ea == 4)) & (ga == 0),
             "ingress_only": (ea == 1) & allow_deny(ga), "bypass": (ga == 6) & (pool["dest"] == 1),
             "uncounted": (ea == 1) & (ga == 1)}
    want = {"both": (True, True), "egress_dropped": (True, False), "ingress_only": (False, True), "uncounted": (False, False)}
    pick = {}
    for case, m in shape.items():  # the verdicts' shape first, then the emulation's counters of the packet alone
        for i in np.nonzero(m)[0][:50]:
            if case == "bypass" or counted_stages(c, pool, int(i), v) == want[case]:
                pick[case] = int(i)
                break
    rows = list(pick.values()) + [i for i in range(N_POOL) if i not in pick.values()]
    rows = np.array(sorted(rows[:64]))
    cols = {k: a[rows] for k, a in pool.items()}
    return cols, {case: int(np.nonzero(rows == i)[0][0]) for case, i in pick.items()}


_STATE = {}


def _path(path):
    """Per path, built once: classifier, 130 packets, the emulation's verdicts of the plain columns."""
    if path not in _STATE:
        wl = workload_of(path)
        c = make_classifier(path, wl, lambda k: k.commit())
        cols = workload.gen_packets(wl, 130, seed=21)
        _STATE[path] = {"wl": wl, "c": c, "cols": cols, "opt": optional_columns(cols, 22)}
    return _STATE[path]


def _device(c, cols, n, count=False, lb=False):
    """gpc_classify over device columns into 0xA5-filled buffers with 64 guard bytes: returns the
    verdict pairs (n, 2) [and LB results (n,)], after checking that the guards are untouched."""
    import torch
    dev = torch.device("cuda", 0)
    signed = {4: np.int32, 2: np.int16, 1: np.uint8}  # the same bits in torch dtypes
    dcols = {k: torch.as_tensor(np.ascontiguousarray(a[:n], dtype=gpc.PKT_COLUMNS[k]).view(signed[np.dtype(gpc.PKT_COLUMNS[k]).itemsize])).to(dev)
             for k, a in cols.items()}
    out = torch.full((16 * n + GUARD,), FILL, dtype=torch.uint8, device=dev)
    lbo = torch.full((16 * n + GUARD,), FILL, dtype=torch.uint8, device=dev) if lb else None
    c.classify_device(gpc.pkt_soa_device(dcols), n, out.data_ptr(), count=count, lb_ptr=lbo.data_ptr() if lb else 0)
    torch.cuda.synchronize(dev)
    res = []
    for t, dt in ((out, gpc.VERDICT_DTYPE), (lbo, gpc.LB_DTYPE)):
        if t is None:
            continue
        h = t.cpu().numpy()
        assert (h[16 * n:] == FILL).all(), "guard bytes written"
        res.append(h[:16 * n].view(dt).copy())
    return (res[0].reshape(n, 2), res[1]) if lb else res[0].reshape(n, 2)


def _emu(c, cols, n, lb=False, counters=None):
    sub = {k: a[:n] for k, a in cols.items()}
    lbo = np.zeros(n, gpc.LB_DTYPE) if lb else None
    v = emu.classify(c, sub, counters=counters, lb=lbo)
    return (v, lbo) if lb else v


def _same_bytes(got, want, cols):
    """Every byte of the stored records equals the expected ones (the all-zero NONE half included)."""
    _cmp(got, want, cols)
    assert got.tobytes() == want.tobytes()


def _check(path, cols, n, count=False, counters=None):
    """Device run of the path over cols[:n] against the emulation: verdict pairs byte for byte (and
    the LB results on the Service path). Returns the device verdicts."""
    s = _path(path)
    lb = path == "svc"
    got = _device(s["c"], cols, n, count=count, lb=lb)
    want = _emu(s["c"], cols, n, lb=lb, counters=counters)
    if lb:
        assert got[1].tobytes() == want[1].tobytes()
        got, want = got[0], want[0]
    _same_bytes(got, want, cols)
    return got


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("path", PATHS)
def test_batch_sizes(path, n):
    """A partial last wave, one full wave, one lane past it: every byte of [0, 16 n) is the expected
    verdict pair and nothing is written behind it."""
    s = _path(path)
    cols = dict(s["cols"], dest=s["opt"]["dest"], ct_state=s["opt"]["ct_state"])  # drops, bypasses, NONE halves
    got = _check(path, cols, n)
    if n == 130:
        assert (np.ascontiguousarray(got[:, 1]).view(np.uint8).reshape(n, 8) == 0).all(axis=1).any(), "no ingress NONE half in the batch"
        assert (got[:, 1]["action"] == 6).any(), "no ingress bypass in the batch"


@pytest.mark.parametrize("present", ["none", "all", "defaults"] + list(OPTIONAL))
@pytest.mark.parametrize("path", PATHS)
def test_column_presence(path, present):
    """The same packets without optional columns, with all of them, with each alone, and with all of
    them holding the defaults (verdicts equal the run without columns)."""
    s = _path(path)
    n = 130
    base = s["cols"]
    if present == "none":
        cols = dict(base)
    elif present == "all":
        cols = dict(base, **s["opt"])
    elif present == "defaults":
        cols = dict(base, **default_columns(base))
    else:
        cols = dict(base, **{present: s["opt"][present]})
    got = _check(path, cols, n)
    if present == "defaults":
        _same_bytes(got, _emu(s["c"], base, n), base)
    if path == "base" and present in ("none", "ct_state", "dest", "ct_mark"):  # columns the oracle models
        want, _ = oracle_verdicts(s["wl"].rules, cols, n)
        _cmp(got, want, cols)


@pytest.mark.parametrize("with_len", [True, False], ids=["len", "nolen"])
@pytest.mark.parametrize("path", PATHS)
def test_counters_of_one_wave(path, with_len):
    """One 64-packet batch holding a packet counted in both stages, one counted in egress only and
    dropped there, one counted in ingress only, one taking the ingress bypass and one not counted,
    +new and -new: verdicts and per-rule {packets, bytes, sessions} equal the emulation's exactly."""
    s = _path(path)
    c = s["c"]
    if "batch" not in s:
        s["batch"] = counter_batch(c, s["wl"])
    cols, cases = s["batch"]
    assert set(cases) == {"both", "egress_dropped", "ingress_only", "bypass", "uncounted"}, cases
    assert {0x21, 0x20} <= set(int(x) for x in cols["ct_state"])
    if not with_len:
        cols = {k: a for k, a in cols.items() if k != "len"}
    _, slots = c.counters()
    arr = np.zeros((max(1, len(slots)), 3), np.uint64)
    c.reset_counters()
    _check(path, cols, 64, count=True, counters=arr)
    exp = {conj: tuple(int(x) for x in arr[i]) for i, conj in enumerate(slots) if conj and arr[i].any()}
    assert exp and (sum(v[1] for v in exp.values()) > 0) == with_len
    assert {k: tuple(v) for k, v in c.network_policy_metrics().items() if any(v)} == exp
