"""GPU tier: the IPv6 launch sequence -- v6_lb_kernel (with Services), v6_code_kernel over 2, 3 or 4
address columns, the grouping pre-pass, the policy / resolved kernels, the un-permute -- at its
edges, as tests/test_gpu_fused_chain.py does for the IPv4 one-launch kernels.

The batch is the native one of tests/v6_cases.py (prefixes of every length class anywhere in the
address space, ct peers, packets at and next to every prefix's ends). Every check runs on four
paths: the base epoch, a delta epoch (v6_code_kernel<true>: new prefix lengths in the journal's
overflow table), the grouped path (group_packets=1) and C1 with IPv6 Services (LB results
requested). Columns are device columns through Classifier.classify6_device (classify6_lb_device
with Services); outputs go into 0xA5-filled buffers with 64 guard bytes behind the 16 n verdict
bytes and the 32 n LB bytes. The device is compared byte for byte with the host emulation of the
same epoch and, on the base and the delta path, with the Python oracle."""
import numpy as np
import pytest

from antrea_amd import gpc, workload
from tests import emu, v6_cases as vc

pytestmark = pytest.mark.gpu

PATHS = vc.PATHS
SEED = 3
N_ORACLE = 257
GUARD = 64
FILL = 0xA5


@pytest.fixture(scope="module", autouse=True)
def _built():
    from antrea_amd.build import build
    build()
    import torch
    assert torch.cuda.is_available(), "GPU tier needs a HIP device"


_STATE = {}


def _path(path):
    """Per path, built once: workload, classifier, the native batch and its optional columns."""
    if path not in _STATE:
        w6 = vc.workload_of(path, SEED)
        c = vc.make_classifier(path, w6, lambda k: k.commit())
        cols, opt, info = vc.native_packets(w6, SEED)
        _STATE[path] = {"w6": w6, "c": c, "cols": cols, "opt": opt, "info": info}
    return _STATE[path]


def _oracle(path, cols, key):
    """The oracle's verdicts of the first N_ORACLE packets, computed once per (path, column set)."""
    s = _path(path)
    if key not in s:
        s[key] = vc.oracle6(s["w6"].rules, vc.head(cols, N_ORACLE), N_ORACLE, vc.log_of(path, s["w6"]))
    return s[key]


def _upload(cols, n):
    import torch
    dev = torch.device("cuda", 0)
    signed = {4: np.int32, 2: np.int16, 1: np.uint8}  # the same bits in torch dtypes
    out = {}
    for k, a in cols.items():
        a = np.ascontiguousarray(a[:n], dtype=gpc.PKT_COLUMNS[k])
        out[k] = torch.as_tensor(a if a.ndim == 2 else a.view(signed[a.dtype.itemsize])).to(dev)
    return out


def _buffers(n, lb):
    import torch
    dev = torch.device("cuda", 0)
    out = torch.full((16 * n + GUARD,), FILL, dtype=torch.uint8, device=dev)
    lbo = torch.full((32 * n + GUARD,), FILL, dtype=torch.uint8, device=dev) if lb else None
    return out, lbo


def _launch(c, dcols, n, out, lbo, count=False, stream=0):
    soa = gpc.pkt_soa_device(dcols)
    if lbo is None:
        c.classify6_device(soa, n, out.data_ptr(), count=count, stream=stream)
    else:
        c.classify6_lb_device(soa, n, out.data_ptr(), lbo.data_ptr(), count=count, stream=stream)


def _read(n, out, lbo):
    """The verdict pairs (n, 2) [and LB results (n,)] of the buffers, after checking the guards."""
    res = []
    for t, size, dt in ((out, 16, gpc.VERDICT_DTYPE), (lbo, 32, gpc.LB6_DTYPE)):
        if t is None:
            continue
        h = t.cpu().numpy()
        assert (h[size * n:] == FILL).all(), "guard bytes written"
        res.append(h[:size * n].view(dt).copy())
    return (res[0].reshape(n, 2), res[1]) if lbo is not None else res[0].reshape(n, 2)


def _device(c, cols, n, lb=False, count=False):
    import torch
    dcols = _upload(cols, n)
    out, lbo = _buffers(n, lb)
    torch.cuda.synchronize()
    _launch(c, dcols, n, out, lbo, count=count)
    torch.cuda.synchronize()
    return _read(n, out, lbo)


def _emu(c, cols, n, lb=False, counters=None):
    lbo = np.zeros(n, gpc.LB6_DTYPE) if lb else None
    v = vc.emulation(c, cols, n, counters=counters, lb=lbo)
    return (v, lbo) if lb else v


def _same_bytes(got, want, cols):
    """Every byte of the stored records equals the expected ones (the all-zero NONE half included)."""
    vc.cmp6(got, want, cols)
    assert got.tobytes() == want.tobytes()


def _same(path, got, want, cols):
    if path == "svc6":
        assert got[1].tobytes() == want[1].tobytes()
        got, want = got[0], want[0]
    _same_bytes(got, want, cols)
    return got


def _check(path, cols, n, count=False, counters=None):
    """Device run of the path over cols[:n] against the emulation: verdict pairs byte for byte (and
    the LB results on the Service path). Returns the device verdicts (and LB results)."""
    s = _path(path)
    lb = path == "svc6"
    got = _device(s["c"], cols, n, lb=lb, count=count)
    _same(path, got, _emu(s["c"], cols, n, lb=lb, counters=counters), cols)
    return got


def _columns(s, present):
    base = s["cols"]
    if present == "none":
        return dict(base)
    if present == "all":
        return dict(base, **s["opt"])
    if present == "defaults":
        return dict(base, **vc.default_columns(base))
    return dict(base, **{present: s["opt"][present]})


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513])
@pytest.mark.parametrize("path", PATHS)
def test_batch_sizes(path, n):
    """A partial last wave and block, one full wave (the policy kernels' 64 lanes) and block (the code
    and Service kernels' 256), one lane past each, more than two blocks: every byte of [0, 16 n) and
    [0, 32 n) is the expected record and nothing is written behind them."""
    s = _path(path)
    cols = dict(s["cols"], dest=s["opt"]["dest"], ct_state=s["opt"]["ct_state"])  # drops, bypasses, NONE halves
    got = _check(path, cols, n)
    v = got[0] if path == "svc6" else got
    if path in ("base", "delta"):
        k = min(n, N_ORACLE)
        vc.cmp6(v[:k], _oracle(path, cols, "oracle_sizes")[:k], vc.head(cols, k))
    if n == 513:
        assert (s["info"]["case"][:n] >= 0).sum() > 200
        assert (v[:, 1]["action"] == 6).any(), "no ingress bypass in the batch"
        if path == "svc6":
            f = got[1]["flags"]
            noep = (f & gpc.LB_NO_ENDPOINT) != 0
            assert ((f & gpc.LB_HIT) != 0).sum() > 20 and ((f & gpc.LB_DNAT) != 0).any(), "no Service hit in the batch"
            assert noep.any() and (v[noep, 0]["table"] == gpc.VTABLE_ENDPOINT_DNAT).all(), "no NO_ENDPOINT reject in the batch"
        live = np.ones(n, bool) if path != "svc6" else (got[1]["flags"] & gpc.LB_NO_ENDPOINT) == 0
        none = (np.ascontiguousarray(v[:, 1]).view(np.uint8).reshape(n, 8) == 0).all(axis=1)
        assert (none & live).any(), "no ingress NONE half in the batch"


@pytest.mark.parametrize("present", ["none", "all", "defaults"] + list(vc.OPTIONAL))
@pytest.mark.parametrize("path", PATHS)
def test_column_presence(path, present):
    """The same packets without optional columns (2 code columns; 3 with Services), with all of them
    (4), with each alone (ct_src6 or ct_dst6 alone: 3) and with all of them holding the defaults
    (verdicts equal the run without columns). ct_src6 / ct_dst6 hold other addresses than src6 /
    dst6, and rules with ct peers read them (asserted: they decide verdicts of the batch).

    The placement of the third and fourth code column (classify.hip launch_classify6: "ct_src6 if
    present, then ct_dst6" at codes + nc * n) is device-only logic. By reading: the two columns
    swapped fails "all" (the ct cases of either side then read the other side's codes); ct_dst6
    always taken as the fourth column fails "ct_dst6" alone (its codes lie at 2 n, 3 n is never
    written) and, with Services, "none" (the synthesized ct_dst6); a grid of too few columns fails
    "ct_src6", "ct_dst6" and "all" (stale codes of the launch before); one too many reads a null
    column pointer."""
    s = _path(path)
    n = 257
    cols = _columns(s, present)
    got = _check(path, cols, n)
    v = got[0] if path == "svc6" else got
    if present == "defaults":
        _same(path, got, _emu(s["c"], s["cols"], n, lb=path == "svc6"), s["cols"])
    if present in ("ct_src6", "ct_dst6", "all"):
        plain = _emu(s["c"], s["cols"], n)
        assert (v != plain).any(axis=1).sum() >= 2, "the ct column decides no verdict"
    if path in ("base", "delta") and present in ("none", "ct_src6", "ct_dst6", "ct_state", "dest", "ct_mark"):
        vc.cmp6(v, _oracle(path, cols, "oracle_" + present), vc.head(cols, n))  # columns the oracle models


@pytest.mark.parametrize("with_len", [True, False], ids=["len", "nolen"])
@pytest.mark.parametrize("path", PATHS)
def test_counters_of_one_wave(path, with_len):
    """One 64-packet batch holding a packet counted in both stages, one counted in egress only and
    dropped there, one counted in ingress only, one taking the ingress bypass and one not counted,
    +new and -new: verdicts and per-rule {packets, bytes, sessions} equal the emulation's exactly."""
    s = _path(path)
    c, k = s["c"], s["w6"].counted
    if "batch" not in s:
        s["batch"] = vc.counter_batch(s["w6"], s["cols"])
    cols, rows = s["batch"]
    alone = {case: vc.counted_alone(c, cols, i) for case, i in rows.items()}  # what the batch holds, by the emulation
    one = lambda case, i: {conj: v[i] for conj, v in alone[case][0].items()}
    assert one("both", 0) == {k["egress"]: 1, k["ingress"]: 1} == one("both", 2)
    assert one("both_est", 0) == {k["egress"]: 1, k["ingress"]: 1} and one("both_est", 2) == {k["egress"]: 0, k["ingress"]: 0}
    assert one("egress_dropped", 0) == {k["drop"]: 1} and not alone["egress_dropped"][1][1].tobytes().strip(b"\0")
    assert alone["egress_dropped"][1][0]["action"] == 3
    assert one("ingress_only", 0) == {k["ingress"]: 1} == one("ingress_only_est", 0)
    assert alone["bypass"][0] == {} and alone["bypass"][1][1]["action"] == 6
    assert alone["uncounted"][0] == {} and alone["uncounted"][1][1]["action"] != 6
    if not with_len:
        cols = {name: a for name, a in cols.items() if name != "len"}
    _, slots = c.counters()
    arr = np.zeros((max(1, len(slots)), 3), np.uint64)
    c.reset_counters()
    _check(path, cols, 64, count=True, counters=arr)
    exp = {conj: tuple(int(x) for x in arr[i]) for i, conj in enumerate(slots) if conj and arr[i].any()}
    assert {k["egress"], k["drop"], k["ingress"]} <= set(exp) and (sum(v[1] for v in exp.values()) > 0) == with_len
    assert exp[k["ingress"]][0] >= 4 and exp[k["ingress"]][2] == exp[k["ingress"]][0] - 2
    assert {conj: tuple(v) for conj, v in c.network_policy_metrics().items() if any(v)} == exp


LAUNCHES = ((513, "all"), (1, "none"), (257, "ct_src6"), (64, "ct_dst6"))  # 4, 2, 3 and 3 code columns (+1 with Services)


@pytest.mark.parametrize("path", ["base", "svc6"])
def test_scratch_reuse_on_one_stream(path):
    """The per-stream scratch (code columns, Service columns, grouping scratch, each carved anew on
    every call) under a large batch followed by smaller ones with other column sets, queued on one
    non-default stream without a host synchronisation in between; then the same four launches as two
    interleaved pairs on two streams. Every result equals the emulation."""
    import torch
    s = _path(path)
    c, lb = s["c"], path == "svc6"
    jobs = [(n, _columns(s, present)) for n, present in LAUNCHES]
    want = [_emu(c, cols, n, lb=lb) for n, cols in jobs]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for order in ((0, 0, 0, 0), (0, 1, 0, 1)):
        dcols = [_upload(cols, n) for n, cols in jobs]
        bufs = [_buffers(n, lb) for n, _ in jobs]
        torch.cuda.synchronize()
        for (n, _), d, (out, lbo), k in zip(jobs, dcols, bufs, order):
            _launch(c, d, n, out, lbo, stream=streams[k].cuda_stream)
        torch.cuda.synchronize()
        for (n, cols), (out, lbo), w in zip(jobs, bufs, want):
            _same(path, _read(n, out, lbo), w, cols)


@pytest.mark.parametrize("path", ["base", "svc6"])
def test_alignment_is_checked(path):
    """Every IPv6 address column is read with one 128-bit load per packet and gpc_lb_result6 written
    with two 128-bit stores: a column or an LB buffer that is not 16-B aligned is refused (EINVAL)
    before anything is launched. A batch of no packets is accepted and writes nothing."""
    import torch
    s = _path(path)
    c, n = s["c"], 65
    cols = dict(s["cols"], ct_src6=s["opt"]["ct_src6"], ct_dst6=s["opt"]["ct_dst6"])
    dcols = _upload(cols, n)
    out, lbo = _buffers(n, True)
    torch.cuda.synchronize()

    def untouched():
        torch.cuda.synchronize()
        return bool((out == FILL).all()) and bool((lbo == FILL).all())

    for name in ("src6", "dst6", "ct_src6", "ct_dst6"):
        shifted = torch.zeros(16 * n + 16, dtype=torch.uint8, device=out.device)
        shifted[8:8 + 16 * n] = dcols[name].reshape(-1)
        soa = gpc.pkt_soa_device(dcols)
        setattr(soa, name, shifted.data_ptr() + 8)
        for call in (lambda: c.classify6_device(soa, n, out.data_ptr()),
                     lambda: c.classify6_lb_device(soa, n, out.data_ptr(), lbo.data_ptr())):
            with pytest.raises(gpc.GpcError) as e:
                call()
            assert e.value.code == gpc.GPC_EINVAL, name
        assert untouched(), name
    soa = gpc.pkt_soa_device(dcols)
    with pytest.raises(gpc.GpcError) as e:
        c.classify6_lb_device(soa, n, out.data_ptr(), lbo.data_ptr() + 8)
    assert e.value.code == gpc.GPC_EINVAL and untouched()
    c.classify6_device(soa, 0, out.data_ptr())
    c.classify6_lb_device(soa, 0, out.data_ptr(), lbo.data_ptr())
    assert untouched()
    _launch(c, dcols, n, out, lbo)  # the same buffers, aligned: the batch runs
    torch.cuda.synchronize()
    got = _read(n, out, lbo)
    want = _emu(c, cols, n, lb=True)
    _same_bytes(got[0], want[0], cols)
    assert got[1].tobytes() == want[1].tobytes()


VARIANTS = {"default": {}, "one_tag": {"GPC_V6_MAX_TAGS": "1"}, "leaf0": {"GPC_V6_LEAF_LENS": "0"}, "leaf8": {"GPC_V6_LEAF_LENS": "8"}}


@pytest.mark.parametrize("rules_of", ["c3", "native"])
def test_lpm_layout_variants(rules_of, monkeypatch):
    """The region-tag and sub-region layouts of the IPv6 LPM on the device: a rule set spread over
    four /48s with a region table per tag (default), with one tag allowed, with every block split
    down to /128 (no hash probe below the tables) and with blocks split only where a search would go
    global. "c3": 2 000 embedded rules; "native": small C3 with the native prefixes of
    tests/v6_cases.py under the same four /48s (prefixes ending inside, on and below the tables'
    levels; ct columns present; also compared with the oracle). Device == emulation per layout, the
    four give the same verdicts, and every variant's image differs from the default's (the knob acted)."""
    import ctypes as C
    n = 513
    if rules_of == "c3":
        wl = workload.config3(n_policies_per_dir=20, rules_per_policy=50)
        rules = workload.to_ipv6(wl, embed="multi48").rules
        cols = workload.packets_to_v6(workload.gen_packets(wl, n, seed=SEED), embed="multi48")
        del cols["len"]
    else:
        w6, _ = vc.native_workload(SEED, embed="multi48")
        rules = w6.rules
        cols, opt, _ = vc.native_packets(w6, SEED)
        cols = vc.head(dict(cols, ct_src6=opt["ct_src6"], ct_dst6=opt["ct_dst6"]), n)
    blobs, verdicts = {}, {}
    for name, env in VARIANTS.items():
        for k in ("GPC_V6_MAX_TAGS", "GPC_V6_LEAF_LENS"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        c = gpc.Classifier(ipv4=False, ipv6=True)
        c.initialize()
        c.batch_install_policy_rule_flows(rules)
        c.commit()
        blob, nw, _ = c.debug_image6()
        blobs[name] = np.ctypeslib.as_array(C.cast(blob, C.POINTER(C.c_uint32)), shape=(nw,)).tobytes()
        got = _device(c, cols, n)
        _same_bytes(got, emu.classify6(c, cols), cols)
        verdicts[name] = got
        c.close()
    for name in VARIANTS:
        assert verdicts[name].tobytes() == verdicts["default"].tobytes(), name
        assert name == "default" or blobs[name] != blobs["default"], name
    assert {1, 2, 3} <= set(np.unique(verdicts["default"]["action"]).tolist())
    if rules_of == "native":
        vc.cmp6(verdicts["default"][:N_ORACLE], vc.oracle6(rules, vc.head(cols, N_ORACLE), N_ORACLE), vc.head(cols, N_ORACLE))
