"""Shared by tests/test_trace6.py (CPU tier) and tests/test_gpu_trace6.py (device): the references of
gpc_trace6 over the native IPv6 batch of tests/v6_cases.py.

  * the oracle trace: ovs_cls.Pipeline.classify(pkt, trace=...) over the oracle compiler's flows, the
    packet with eth = 0x86DD and 128-bit integer addresses (as v6_cases.oracle6 builds it). On the
    Service path the packet is first rewritten by the product's Service stage run on the host
    (emu_svc6.lb_stage, itself pinned against the flow model in tests/test_service6.py); a packet of a
    Service without Endpoints is rejected before any table: no steps.
  * the flow-text LPM: every ipv6_src / ipv6_dst / ct_ipv6_src / ct_ipv6_dst network of the six rule
    tables in the oracle compiler's dump_flows(), and the longest one that contains an address
    (ipaddress arithmetic alone: no code, no tree).
  * the emulated trace6, composed from what exists: emu_svc6.lb_stage for the rewritten columns,
    emu.v6_codes ("one": the device's instantiation) for the codes, the emulated traced walk
    (tests/csrc/emu.cpp emu_trace) over debug_image6() / debug_epoch6() with the code columns."""
import copy
import ctypes as C
import ipaddress
import re

import numpy as np

from antrea_amd import gpc
from oracle import compiler as oc
from oracle import ovs_cls
from tests import emu, emu_svc6, v6_cases as vc
from tests.golden import make_churn_fixture as mcf

SEED = 3
RULE_TABLES = ("AntreaPolicyEgressRule", "EgressRule", "EgressDefaultRule", "AntreaPolicyIngressRule", "IngressRule",
               "IngressDefaultRule")
ADDR_COLUMNS = ("src6", "dst6", "ct_src6", "ct_dst6")
STEP_KEYS = ("table", "verdict", "flags", "conj_id", "priority")
REJECT_NO_ENDPOINT = ((gpc.ACT_NAMES.index("REJECT"), 0, gpc.VTABLE_ENDPOINT_DNAT, 0, 0), (0, 0, 0, 0, 0))
_TABLE = re.compile(r"\btable=(\w+)")
_NET = re.compile(r"\b(?:ct_)?ipv6_(?:src|dst)=([0-9a-fA-F:.]+(?:/\d+)?)")


# ------------------------------------------------------------------------------------ flow text
def flow_networks(flows):
    """The IPv6 networks the rule tables' flows match addresses against."""
    nets = set()
    for f in flows:
        t = _TABLE.search(f)
        if t and t.group(1) in RULE_TABLES:
            nets |= {ipaddress.IPv6Network(m) for m in _NET.findall(f)}
    return nets


class FlowLpm:
    """Longest-prefix match of an address (int) over a set of networks: the longest one holding it."""

    def __init__(self, nets):
        self.by_len = {}
        for n in nets:
            if n.prefixlen:
                self.by_len.setdefault(n.prefixlen, set()).add(int(n.network_address))
        self.lens = sorted(self.by_len, reverse=True)

    def __call__(self, addr):
        for plen in self.lens:
            net = addr & ~(vc.FULL >> plen) & vc.FULL
            if net in self.by_len[plen]:
                return ipaddress.IPv6Network((net, plen))
        return None


def addr_int(row):
    return int.from_bytes(bytes(row), "big")


# ------------------------------------------------------------------------------------ the oracle
class Oracle:
    """The oracle compiler's flows of a path's rule set: the pipeline of the final epoch, the networks
    of its flow text and (the delta path) of the base epoch's."""

    def __init__(self, path, w6):
        fnp = oc.FeatureNetworkPolicy(ipv4=path == "svc6", ipv6=True)
        fnp.initialize()
        fnp.batch_install_policy_rule_flows(copy.deepcopy(w6.rules))
        self.base_nets = flow_networks(fnp.dump_flows())
        mcf.apply(fnp, vc.log_of(path, w6))
        flows = fnp.dump_flows()
        self.nets = flow_networks(flows)
        self.lpm = FlowLpm(self.nets)
        self.pipe = ovs_cls.Pipeline(flows, {r["flow_id"]: int(r.get("tier_priority") or 0) for r in w6.rules})

    def trace(self, cols, i):
        """((egress, ingress) verdict tuples, [(table, verdict, flags, conj_id, priority)]) of packet i
        of the columns as the policy tables see them."""
        pkt = {k: int(v[i]) for k, v in cols.items() if v.ndim == 1}
        for k in ADDR_COLUMNS:
            if k in cols:
                pkt[k[:-1]] = addr_int(cols[k][i])
        pkt["eth"] = 0x86DD
        steps = []
        e, g = self.pipe.classify(pkt, trace=steps)
        return (e, g), steps


def policy_columns(c, cols):
    """(the columns as the policy stages see them, LB results (n,), no-Endpoint mask): the Service
    stage on the host where c has an IPv6 Service image, the columns themselves otherwise."""
    n = len(cols["proto"])
    if not c.debug_service_image6():
        return cols, np.zeros(n, gpc.LB6_DTYPE), np.zeros(n, bool)
    return emu_svc6.lb_stage(c, cols)


def oracle_traces(oracle, c, cols, n):
    """[(verdict pair, steps)] of the first n packets; a Service without Endpoints: REJECT, no steps."""
    rw, _, noep = policy_columns(c, vc.head(cols, n))
    return [(REJECT_NO_ENDPOINT, []) if noep[i] else oracle.trace(rw, i) for i in range(n)]


# ------------------------------------------------------------------------------------ the emulation
def emu_trace6(c, cols, n):
    """The emulated trace6 of the first n packets: [(verdicts (2,), steps, lb result, codes)]; codes =
    {column: code} of the address columns that take part (None: rejected before the policy tables)."""
    cols = vc.head(cols, n)
    rw, lb, noep = policy_columns(c, cols)
    present = [k for k in ADDR_COLUMNS if k in rw]
    codes = {k: emu.v6_codes(c, rw[k])[0] for k in present}
    blob, _, hdr = c.debug_image6()
    pool, _, jhdr = c.debug_epoch6()
    names = {"src6": "src", "dst6": "dst", "ct_src6": "ct_src", "ct_dst6": "ct_dst"}
    out = []
    for i in range(n):
        if noep[i]:
            v = np.zeros(2, gpc.VERDICT_DTYPE)
            v[0] = (0, gpc.ACT_NAMES.index("REJECT"), gpc.VTABLE_ENDPOINT_DNAT, 0, 0)
            out.append((v, [], lb[i], None))
            continue
        one = {k: a[i:i + 1] for k, a in rw.items() if a.ndim == 1}
        one.update({names[k]: codes[k][i:i + 1] for k in present})
        soa, keep, _ = gpc.pkt_soa_host(one)
        v = np.zeros(2, gpc.VERDICT_DTYPE)
        steps = (gpc.gpc_trace_step * 8)()
        ns = C.c_uint32()
        emu.load().emu_trace(blob, hdr, pool, jhdr, C.byref(soa), v.ctypes.data, steps, C.byref(ns))
        out.append((v, [{k: getattr(steps[j], k) for k in STEP_KEYS} for j in range(ns.value)], lb[i],
                    {k: int(codes[k][i]) for k in present}))
    return out


# ------------------------------------------------------------------------------------ comparisons
def same_trace(got_verdicts, got_steps, want, what):
    """The verdict pair and, step by step, (table, verdict, flags, conj_id, priority)."""
    (e, g), steps = want
    got = [tuple(s[k] for k in STEP_KEYS) for s in got_steps]
    assert got == steps, (what, got, steps)
    for j, v in enumerate((e, g)):
        assert tuple(got_verdicts[j][["action", "conj_id", "table", "tier", "flags"]].item()) == tuple(v), (what, got_verdicts, e, g)


def check_prefix(got, addr, oracle, exact, what):
    """The translated prefix `got` (IPv6Network or None) of an address (int) against the flow-text
    LPM. exact (a full build): equal, "no prefix" included. Otherwise (delta epochs: the tree may still
    hold the prefixes of deleted peers): it contains the address, is no shorter than the flow-text
    LPM, and is a prefix of the base epoch's flow text or of the final one's."""
    want = oracle.lpm(addr)
    if exact:
        assert got == want, (what, got, want)
        return
    if got is None:
        assert want is None, (what, got, want)
        return
    assert ipaddress.IPv6Address(addr) in got, (what, got)
    assert got.prefixlen >= (want.prefixlen if want is not None else 0), (what, got, want)
    assert got in oracle.nets or got in oracle.base_nets, (what, got)


def length_classes(oracle, addrs):
    """{prefix length of the flow-text LPM (0: none): addresses} over (n, 16) uint8 addresses."""
    out = {}
    for a in addrs:
        p = oracle.lpm(addr_int(a))
        out[p.prefixlen if p is not None else 0] = out.get(p.prefixlen if p is not None else 0, 0) + 1
    return out
