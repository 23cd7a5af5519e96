"""Shared by tests/test_combo.py (host emulation) and tests/test_gpu_combo.py (device): small IPv4 rule
sets that reach the host-set combination index (image.cpp build_composite, core.hpp kBandCombo) and
packets aimed at it.

  tiny   3 AddressGroups over the 40 hosts 10.0.0.1 .. 10.0.0.40: host i (i <= 35) lies in the groups
         whose bit is set in 1 + (i - 1) % 7, so the seven non-empty combinations all occur and
         hosts 36 .. 40 lie in no group. 12 rules per direction. The format's entry threshold is
         forced down (GPC_COMBO_MIN_ENTRIES=1, Case.env); everything else is as in production.
  dense  9 groups over the 4 096 hosts 10.0.0.1 .. 10.0.16.0: each of the first 4 032 hosts in each
         group with probability 1/2 (about 500 distinct combinations, ids above 255), the last 64 in
         none. 60 rules per direction. Passes the production threshold without an override.

Rules come from workload._acnp_config with a scripted peer and service function. In direction In a
rule's From is a group and its To the policy's ofports (source-axis combination band of
AntreaPolicyIngressRule), in direction Out its From is the policy's Pod IPs and its To a group
(destination-axis band of AntreaPolicyEgressRule). Rule i of a direction takes group i mod n and
service shape SHAPES[(i + 1) mod 5]:

  none   no service: a two-clause rule          multi  2-4 single ports: one exact entry per interval
  one    one port                               range  a port range
  many   six single ports: more intervals than an entry list takes, so the hull is verified from the
         record

and three rules per direction are special: `plus24` (a group plus a /24 ipBlock: the combination
does not decide its band clause), `only28` (only a /28 ipBlock: another band) and the `twins` (two
rules of one policy over the same group, no service, Allow above Drop).

packets() aims packets at every rule: members of several groups, of exactly one, pool addresses in
no group (combination id 0), member +- 1, addresses outside the pool, the two blocks' addresses and
edges; destination ports on, beside and between the rule's ports and range ends; other protocols;
ct_state / dest / ct_mark / len columns. It also aims packets at the rules and addresses of
delta_script(), the control-plane script both tiers replay over the committed base.

The reference is the C restatement of the OVS classifier over the oracle compiler's flows (Oracle),
every packet, counters on. conditions() states on the oracle's verdicts and the image's combination
ids that the batch depends on the format; it is a condition on the cases, not on the product."""
import contextlib
import copy
import gc
import ipaddress

import numpy as np

from antrea_amd import gpc, workload
from oracle import compiler as oc
from oracle import parity
from oracle.cls_c import CPipeline
from tests import emu
from tests.golden import make_churn_fixture as mcf

SHAPES = ("none", "one", "multi", "range", "many")
TABLE = {"In": "AntreaPolicyIngressRule", "Out": "AntreaPolicyEgressRule"}
POOL_BASE = int(ipaddress.ip_address("10.0.0.0"))
LOCAL_BASE = "10.1.0.0"
BLOCK24 = ipaddress.ip_network("10.9.1.0/24")
BLOCK28 = ipaddress.ip_network("10.9.2.16/28")
OUTSIDE = [int(ipaddress.ip_address(a)) for a in ("10.0.200.7", "10.2.0.9", "172.16.3.4", "10.0.0.0", "9.255.255.255")]
NO_MATCH, ALLOW, DROP = 1, 2, 3
# address categories of packets()
MULTI, SINGLE, FREE, NEIGHBOUR, OUT, B24, B28, MEMBER, DELTA = range(9)

_ip = workload._ip


class Case:
    """name, wl (workload.Workload), env (variables to set before a build), pool / groups / free
    (uint32 host values), and per flow id: direction, kind ("group", "plus24", "only28", "twin"),
    group index (None: only28) and service shape; delta[direction]: the rules and addresses of
    delta_script()."""

    def by_id(self):
        return {r["flow_id"]: r for r in self.wl.rules}

    def group_rules(self, direction):
        return [f for f, k in self.kind.items() if self.direction[f] == direction and k != "only28"]


def _service(shape, k):
    """(service list, protocol number, lowest port, highest port) of rule k's shape."""
    proto = "UDP" if k % 7 == 3 else "TCP"
    one = lambda p: {"protocol": proto, "port": int(p)}
    if shape == "none":
        return None, 6, 0, 0
    if shape == "one":
        ports = [1000 + 7 * k]
    elif shape == "multi":
        ports = [2000 + 10 * k + 3 * j for j in range(2 + k % 3)]
    elif shape == "many":
        ports = [4000 + 20 * k + 3 * j for j in range(6)]
    else:
        lo = 3000 + 20 * k
        return [dict(one(lo), end_port=lo + 5 + k % 9)], 17 if proto == "UDP" else 6, lo, lo + 5 + k % 9
    return [one(p) for p in ports], 17 if proto == "UDP" else 6, ports[0], ports[-1]


def _plan(name, i):
    """(kind, group, shape) of rule i of a direction."""
    n_groups, plus24, only28, twins, twin_group = (3, 5, 8, (9, 10), 0) if name == "tiny" else (9, 7, 13, (20, 21), 4)
    if i in twins:
        return "twin", twin_group, "none"
    if i == only28:
        return "only28", None, SHAPES[(i + 1) % 5]
    return ("plus24" if i == plus24 else "group"), i % n_groups, SHAPES[(i + 1) % 5]


def make(name):
    c = Case()
    c.name = name
    if name == "tiny":
        c.env = {"GPC_COMBO_MIN_ENTRIES": "1"}
        c.pool = (POOL_BASE + 1 + np.arange(40)).astype(np.uint32)
        member = np.array([[i < 35 and (1 + i % 7) >> g & 1 for i in range(40)] for g in range(3)], bool)
        n_pol, per_pol, n_local = 4, 3, 12
    else:
        c.env = {}
        c.pool = (POOL_BASE + 1 + np.arange(4096)).astype(np.uint32)
        member = np.random.default_rng(0xC0B0).random((9, 4096)) < 0.5
        member[:, -64:] = False
        n_pol, per_pol, n_local = 12, 5, 40
    c.groups = [c.pool[m] for m in member]
    c.n_in = member.sum(axis=0)  # groups holding each pool host
    c.free = c.pool[c.n_in == 0]
    n_dir = n_pol * per_pol
    calls = {"peer": 0, "svc": 0}
    plans = []

    def peers(rng):
        i = calls["peer"] % n_dir
        calls["peer"] += 1
        kind, g, shape = _plan(name, i)
        plans.append((kind, g, shape))
        if kind == "only28":
            return [{"ipnet": str(BLOCK28)}], (int(BLOCK28.network_address), 28)
        lst = [_ip(v) for v in c.groups[g]]
        if kind == "plus24":
            lst.append({"ipnet": str(BLOCK24)})
        return lst, (int(c.groups[g][0]), 32)

    def svc(rng):
        i = calls["svc"] % n_dir
        calls["svc"] += 1
        return _service(_plan(name, i)[2], i)

    c.wl = workload._acnp_config("combo-" + name, n_pol, per_pol, peers, svc, seed=0xC0B0 + len(name), n_local=n_local,
                                 local_base=LOCAL_BASE, actions=(0.55, 0.45, 0.0))
    c.direction, c.kind, c.group, c.shape = {}, {}, {}, {}
    for r, (kind, g, shape) in zip(c.wl.rules, plans):
        f = r["flow_id"]
        c.direction[f], c.kind[f], c.group[f], c.shape[f] = r["direction"], kind, g, shape
    c.delta = {}
    for d in ("In", "Out"):
        t = [f for f in c.group_rules(d) if c.kind[f] == "twin"]
        hi, lo = sorted(t, key=lambda f: -c.by_id()[f]["priority"])
        c.by_id()[hi]["action"], c.by_id()[lo]["action"] = "Allow", "Drop"
        plain = [f for f in c.group_rules(d) if c.kind[f] == "group"]
        ext = plain[0]  # the rule that takes the point extensions
        g = c.group[ext]
        same = [f for f in plain[1:] if c.group[f] == g]
        in_g = member[g]
        c.delta[d] = {"ext": ext, "shared": same[0], "cycled": plain[1], "twins": (hi, lo),
                      "with_id": int(c.pool[~in_g & (c.n_in >= 1)][0]), "free": int(c.free[0]), "outside": OUTSIDE[0],
                      "base_member": int(c.pool[in_g & (c.n_in >= 2)][0]), "new": max(c.by_id()) + (1 if d == "In" else 2)}
    return c


# ------------------------------------------------------------------------------------- packets
def _ports_of(r, rng, on):
    """A destination port for rule r: one of its ports (on), else beside / between them or anywhere."""
    svc = r.get("service")
    if not svc:
        return int(rng.integers(1, 65536))
    own, near = [], []
    for s in svc:
        lo, hi = s["port"], s.get("end_port", s["port"])
        own += [lo, hi, (lo + hi) // 2]
        near += [lo - 1, hi + 1]
    lows = sorted(s["port"] for s in svc)
    near += [(a + b) // 2 for a, b in zip(lows, lows[1:]) if b - a > 1]  # between two of its ports
    near.append(int(rng.integers(1, 65536)))
    return int(rng.choice(own if on else near))


def _proto_of(r):
    svc = r.get("service")
    return 17 if svc and svc[0]["protocol"] == "UDP" else 6


def _address(c, r, cat, rng):
    g = c.group[r["flow_id"]]
    if g is None and cat in (MULTI, SINGLE, MEMBER, NEIGHBOUR):
        cat = B28
    if cat in (MULTI, SINGLE, MEMBER, NEIGHBOUR):
        grp = c.groups[g]
        n_in = c.n_in[grp - c.pool[0]]
        pick = grp[n_in >= 2] if cat == MULTI else grp[n_in == 1] if cat == SINGLE else grp
        v = int(rng.choice(pick if len(pick) else grp))
        return v + int(rng.choice([-1, 1])) if cat == NEIGHBOUR else v
    if cat == FREE:
        return int(rng.choice(c.free))
    if cat == OUT:
        return int(rng.choice(OUTSIDE))
    net = BLOCK24 if cat == B24 else BLOCK28
    lo, hi = int(net.network_address), int(net.broadcast_address)
    return int(rng.choice([lo - 1, lo, hi, hi + 1, int(rng.integers(lo, hi + 1))]))


def _packet(c, r, addr, rng, on=True, own_proto=True, own_local=True):
    wl = c.wl
    proto = _proto_of(r) if own_proto else int(rng.choice([17, 1, 132, 6]))
    j = int(rng.integers(len(wl.local_ips)))
    p = {"sport": int(rng.integers(1024, 65536)), "dport": _ports_of(r, rng, on), "proto": proto}
    if proto == 1:
        p["sport"], p["dport"] = int(rng.choice([0, 3, 8, 11])), 0
    if r["direction"] == "In":
        port = int(rng.choice([t["ofport"] for t in r["to"]])) if own_local else int(wl.local_ports[j])
        p.update(src=addr, dst=int(wl.local_ips[port - 3]), out_port=port)
    else:
        src = int(ipaddress.ip_address(str(rng.choice(r["from"])))) if own_local else int(wl.local_ips[j])
        p.update(src=src, dst=addr, out_port=int(wl.local_ports[j]))
    return p


def packets(c, n=4200, seed=7):
    """(cols, info): n packets, both directions interleaved, the delta script's packets among the first
    third. info["aim"] / ["cat"]: the rule (flow id) and the address category each packet is aimed at."""
    rng = np.random.default_rng(seed)
    by_id = c.by_id()
    pkts, aim, cat = [], [], []

    def add(r, addr, k, **kw):
        pkts.append(_packet(c, r, addr, rng, **kw))
        aim.append(r["flow_id"])
        cat.append(k)

    for d in ("In", "Out"):
        z = c.delta[d]
        for _ in range(4):
            for key in ("with_id", "free", "outside", "base_member"):
                add(by_id[z["ext"]], z[key], DELTA)
            add(by_id[z["shared"]], z["base_member"], DELTA)
            add(by_id[z["shared"]], z["base_member"], DELTA, on=False)
            add(by_id[z["cycled"]], _address(c, by_id[z["cycled"]], MEMBER, rng), DELTA)
    n_script = len(pkts)
    cats = [MULTI, MEMBER, SINGLE, MEMBER, FREE, MULTI, NEIGHBOUR, MEMBER, OUT, MULTI, B24, MEMBER, B28, SINGLE]
    k = 0
    while len(pkts) < n:
        r = c.wl.rules[k % len(c.wl.rules)]
        kc = cats[(k // len(c.wl.rules) + k) % len(cats)]
        u = rng.random(3)
        add(r, _address(c, r, kc, rng), kc, on=u[0] < 0.6, own_proto=u[1] < 0.85, own_local=u[2] < 0.85)
        k += 1
    order = np.concatenate([rng.permutation(n_script), n_script + rng.permutation(n - n_script)])
    order[:n // 3] = order[:n // 3][rng.permutation(n // 3)]  # every larger head holds all of the script's packets
    cols = {k: np.array([pkts[i][k] for i in order], dtype=gpc.PKT_COLUMNS[k]) for k in
            ("src", "dst", "sport", "dport", "proto", "out_port")}
    u = rng.random(n)  # the optional columns of tests/test_gpu_fused_chain.py optional_columns
    cols["ct_state"] = np.where(u < 0.6, 0x21, np.where(u < 0.85, 0x20, 0x22)).astype(np.uint8)
    cols["dest"] = rng.choice([0, 0, 1, 2, 3], n).astype(np.uint8)
    cols["ct_mark"] = np.where(rng.random(n) < 0.25, 0x40, rng.choice([0, 0x10, 0x20], n)).astype(np.uint8)
    cols["len"] = rng.integers(1, 65536, n).astype(np.uint16)
    return cols, {"aim": np.array(aim)[order], "cat": np.array(cat)[order]}


def head(cols, n):
    return {k: np.ascontiguousarray(v[:n]) for k, v in cols.items()}


# ------------------------------------------------------------------------------------ references
@contextlib.contextmanager
def _gc_off():
    """The dense case's quarter of a million flows are millions of long-lived Python objects: the
    cycle collector's full passes while they are allocated cost a third of the time."""
    on = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if on:
            gc.enable()


class Oracle:
    """The oracle compiler over the case's rules; apply() replays control-plane ops, run() walks the
    current flows with the C classifier: (verdicts (n, 2), {conj: (packets, bytes, sessions)}).

    flows() is the compiler's dump_flows() kept up to date: the compiler's flow table (`installed`,
    written by its bundles alone) notes the identities set or removed, so only those flows are rendered
    and parsed again since the last dump (`lines`, `parsed`); check_dump() compares with a fresh
    dump_flows()."""

    class _Table(dict):
        def __init__(self, dirty):
            super().__init__()
            self.dirty = dirty

        def __setitem__(self, k, f):
            self.dirty.add(k)
            super().__setitem__(k, f)

        def __delitem__(self, k):
            self.dirty.add(k)
            super().__delitem__(k)

        def pop(self, k, *default):
            self.dirty.add(k)
            return super().pop(k, *default)

    def __init__(self, rules):
        self.parsed = {}  # flow line -> its C records
        self.lines = {}   # flow identity -> flow line
        self.dirty = set()
        self.fnp = oc.FeatureNetworkPolicy()
        assert not self.fnp.installed
        self.fnp.installed = self._Table(self.dirty)
        self.fnp.initialize()
        with _gc_off():
            self.fnp.batch_install_policy_rule_flows(copy.deepcopy(rules))
        self.tiers = {r["flow_id"]: int(r.get("tier_priority") or 0) for r in rules}

    def apply(self, ops):
        for o in ops:
            if o["op"] == "install":
                self.tiers[o["rule"]["flow_id"]] = int(o["rule"].get("tier_priority") or 0)
        apply(self.fnp, ops)

    def flows(self):
        installed = self.fnp.installed
        for k in self.dirty:
            if k in installed:
                self.lines[k] = oc.flow_to_string(installed[k])
            else:
                self.lines.pop(k, None)
        self.dirty.clear()
        return [self.lines[k] for k in installed]

    def check_dump(self):
        assert self.flows() == self.fnp.dump_flows()

    def run(self, cols):
        with _gc_off():
            cp = CPipeline(self.flows(), self.tiers, procs=1, cache=self.parsed)
        v = cp.classify(cols, threads=1, count=True)
        v = np.ascontiguousarray(v).view(gpc.VERDICT_DTYPE).reshape(-1, 2)
        return v, {k: tuple(m) for k, m in parity.oracle_metrics(cp).items() if any(m)}


def classifier(c, monkeypatch, env=None, commit=emu.commit_host, **kw):
    """A classifier over the case's rules, built and committed under the case's variables plus env
    (the image builder reads them at every build; they are restored afterwards)."""
    with monkeypatch.context() as m:
        for k, v in dict(c.env, **(env or {})).items():
            m.setenv(k, v)
        clf = gpc.Classifier(**kw)
        clf.initialize()
        clf.batch_install_policy_rule_flows(copy.deepcopy(c.wl.rules))
        commit(clf)
    return clf


_REF = {}
N_PKTS = 4200
N_HEAD = 4099  # the device tier's largest batch: the head of the packet set


def reference(name):
    """Per case, once per process: {"case", "cols", "info", "want", "metrics", "flows", "tiers"} -- the
    packets, the oracle's verdicts and per-rule metrics of all of them, the base's flow dump -- and
    "metrics_head", the metrics of the first N_HEAD packets alone."""
    if name not in _REF:
        c = make(name)
        cols, info = packets(c, N_PKTS)
        o = Oracle(c.wl.rules)
        want, metrics = o.run(cols)
        _REF[name] = {"case": c, "cols": cols, "info": info, "oracle": o, "want": want, "metrics": metrics,
                      "metrics_head": o.run(head(cols, N_HEAD))[1], "flows": o.flows(), "tiers": dict(o.tiers)}
        gc.freeze()  # the flows stay for the process: keep the collector's later passes off them
    return _REF[name]


def delta_reference(name):
    """Once per process: [(label, ops, verdicts, metrics)] -- the oracle compiler's replay of
    delta_script() over the case's rules, its flows walked after every step (all packets). The
    replay goes on in the reference's own compiler, which is used up by it."""
    ref = reference(name)
    if "delta" not in ref:
        o = ref.pop("oracle")
        out = []
        for label, ops in delta_script(ref["case"]):
            o.apply(ops)
            out.append((label, ops) + o.run(ref["cols"]))
        o.check_dump()
        ref["delta"] = out
        gc.freeze()
    return ref["delta"]


def emulate(clf, cols):
    """Emulated (verdicts, {conj: (packets, bytes, sessions)}) of clf's committed epoch."""
    _, slots = clf.counters()
    arr = np.zeros((max(1, len(slots)), 3), np.uint64)
    v = emu.classify(clf, cols, counters=arr)
    return v, {int(s): tuple(int(x) for x in arr[i]) for i, s in enumerate(slots) if s and arr[i].any()}


def same(got, want, cols, what=""):
    """Verdict pairs equal byte for byte; the first differing packet in the message."""
    bad = np.nonzero((got != want).reshape(len(got), -1).any(axis=1))[0]
    if len(bad):
        i = bad[0]
        raise AssertionError("%s: %d/%d mismatches; first: packet %d %s\n got  %s\n want %s" % (
            what, len(bad), len(got), i, {k: int(v[i]) for k, v in cols.items()}, got[i], want[i]))
    assert got.tobytes() == want.tobytes(), what


def bands(clf, direction):
    """Bands of the direction's composite sub-indexes (emu.BAND_COMBO: the combination band)."""
    return sorted(s["band"] for s in emu.composite_layout(clf)[TABLE[direction]])


def conditions(c, clf, cols, want):
    """Per direction, from the oracle's verdicts `want` and clf's combination ids: packets decided by
    a group rule, the largest combination id among them, the service shapes of the deciding rules;
    and the actions that occur."""
    out = {"actions": {int(a) for a in np.unique(want["action"])}}
    for d, stage, col in (("In", 1, "src"), ("Out", 0, "dst")):
        rules = set(c.group_rules(d))
        conj, act = want[:, stage]["conj_id"], want[:, stage]["action"]
        decided = np.array([int(x) in rules for x in conj]) & ((act == ALLOW) | (act == DROP))
        ids = emu.combo_ids(clf, TABLE[d], cols[col])
        out[d] = {"decided": int(decided.sum()), "max_id": int(ids[decided].max()) if decided.any() else 0,
                  "ids": {int(x) for x in ids}, "id0_in_pool": int(((ids == 0) & np.isin(cols[col], c.pool)).sum()),
                  "shapes": {c.shape[int(x)] for x in conj[decided]}}
    return out


# ----------------------------------------------------------------------------------- delta script
def apply(client, ops):
    """Replays ops through an openflow.Client NetworkPolicy surface (oracle compiler or product)."""
    for o in ops:
        if o["op"] == "swap":  # one ReassignFlowPriorities call that exchanges two priorities
            client.reassign_flow_priorities(dict(o["updates"]), o["table"])
        else:
            mcf.apply(client, [o])


def delta_script(c):
    """[(label, ops)]: the control-plane steps replayed over the committed base, each followed by a
    commit, on both directions at once (ops in tests/golden/make_churn_fixture.py's format):
    point extensions of a group rule by an address that has a combination id, one of the pool in
    no group and one outside the pool; the first deleted again; a base member deleted from one rule
    of a group that other rules share; a group rule uninstalled and reinstalled; the twins'
    priorities swapped; a new rule installed over an existing group."""
    by_id = c.by_id()
    side = {"In": "src", "Out": "dst"}
    op = lambda kind, d, f, a: {"op": kind, "fid": f, "side": side[d], "addrs": [_ip(a)], "priority": by_id[f]["priority"]}
    z = c.delta
    steps = [("add with_id", [op("add", d, z[d]["ext"], z[d]["with_id"]) for d in z]),
             ("add free", [op("add", d, z[d]["ext"], z[d]["free"]) for d in z]),
             ("add outside", [op("add", d, z[d]["ext"], z[d]["outside"]) for d in z]),
             ("del with_id", [op("del", d, z[d]["ext"], z[d]["with_id"]) for d in z]),
             ("del base_member", [op("del", d, z[d]["shared"], z[d]["base_member"]) for d in z]),
             ("uninstall", [{"op": "uninstall", "fid": z[d]["cycled"]} for d in z]),
             ("reinstall", [{"op": "install", "rule": copy.deepcopy(by_id[z[d]["cycled"]])} for d in z])]
    swap = []
    for d in z:
        p, q = (by_id[f]["priority"] for f in z[d]["twins"])
        swap.append({"op": "swap", "table": TABLE[d], "updates": {p: q, q: p}})
    steps.append(("swap twins", swap))
    new = []
    for d in z:
        r = copy.deepcopy(by_id[z[d]["ext"]])
        used = {x["priority"] for x in c.wl.rules if x["table"] == r["table"]}
        r.update(flow_id=z[d]["new"], name="rule-new", action="Drop" if r["action"] == "Allow" else "Allow",
                 priority=next(p for p in range(max(used) + 1, max(used) + 50) if p not in used))
        new.append({"op": "install", "rule": r})
    steps.append(("install new", new))
    return steps
