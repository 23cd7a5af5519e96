"""Shared by tests/test_v6_native.py (host emulation) and tests/test_gpu_v6_chain.py (device): IPv6
rule sets and packets whose addresses do NOT lie in one embedding.

Every other IPv6 test maps an IPv4 workload into fd00:10::/96 (or four /48s), so rules and packets
share their top 96 bits and the LPM (core.hpp v6_codes) only ever tells addresses apart by their
last word. native_workload() adds native prefixes to the rules of a small workload:

  * one random prefix of every length in LENGTHS (1 .. 128: below 32 bits, on and next to every
    32-bit word boundary, the /48 and /64 of real address plans);
  * a nested chain of the lengths CHAIN over one random 128-bit value, every member in another rule;
  * two /128s that differ in word 0 only and two that differ in word 3 only;
  * some of them once more as ct peers ("ctipnet": matched against ct_src6 / ct_dst6), so that the
    optional address columns decide verdicts;
  * three rules over two more native prefixes that make a packet counted in both stages, one
    counted and dropped in egress, and one counted in ingress only (counter_batch).

With embed="multi48" the same prefixes are drawn under the four /48s of that embedding instead, where
the LPM keeps region tables and sub-region tables (core.hpp V6Lpm).

native_packets() aims packets at every (rule, side, prefix): the prefix's first and last address,
a random address inside and the address just outside (the prefix's last bit flipped), the rest of
the packet satisfying the rule that carries the prefix (as tests/test_ipv6_delta.py _hit_packets
does). For the chain every member's rule also meets an address inside every other member. Workload
packets in the embedding are mixed in, and the whole batch is shuffled, so that any leading part of
it holds native packets.

The paths (make_classifier): "base"; "delta" -- the base commit, then w6.log: address adds bringing
three prefix lengths the base LPM does not search (NEW_LENGTHS: probed in the journal's overflow
table after the search) and one of a length it does, the delete of a chain member, an uninstall and
a reinstall of a rule carrying one, each committed, all as delta epochs; "grouped" (group_packets =
1); "svc6" -- C1 with IPv6 Services (tests/test_service6.py), the same native prefixes in its rules.

The reference is the Python oracle (oracle6: the oracle compiler's IPv6 flows walked by the OVS
classifier restatement, as tests/test_ipv6.py _oracle6 and tests/test_ipv6_delta.py _oracle_after,
with the ct address columns passed on as well). sensitivity() states on the oracle's verdicts alone
that the batch depends on the native prefixes: it is a condition on the cases, not on the product."""
import collections
import copy
import ipaddress
import random

import numpy as np

from antrea_amd import gpc, workload
from oracle import compiler as oc
from oracle import ovs_cls
from tests import emu_svc6
from tests.golden import make_churn_fixture as mcf

LENGTHS = (1, 7, 16, 31, 32, 33, 47, 48, 63, 64, 65, 95, 96, 97, 112, 127, 128)
CHAIN = (20, 31, 32, 33, 60, 64, 65, 90, 96, 97, 120, 128)
NEW_LENGTHS = (24, 50, 77)   # searched by no base LPM of these workloads (embedded lengths are >= 104)
CT_GROUPS = ("word0", "word3")   # prefixes that some rule also carries as a ct peer, besides CT_LENGTHS
CT_LENGTHS = (32, 64, 65, 96, 127)
PATHS = ("base", "delta", "grouped", "svc6")
OPTIONAL = ("ct_src6", "ct_dst6", "in_port", "svc_group", "tun_id", "ct_state", "dest", "ct_mark", "len")
N_BATCH = 640
FULL = (1 << 128) - 1
MISS_SRC = int(ipaddress.IPv6Address("2001:db8:ffff::1"))   # addresses that no rule holds on purpose
MISS_DST = int(ipaddress.IPv6Address("2001:db8:fffe::2"))
FIRST, LAST, INSIDE, OUTSIDE, CROSS = range(5)

# rule: flow id; side: "from" / "to"; prefix: ipaddress.IPv6Network; group: "len", "chain", "word0",
# "word3", "new" (added by the delta path's log); ct: a ct peer (matched against ct_src6 / ct_dst6)
Case = collections.namedtuple("Case", "rule side prefix group ct")


def _net(value, plen):
    return ipaddress.IPv6Network((value & ~(FULL >> plen) & FULL, plen))


def _peer(c):
    return {"ctipnet" if c.ct else "ipnet": str(c.prefix)}


def native_prefixes(rnd, embed="96"):
    """[(group, prefix)]: the random lengths, the chain, the word-0 and the word-3 pair. embed
    "multi48": every value lies under one of the embedding's four /48s, so the prefixes longer than
    /48 sit inside the LPM's region tables and their sub-region tables (core.hpp V6Lpm) and the
    shorter ones hold whole regions."""
    if embed == "multi48":
        value = lambda: workload.V6_MULTI48 | rnd.randrange(4) << 80 | rnd.getrandbits(80)
    else:
        value = lambda: rnd.getrandbits(128)
    out = [("len", _net(value(), plen)) for plen in LENGTHS]
    v = value()
    out += [("chain", _net(v, plen)) for plen in CHAIN]
    a, b = value(), value()
    out += [("word0", _net(a, 128)), ("word0", _net(a ^ 1 << 100, 128))]
    out += [("word3", _net(b, 128)), ("word3", _net(b ^ 1 << 5, 128))]
    return out


def _slots(rules):
    """(rule, side) of every peer list that holds addresses."""
    out = []
    for r in rules:
        if r["direction"] == "In" and r.get("from"):
            out.append((r, "from"))
        if r["direction"] == "Out":
            out += [(r, side) for side in ("to", "from") if r.get(side)]
    return out


def _counter_rules(w6, rnd):
    """Three AntreaClusterNetworkPolicy rules above every other one: egress Allow and ingress Allow of
    the same flows (src in n1, dst in n2, TCP 7001, to the first local Pod) and an egress Drop (TCP
    7002). Returns (rules, {"n1", "n2", "port", "egress", "drop", "ingress"})."""
    n1, n2 = _net(rnd.getrandbits(128), 64), _net(rnd.getrandbits(128), 56)
    port = int(w6.local_ports[0])
    fid = max(r["flow_id"] for r in w6.rules) + 1
    prio = max(int(r.get("priority") or 0) for r in w6.rules)
    prio = prio + 5 if prio else 54990

    def rule(k, direction, action, dport, to):
        return {"direction": direction, "table": "AntreaPolicy%sRule" % ("Egress" if direction == "Out" else "Ingress"),
                "action": action, "flow_id": fid + k, "policy_type": "AntreaClusterNetworkPolicy", "policy_namespace": "",
                "policy_name": "v6-chain-%d" % k, "policy_uid": "uid-v6-chain-%d" % k, "name": "rule-0",
                "tier_priority": 50, "priority": prio + (k == 1), "service": [{"protocol": "TCP", "port": dport}],
                "from": [{"ipnet": str(n1)}], "to": to}

    rules = [rule(0, "Out", "Allow", 7001, [{"ipnet": str(n2)}]), rule(1, "Out", "Drop", 7002, [{"ipnet": str(n2)}]),
             rule(2, "In", "Allow", 7001, [{"ofport": port}])]
    return rules, {"n1": n1, "n2": n2, "port": port, "egress": fid, "drop": fid + 1, "ingress": fid + 2}


def native_workload(seed, base=None, dual=False, embed="96"):
    """Small C3 in IPv6 (or `base`, a workload already in IPv6) with the native prefixes added to its
    rules. Returns (w6, cases); w6.cases are the same (rule, side, prefix, group, ct) tuples,
    w6.log / w6.new_cases the delta path's ops and the cases they add, w6.counted the counter rules."""
    if base is None:
        base = workload.to_ipv6(workload.config3(seed=seed, n_policies_per_dir=6, rules_per_policy=8), dual=dual, embed=embed)
    w6 = copy.copy(base)
    w6.rules = copy.deepcopy(base.rules)
    w6.embed = embed
    rnd = random.Random(seed)
    slots = _slots(w6.rules)
    rnd.shuffle(slots)
    take = iter(slots * 3)
    cases = []
    for group, prefix in native_prefixes(rnd, embed):
        r, side = next(take)
        cases.append(Case(r["flow_id"], side, prefix, group, False))
        if group in CT_GROUPS or (group == "len" and prefix.prefixlen in CT_LENGTHS):
            r, side = next(take)
            cases.append(Case(r["flow_id"], side, prefix, group, True))
    by_id = {r["flow_id"]: r for r in w6.rules}
    for c in cases:
        by_id[c.rule][c.side].append(_peer(c))
    # the delta path's ops, over the rules as they are now (a reinstall brings the native peers back)
    carrier = lambda plen: next(c for c in cases if c.group == "chain" and c.prefix.prefixlen == plen)
    busy = {carrier(60).rule, carrier(90).rule}
    free = [(r, side) for r, side in slots if r["flow_id"] not in busy][-4:]
    new = [Case(r["flow_id"], side, _net(rnd.getrandbits(128), plen), "new", False)
           for (r, side), plen in zip(free, NEW_LENGTHS + (64,))]
    op = lambda kind, c: {"op": kind, "fid": c.rule, "side": "src" if c.side == "from" else "dst", "addrs": [_peer(c)],
                          "priority": by_id[c.rule].get("priority")}
    log = [op("add", new[0]), {"op": "commit"}, op("add", new[1]), {"op": "commit"}, op("add", new[2]), op("add", new[3]),
           {"op": "commit"}, op("del", carrier(60)), {"op": "commit"}, {"op": "uninstall", "fid": carrier(90).rule},
           {"op": "commit"}, {"op": "install", "rule": copy.deepcopy(by_id[carrier(90).rule])}, {"op": "commit"}]
    extra, w6.counted = _counter_rules(w6, rnd)
    w6.rules += extra
    w6.cases, w6.new_cases, w6.log = cases, new, log
    return w6, cases


def _first_v6(peers):
    for p in peers:
        s = p if isinstance(p, str) else next(iter(p.values()))
        if isinstance(s, str) and ":" in s:
            return int(ipaddress.ip_network(s, strict=False).network_address)
    raise ValueError("no IPv6 peer")


def hit_packet(r, side, addr, ct=False):
    """One packet (dict of ints) that satisfies every clause of rule r, its `side` by `addr` (ct: by
    the ct address of that side, the plain address then misses)."""
    svc = (r.get("service") or [None])[0]
    p = {"sport": 40000, "dport": svc["port"] if svc else 80, "proto": {"TCP": 6, "UDP": 17, "SCTP": 132}[svc["protocol"]] if svc else 6,
         "ct_src6": None, "ct_dst6": None}
    if r["direction"] == "In":
        p.update(src6=_first_v6(r["from"]), dst6=int(ipaddress.IPv6Address("fd00:10::a00:5")), out_port=r["to"][0]["ofport"])
    else:
        p.update(src6=_first_v6(r["from"]), dst6=_first_v6(r["to"]), out_port=1)
    col = "src6" if side == "from" else "dst6"
    if ct:
        p[col] = MISS_SRC if side == "from" else MISS_DST
        col = "ct_" + col
    p[col] = addr
    return p


def _bytes16(values):
    return np.array([list(int(v).to_bytes(16, "big")) for v in values], np.uint8).reshape(-1, 16)


def native_packets(w6, seed, n=N_BATCH):
    """The native batch of w6: (cols, opt, info). cols: the six required columns; opt: every optional
    column (ct_src6 / ct_dst6: the ct cases' addresses, else native addresses of other packets);
    info["case"] / info["role"]: per packet the index into w6.cases + w6.new_cases (-1: an embedded
    workload packet) and FIRST / LAST / INSIDE / OUTSIDE / CROSS."""
    rnd = random.Random(seed + 1)
    by_id = {r["flow_id"]: r for r in w6.rules}
    cases = list(w6.cases) + list(w6.new_cases)
    pkts, case_of, role_of = [], [], []
    for k, c in enumerate(cases):
        lo = int(c.prefix.network_address)
        host = FULL >> c.prefix.prefixlen
        for role, a in ((FIRST, lo), (LAST, lo | host), (INSIDE, lo | (rnd.getrandbits(128) & host)),
                        (OUTSIDE, lo ^ (1 << (128 - c.prefix.prefixlen)) | (rnd.getrandbits(128) & host))):
            pkts.append(hit_packet(by_id[c.rule], c.side, a, c.ct))
            case_of.append(k)
            role_of.append(role)
    chain = [(k, c) for k, c in enumerate(cases) if c.group == "chain"]
    for k, c in chain:  # every chain member's rule meets an address inside every other member
        for _, o in chain:
            if o is not c:
                a = int(o.prefix.network_address) | (rnd.getrandbits(128) & (FULL >> o.prefix.prefixlen))
                pkts.append(hit_packet(by_id[c.rule], c.side, a))
                case_of.append(k)
                role_of.append(CROSS)
    m = n - len(pkts)
    assert m >= n // 4, "the batch leaves no room for embedded packets"
    emb = workload.gen_packets(w6, m, seed=seed)
    to_v6 = workload.service_packets_to_v6 if getattr(w6, "svc_meta", None) is not None else workload.packets_to_v6
    emb = to_v6(emb, w6.embed)
    natives = [p[k] for p in pkts for k in ("src6", "dst6", "ct_src6", "ct_dst6") if p[k] is not None and p[k] >> 96 != 0xfd000010]
    for p in pkts:  # the ct columns of the other packets: native addresses of the batch
        for k in ("ct_src6", "ct_dst6"):
            if p[k] is None:
                p[k] = rnd.choice(natives)
    order = np.random.default_rng(seed).permutation(n)
    scalar = lambda name, dt: np.concatenate([np.array([p[name] for p in pkts], dt), emb[name].astype(dt)])[order]
    cols = {"src6": np.concatenate([_bytes16(p["src6"] for p in pkts), emb["src6"]])[order],
            "dst6": np.concatenate([_bytes16(p["dst6"] for p in pkts), emb["dst6"]])[order],
            "sport": scalar("sport", np.uint16), "dport": scalar("dport", np.uint16), "proto": scalar("proto", np.uint8),
            "out_port": scalar("out_port", np.uint32)}
    cols = {k: np.ascontiguousarray(v) for k, v in cols.items()}
    rng = np.random.default_rng(seed + 2)
    ct_emb = _bytes16(rnd.choice(natives) for _ in range(2 * m)).reshape(2, m, 16)
    opt = {"ct_src6": np.ascontiguousarray(np.concatenate([_bytes16(p["ct_src6"] for p in pkts), ct_emb[0]])[order]),
           "ct_dst6": np.ascontiguousarray(np.concatenate([_bytes16(p["ct_dst6"] for p in pkts), ct_emb[1]])[order])}
    opt["in_port"] = cols["out_port"][rng.permutation(n)].astype(np.uint32)
    opt["svc_group"] = rng.integers(0, 4, n).astype(np.uint32)
    opt["tun_id"] = rng.integers(0, 3, n).astype(np.uint32)
    u = rng.random(n)  # +new+trk / +trk (-new: no session) / +est+trk
    opt["ct_state"] = np.where(u < 0.6, 0x21, np.where(u < 0.85, 0x20, 0x22)).astype(np.uint8)
    opt["dest"] = rng.choice([0, 0, 0, 1, 2, 3], n).astype(np.uint8)
    opt["ct_mark"] = np.where(rng.random(n) < 0.25, 0x40, rng.choice([0, 0x10, 0x20], n)).astype(np.uint8)
    opt["len"] = rng.integers(1, 65536, n).astype(np.uint16)
    info = {"case": np.concatenate([np.array(case_of), np.full(m, -1)])[order],
            "role": np.concatenate([np.array(role_of), np.full(m, -1)])[order], "cases": cases}
    return cols, opt, info


def default_columns(cols):
    """Every optional column present with the value its absence stands for (len: no verdict effect)."""
    n = len(cols["proto"])
    return {"ct_src6": cols["src6"].copy(), "ct_dst6": cols["dst6"].copy(), "in_port": np.zeros(n, np.uint32),
            "svc_group": np.zeros(n, np.uint32), "tun_id": np.zeros(n, np.uint32), "ct_state": np.full(n, 0x21, np.uint8),
            "dest": np.zeros(n, np.uint8), "ct_mark": np.zeros(n, np.uint8), "len": np.full(n, 100, np.uint16)}


def head(cols, n):
    return {k: np.ascontiguousarray(v[:n]) for k, v in cols.items()}


# ------------------------------------------------------------------------------------ references
def oracle6(rules, cols6, n, log=(), ipv4=False):
    """Python oracle verdicts (n, 2) of the IPv6 packets, after the oracle compiler replayed `log`."""
    fnp = oc.FeatureNetworkPolicy(ipv4=ipv4, ipv6=True)
    fnp.initialize()
    fnp.batch_install_policy_rule_flows(copy.deepcopy(rules))
    mcf.apply(fnp, log)
    pipe = ovs_cls.Pipeline(fnp.dump_flows(), {r["flow_id"]: int(r.get("tier_priority") or 0) for r in rules})
    out = np.zeros((n, 2), dtype=gpc.VERDICT_DTYPE)
    for i in range(n):
        pkt = {k: int(v[i]) for k, v in cols6.items() if v.ndim == 1}
        for k in ("src6", "dst6", "ct_src6", "ct_dst6"):
            if k in cols6:
                pkt[k[:-1]] = int.from_bytes(bytes(cols6[k][i]), "big")
        pkt["eth"] = 0x86DD
        e, g = pipe.classify(pkt)
        for j, v in enumerate((e, g)):
            out[i, j] = (v[1], v[0], v[2], v[3], v[4])
    return out


def cmp6(got, want, cols):
    """got == want, verdict pair by verdict pair; the first differing packet in the message."""
    bad = np.nonzero((got != want).reshape(len(got), -1).any(axis=1))[0]
    if len(bad):
        i = bad[0]
        pkt = {k: str(ipaddress.IPv6Address(bytes(v[i]))) if v.ndim == 2 else int(v[i]) for k, v in cols.items()}
        raise AssertionError("%d/%d mismatches; first: packet %d %s\n got  %s\n want %s" % (len(bad), len(got), i, pkt, got[i], want[i]))


def emulation(c, cols, n=None, counters=None, lb=None):
    """The host emulation of c's committed epoch (the Service stage included where it has one)."""
    return emu_svc6.classify6(c, cols if n is None else head(cols, n), counters=counters, lb=lb)


def sensitivity(want, info, ct=False):
    """From the oracle's verdict pairs alone: {(group, length): pairs} of (inside, just outside)
    packets of one case that get different verdict pairs, over the plain (ct: the ct) cases; and the
    deciding conjunctions of the chain's packets."""
    n = len(want)
    rows = collections.defaultdict(dict)
    for i in range(n):
        if info["case"][i] >= 0 and info["role"][i] in (INSIDE, OUTSIDE):
            rows[int(info["case"][i])][int(info["role"][i])] = i
    differ = collections.Counter()
    for k, r in rows.items():
        c = info["cases"][k]
        if c.ct == ct and len(r) == 2 and want[r[INSIDE]].tobytes() != want[r[OUTSIDE]].tobytes():
            differ[(c.group, c.prefix.prefixlen)] += 1
    chain = {info["cases"][k].rule for k in range(len(info["cases"])) if info["cases"][k].group == "chain"}
    decided = {int(x) for i in range(n) if info["case"][i] >= 0 and info["cases"][info["case"][i]].group == "chain"
               for x in want[i]["conj_id"] if int(x) in chain}
    return differ, decided


# ----------------------------------------------------------------------------------------- paths
def workload_of(path, seed=3):
    if path == "svc6":
        from tests.test_service6 import svc_workload6
        return native_workload(seed, base=svc_workload6("C1", 61)[1])[0]
    return native_workload(seed)[0]


def make_classifier(path, w6, commit, ipv4=False):
    """The path's classifier with its rule set committed through `commit` (the delta path: w6.log
    replayed on top, every commit of it a delta epoch)."""
    kw = {"group_packets": 1} if path == "grouped" else {"compact_after": -1} if path == "delta" else {}
    if path == "svc6":
        from tests.test_service6 import product6
        c = product6(w6, **kw)
    else:
        c = gpc.Classifier(ipv4=ipv4, ipv6=True, **kw)
        c.initialize()
        c.batch_install_policy_rule_flows(copy.deepcopy(w6.rules))
    commit(c)
    if path == "delta":
        s0 = c.image_stats()
        for o in w6.log:
            if o["op"] == "commit":
                commit(c)
            else:
                mcf.apply(c, [o])
        st = c.image_stats()
        assert st["v6_delta_builds"] > 0 and st["v6_overlay_rules"] > 0 and st["v6_full_builds"] == s0["v6_full_builds"], st
    return c


def log_of(path, w6):
    return w6.log if path == "delta" else ()


# -------------------------------------------------------------------------------------- counters
def counter_batch(w6, cols, seed=5):
    """A 64-packet batch (with ct_state, dest and len columns) over w6.counted's rules: a packet counted
    in both stages (+new and -new), one counted in egress only and dropped there, one counted in
    ingress only (+new and -new), one that takes the ingress bypass (dest = gateway) and one that no
    rule counts; the rest are the first packets of `cols`. Returns (cols, {case: row})."""
    k = w6.counted
    rng = np.random.default_rng(seed)
    src, dst = int(k["n1"].network_address) | 0x17, int(k["n2"].network_address) | 0x29
    quiet = [int(p) for p in w6.local_ports if not any(
        t.get("ofport") == int(p) for r in w6.rules if r["direction"] == "In" for t in r.get("to") or [])]
    spare = quiet[0] if quiet else int(w6.local_ports[-1])
    #           src6      dst6      dport out_port   ct_state dest
    special = {"both": (src, dst, 7001, k["port"], 0x21, 0), "both_est": (src, dst, 7001, k["port"], 0x20, 0),
               "egress_dropped": (src, dst, 7002, k["port"], 0x21, 0), "ingress_only": (src, MISS_DST, 7001, k["port"], 0x21, 0),
               "ingress_only_est": (src, MISS_DST, 7001, k["port"], 0x20, 0), "bypass": (MISS_SRC, MISS_DST, 9, spare, 0x21, 1),
               "uncounted": (MISS_SRC, MISS_DST, 9, spare, 0x21, 0)}
    rows = {case: int(r) for case, r in zip(special, rng.choice(64, len(special), replace=False))}
    out = {name: a[:64].copy() for name, a in cols.items()}
    out["ct_state"] = np.where(rng.random(64) < 0.7, 0x21, 0x20).astype(np.uint8)
    out["dest"] = np.zeros(64, np.uint8)
    out["len"] = rng.integers(1, 1500, 64).astype(np.uint16)
    for case, (s, d, dport, port, state, dest) in special.items():
        i = rows[case]
        out["src6"][i], out["dst6"][i] = _bytes16([s])[0], _bytes16([d])[0]
        out["sport"][i], out["dport"][i], out["proto"][i], out["out_port"][i] = 40000, dport, 6, port
        out["ct_state"][i], out["dest"][i] = state, dest
    return out, rows


def counted_alone(c, batch, i):
    """{conj: (packets, bytes, sessions)} of packet i of the batch alone, and its verdict pair (emulation)."""
    _, slots = c.counters()
    arr = np.zeros((max(1, len(slots)), 3), np.uint64)
    v = emulation(c, {name: np.ascontiguousarray(a[i:i + 1]) for name, a in batch.items()}, counters=arr)
    return {int(conj): tuple(int(x) for x in arr[s]) for s, conj in enumerate(slots) if conj and arr[s].any()}, v[0]
