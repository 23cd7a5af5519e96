"""Shared by tests/test_affinity6.py (host emulation) and tests/test_gpu_affinity6.py (device): the
IPv6 session-affinity workload (tests/affinity_cases.py carried to IPv6), its batches, the model over
the realized text (tests/affinity6_model.py), the scripted time / Endpoint-change / reinstall
sequence and the key sets that put a 256-slot table under hash pressure. A side under test is a
`runner(step name, IPv6 columns, clock) -> (verdicts, lb results, reachable live entries, stats, live
entries in all)`; live entries are (client, id word or destination, Endpoint address, Endpoint port |
REMOTE << 16, expires) with addresses as ints."""
import collections
import copy
import ipaddress

import numpy as np

from antrea_amd import gpc, workload
from oracle import compiler as oc
from tests import affinity6_model, affinity_cases as ac, emu_aff6, emu_svc6
from tests.test_emu_parity import _cmp

T, T0, LOG2 = ac.T, ac.T0, ac.LOG2
SVC_TABLES = ("table=ServiceLB", "table=EndpointDNAT", "table=NodePortMark")
FLAGS = gpc.LB_AFFINITY | gpc.LB_LEARNED
VIRT4 = int(ipaddress.ip_address(workload.VIRTUAL_NODE_PORT_DNAT))


def ip6(a):
    return int(ipaddress.IPv6Address(a))


def b16(a):
    return np.frombuffer(int(a).to_bytes(16, "big"), np.uint8)


def make_workload(seed):
    """tests/affinity_cases.py make_workload (C1 + 60 Services: 40 % affinity, 30 % NodePort) and its
    IPv6 image under the /96 embedding: (IPv4 workload, IPv6 workload)."""
    wl = ac.make_workload(seed)
    return wl, workload.services_to_ipv6(wl)


def make_product(w6, log2=LOG2, **kw):
    c = gpc.Classifier(ipv4=True, ipv6=True, session_affinity6=log2, **kw)
    c.initialize()
    c.batch_install_policy_rule_flows(copy.deepcopy(w6.rules))
    workload.install_services(c, w6)
    return c


def make_batch(wl, n, seed, clients=16, established=0.0, embedded_only=False):
    """tests/affinity_cases.py make_batch of the IPv4 workload and the same packets in IPv6:
    (IPv4 columns, IPv6 columns). embedded_only: packets to the virtual NodePort DNAT IP (whose IPv6
    counterpart is not its /96 embedding) go to the first NodePort address instead, in both."""
    cols = ac.make_batch(wl, n, seed, clients, established)
    if embedded_only:
        cols["dst"] = np.where(cols["dst"] == VIRT4, int(ipaddress.ip_address(workload.NODE_PORT_ADDRESSES[0])),
                               cols["dst"]).astype(np.uint32)
    return cols, workload.service_packets_to_v6(cols)


class Model:
    """The model over the product's realized IPv6 Service text and the oracle compiler's NP flows."""

    def __init__(self, rules, pods, clf):
        self.rules, self.pods = copy.deepcopy(rules), pods
        self.pipe = None
        self.refresh(clf)

    def refresh(self, clf, reinstalled=()):
        fnp = oc.FeatureNetworkPolicy(ipv4=True, ipv6=True)
        fnp.initialize()
        fnp.batch_install_policy_rule_flows(copy.deepcopy(self.rules))
        svc_flows = [f for f in clf.dump_flows() if any(t in f for t in SVC_TABLES)]
        tiers = {r["flow_id"]: int(r.get("tier_priority") or 0) for r in self.rules}
        args = (fnp.dump_flows() + svc_flows, tiers, clf.dump_groups(), self.pods)
        if self.pipe is None:
            self.pipe = affinity6_model.Affinity6Pipeline(*args)
        else:
            self.pipe.set_flows(*args, reinstalled=reinstalled)

    def run(self, cols6, now):
        return affinity6_model.run(self.pipe, cols6, now)


def entry_sets(got_live, model_live):
    """Both sides' live entries without their second field (the model keys by destination address, the
    table by install and address ids)."""
    strip = lambda es: sorted((e[0],) + tuple(e[2:]) for e in es)
    return strip(got_live), strip(model_live)


def check_step(name, cols4, got, want, pipe, got_live, got_stats, n_live_all, dst_known=False):
    """Verdicts, LB results (the two affinity flag bits included), live entries, counters: exact."""
    v, lb = got
    wv, wlb = want
    _cmp(v, wv, cols4)
    bad = np.nonzero(lb != wlb)[0]
    assert len(bad) == 0, (name, bad[:5], lb[bad[:3]], wlb[bad[:3]])
    a, b = entry_sets(got_live, pipe.live())
    assert a == b, name
    if dst_known:  # gpc_debug_affinity_table6 names the destination: the learned flows' NXM_NX_IPV6_DST too
        assert sorted(got_live) == sorted(pipe.live()), name
    assert got_stats["overflow"] == pipe.n_overflow, (name, got_stats, pipe.n_overflow)
    assert (got_stats["learned"], got_stats["hits"]) == (pipe.n_learned, pipe.n_hits), (name, got_stats)
    assert got_stats["live"] == n_live_all >= len(pipe.live()), (name, got_stats, n_live_all)


def scripted_sequence(wl, w6, clf, commit, runner, n=500, seed=7, established=0.0, dst_known=False):
    """tests/affinity_cases.py scripted_sequence in IPv6: a batch at t; the same at t + 1 (all hits); at
    t + T - 1; at t + T (all re-learn); after removing one Endpoint of an affinity Service and
    committing; after reinstalling one Service; after a NetworkPolicy-only commit."""
    commit()
    model = Model(w6.rules, w6.pods, clf)
    cols4, cols = make_batch(wl, n, seed, established=established)
    learned = {}

    def step(name, now):
        want = model.run(cols, now)
        v, lb, live, stats, n_all = runner(name, cols, now)
        check_step(name, cols4, (v, lb), want, model.pipe, live, stats, n_all, dst_known)
        learned[name] = lb[(lb["flags"] & gpc.LB_LEARNED) != 0]
        return lb

    lb0 = step("t", T0)
    n_keys = len(learned["t"])
    assert n_keys > 20 and ((lb0["flags"] & gpc.LB_AFFINITY) != 0).sum() > n_keys, "keys must repeat inside the batch"
    assert (lb0["flags"] & gpc.LB_NO_ENDPOINT).any() and ((lb0["flags"] & (gpc.LB_HIT | gpc.LB_AFFINITY)) == gpc.LB_HIT).any()
    lb1 = step("t+1", T0 + 1)
    assert len(learned["t+1"]) == 0
    if established == 0.0:
        aff = (lb0["flags"] & gpc.LB_AFFINITY) != 0
        assert ((lb1["flags"][aff] & gpc.LB_AFFINITY) != 0).all()
    step("t+T-1", T0 + T - 1)
    assert len(learned["t+T-1"]) == 0
    step("t+T", T0 + T)
    assert len(learned["t+T"]) == n_keys  # hard timeout: the hits did not refresh anything
    # --- one Endpoint of an affinity Service leaves its group
    bound = learned["t+T"]
    groups = {int(g): cnt for g, cnt in zip(*np.unique(bound["group_id"], return_counts=True))}
    gid = next(g for g in sorted(groups, key=lambda g: -groups[g]) if len(w6.groups[g]) >= 2)
    gone = w6.groups[gid][0]
    w6.groups[gid] = w6.groups[gid][1:]
    clf.install_service_group(gid, w6.groups[gid], True)
    commit()
    model.refresh(clf)
    n_bound = int(((bound["group_id"] == gid) & (bound["endpoint_ip"] == b16(ip6(gone["ip"]))).all(axis=1) &
                   (bound["endpoint_port"] == gone["port"])).sum())
    assert n_bound > 0
    step("endpoint removed", T0 + T + 1)
    rl = learned["endpoint removed"]
    assert len(rl) == n_bound and (rl["group_id"] == gid).all(), (len(rl), n_bound)
    # --- one affinity Service installed again: a new install id, its learned flows are orphaned
    tpg = lambda s: s["local_group_id"] if s["traffic_policy_local"] else s["cluster_group_id"]
    cfg = next(s for s in w6.services if s.get("affinity_timeout") and not s.get("is_nodeport") and tpg(s) in groups and
               tpg(s) != gid)
    clf.install_service_flows(cfg)
    commit()
    model.refresh(clf, reinstalled=[(dict(workload.SVC_PROTOS)[cfg["protocol"]], ip6(cfg["ip"]), cfg["port"])])
    step("reinstalled", T0 + T + 2)
    rl = learned["reinstalled"]
    assert len(rl) == groups[tpg(cfg)] and (rl["group_id"] == tpg(cfg)).all(), (len(rl), groups[tpg(cfg)])
    # --- a NetworkPolicy-only commit: the table is not an epoch's
    extra = dict(copy.deepcopy(w6.rules[0]), flow_id=max(r["flow_id"] for r in w6.rules) + 1)
    clf.install_policy_rule_flows(copy.deepcopy(extra))
    model.rules.append(extra)
    commit()
    model.refresh(clf)
    step("np commit", T0 + T + 3)
    assert len(learned["np commit"]) == 0
    return model


# ------------------------------------------------------------------ the table under hash pressure
# A table of 2^8 slots and keys chosen, with the product's own digest and hash (emu_aff6.candidates),
# to share buckets. The exact key sets satisfy tests/affinity_cases.py no_overflow (every key has more
# candidate slots than neighbours), so device, emulation, stale-find emulation and the model (which has
# no capacity) agree exactly whatever the arrival order.
P_LOG2 = 8
P_TIMEOUTS = (40, 200)                                  # Service A, Service B
P_NETS = (ip6("2001:db8:a::"), ip6("2001:db8:b::"))    # the clients of A / of B are searched from here on
P_SVC = ("fd00:10:96::100", "fd00:10:96::101")
P_PER_KEY = 48
Key = collections.namedtuple("Key", "svc src c d")  # Service (0: A, 1: B), client address, candidate slots, digest


def make_pressure_product(bits=None, **kw):
    """C1's rules in IPv6 + the affinity ClusterIP Services A (timeout 40) and B (timeout 200) of 8
    remote Endpoints each over a table of 256 slots: (IPv4 C1 workload for packet generation, IPv6
    rules, product -- not committed yet, [(config, Endpoints)]). One egress rule more applies to the
    two client networks and allows A's Endpoints and all but the last of B's."""
    wl = workload.config1(seed=81)
    w6 = workload.to_ipv6(wl)
    egress = next(r for r in w6.rules if r["direction"] == "Out" and not r.get("service"))
    rules = copy.deepcopy(w6.rules) + [dict(copy.deepcopy(egress), flow_id=max(r["flow_id"] for r in w6.rules) + 1,
                                            **{"from": [{"ipnet": "2001:db8:a::/47"}],
                                               "to": [{"ipnet": "fd00:10:128:1::/64"}, {"ipnet": "fd00:10:128:2::/125"}]})]
    c = gpc.Classifier(ipv4=True, ipv6=True, session_affinity6=P_LOG2, **kw)
    c.initialize()
    c.batch_install_policy_rule_flows(copy.deepcopy(rules))
    svcs = []
    for s, timeout in enumerate(P_TIMEOUTS):
        eps = [{"ip": "fd00:10:128:%d::%x" % (s + 1, k), "port": 8000 + k, "is_local": False, "node_name": "n%d" % k}
               for k in range(8)]
        cfg = {"ip": P_SVC[s], "port": 80, "protocol": "TCP", "cluster_group_id": 100 + 2 * s, "local_group_id": 101 + 2 * s,
               "affinity_timeout": timeout}
        c.install_service_group(cfg["cluster_group_id"], eps, True)
        c.install_endpoint_flows("TCP", eps, 6)
        c.install_service_flows(cfg)
        svcs.append((cfg, eps))
    if bits is not None:
        c.debug_set_affinity6_digest_bits(bits)
    return wl, rules, c, svcs


class KeySet:
    """Clusters of colliding keys of the committed Services A and B, found by a search over 2^15
    client addresses per Service (bits: the digest width of the table).
      shared     a1, a2, b1, b2 with one common first bucket; the second buckets pairwise distinct
      degenerate a key of A whose two buckets coincide, and a key of B whose first bucket that is
      identical  a1, a2, b1 .. b4 with the same bucket pair: six keys for four slots (overflows on
                 purpose; never part of exact_keys())
      background 24 keys away from all of them, no two sharing a bucket"""
    N = 1 << 15

    def __init__(self, clf, bits=64):
        by_group = {gid: inst for inst, gid, _ in emu_aff6.affinity_services(clf)}
        self.install = [by_group[100], by_group[102]]
        self.bits = bits
        self.addr, self.dig, self.cand = [], [], []
        for inst, net in zip(self.install, P_NETS):
            a = np.zeros((self.N, 16), np.uint8)
            a[:] = b16(net)
            a[:, 12:] = np.arange(self.N, dtype=">u4").view(np.uint8).reshape(-1, 4)
            d, c = emu_aff6.candidates(inst, a, P_LOG2, bits=bits)
            self.addr.append(a), self.dig.append(d), self.cand.append(c)
        self.b1 = [(c[:, 0] >> 1).astype(np.int64) for c in self.cand]
        self.b2 = [(c[:, 2] >> 1).astype(np.int64) for c in self.cand]
        assert all((c[:, 1] == c[:, 0] + 1).all() and (c[:, 3] == c[:, 2] + 1).all() and (c < (1 << P_LOG2)).all() for c in self.cand)
        if bits != 64:
            return
        self.used = set()
        self.identical = self._identical()
        self.shared = self._shared()
        self.degenerate = self._degenerate()
        self.background = self._background(24)
        ac.check_no_overflow(self.exact_keys())
        assert not ac.no_overflow(self.identical)
        digs = [k.d for k in self.exact_keys() + self.identical]
        assert len(set(digs)) == len(digs), "the pressure cases are about buckets, not digests"

    def key(self, svc, i):
        return Key(svc, P_NETS[svc] + int(i), tuple(int(x) for x in self.cand[svc][i]), int(self.dig[svc][i]))

    def _take(self, keys):
        self.used |= {s >> 1 for k in keys for s in k.c}
        return keys

    def _free(self, b):
        return ~np.isin(b, sorted(self.used))

    def _identical(self):
        pair = [self.b1[s] * 128 + self.b2[s] for s in (0, 1)]
        cnt = [np.bincount(p[self.b1[s] != self.b2[s]], minlength=128 * 128) for s, p in enumerate(pair)]
        p = np.nonzero((cnt[0] >= 2) & (cnt[1] >= 4))[0][0]
        keys = [self.key(0, i) for i in np.nonzero(pair[0] == p)[0][:2]] + [self.key(1, i) for i in np.nonzero(pair[1] == p)[0][:4]]
        assert len({k.c for k in keys}) == 1 and len(set(keys[0].c)) == 4
        return self._take(keys)

    def _shared(self):
        x = min(set(range(128)) - self.used)
        keys, seconds = [], {x}
        for s in (0, 1):
            got = 0
            for i in np.nonzero((self.b1[s] == x) & self._free(self.b2[s]))[0]:
                if got < 2 and int(self.b2[s][i]) not in seconds:
                    seconds.add(int(self.b2[s][i]))
                    keys.append(self.key(s, i))
                    got += 1
            assert got == 2
        self.used.add(x)
        return self._take(keys)

    def _degenerate(self):
        for i in np.nonzero((self.b1[0] == self.b2[0]) & self._free(self.b1[0]))[0]:
            d = self.b1[0][i]
            j = np.nonzero((self.b1[1] == d) & (self.b2[1] != d) & self._free(self.b2[1]))[0]
            if len(j):
                keys = [self.key(0, i), self.key(1, j[0])]
                assert len(set(keys[0].c)) == 2 and keys[1].c[0] == keys[0].c[0]
                return self._take(keys)
        raise AssertionError("no degenerate key with a neighbour")

    def _background(self, n):
        keys = []
        for i in np.nonzero(self.b1[0] != self.b2[0])[0]:
            p, q = int(self.b1[0][i]), int(self.b2[0][i])
            if p in self.used or q in self.used:
                continue
            keys += self._take([self.key(0, i)])
            if len(keys) >= n:
                return keys
        raise AssertionError("only %d background keys" % len(keys))

    def exact_keys(self):
        return self.shared + self.degenerate + self.background

    def spread(self, svc, n):
        """n keys of one Service with 2 n distinct buckets among them (an own key set)."""
        keys, used = [], set()
        for i in np.nonzero(self.b1[svc] != self.b2[svc])[0]:
            p, q = int(self.b1[svc][i]), int(self.b2[svc][i])
            if p not in used and q not in used:
                used |= {p, q}
                keys.append(self.key(svc, i))
                if len(keys) == n:
                    ac.check_no_overflow(keys)
                    assert len({k.d for k in keys}) == n
                    return keys
        raise AssertionError("only %d spread keys" % len(keys))

    def same_digest(self, svc, n=2):
        """n clients of one Service whose (narrowed) digests are equal."""
        vals, cnt = np.unique(self.dig[svc], return_counts=True)
        d = vals[np.nonzero(cnt >= n)[0][0]]
        return [self.key(svc, i) for i in np.nonzero(self.dig[svc] == d)[0][:n]]


def slot_of(tab_words, k):
    """The slots of a host copy of the table (emu_aff6.Table6.tab) claimed with k's digest."""
    t = tab_words.reshape(-1, emu_aff6.SLOT_WORDS)
    words = t[:, 0].astype(np.uint64) | (t[:, 1].astype(np.uint64) << np.uint64(32))
    return [int(s) for s in np.nonzero(words == np.uint64(k.d))[0]]


def key_batch(wl, svcs, keys, seed, order=0, per_key=P_PER_KEY, established=0.3):
    """per_key packets of every key to its Service, random source ports, `established` of them +est,
    the whole batch shuffled; `order` picks the shuffle of the same packets. (IPv4 columns of the
    generator -- for messages only -- and the IPv6 batch.)"""
    n = len(keys) * per_key
    assert n <= 8192
    rng = np.random.default_rng(seed)
    cols4 = workload.gen_packets(wl, n, seed=seed)
    cols = workload.packets_to_v6(cols4)
    k = np.repeat(np.arange(len(keys)), per_key)
    cols["src6"] = np.array([b16(key.src) for key in keys], np.uint8)[k]
    cols["dst6"] = np.array([b16(ip6(svcs[key.svc][0]["ip"])) for key in keys], np.uint8)[k]
    cols["dport"] = np.full(n, 80, np.uint16)
    cols["proto"] = np.full(n, 6, np.uint8)
    cols["sport"] = rng.integers(1024, 65536, size=n).astype(np.uint16)
    cols["ct_state"] = np.where(rng.random(n) < established, ac.gpc_ct("est"), ac.gpc_ct("new")).astype(np.uint8)
    perm = np.random.default_rng([seed, order]).permutation(n)
    return ({name: np.ascontiguousarray(v[perm]) for name, v in cols4.items()},
            {name: np.ascontiguousarray(v[perm]) for name, v in cols.items()})


def key_index(cols, svcs, keys):
    """{key: caller indexes of its packets, ascending}."""
    out = {}
    for key in keys:
        m = (cols["src6"] == b16(key.src)).all(axis=1) & (cols["dst6"] == b16(ip6(svcs[key.svc][0]["ip"]))).all(axis=1)
        out[key] = np.nonzero(m)[0]
        assert len(out[key])
    assert sum(len(v) for v in out.values()) == len(cols["dport"])
    return out


def own_choices(clf, cols, verdicts=False):
    """Every packet's own hash choice (the plain Service stage), (n,) LB6_DTYPE."""
    own = np.zeros(len(cols["dport"]), gpc.LB6_DTYPE)
    v = emu_svc6.classify6(clf, cols, lb=own)
    return (v, own) if verdicts else own


def first_new(cols, idx):
    new = (cols["ct_state"][idx] & 1) != 0
    assert new.any()
    return int(idx[new][0])


def ep_of(lb, i):
    return (bytes(lb["endpoint_ip"][i]), int(lb["endpoint_port"][i]))


def learned_endpoints(cols, lb, index):
    """{key: Endpoint of its one GPC_LB_LEARNED packet}, which must be the key's first +new packet."""
    out = {}
    for key, idx in index.items():
        l = idx[(lb["flags"][idx] & gpc.LB_LEARNED) != 0]
        assert list(l) == [first_new(cols, idx)], key
        out[key] = ep_of(lb, l[0])
    return out


def check_all_hits(lb, index, bound):
    for key, idx in index.items():
        assert ((lb["flags"][idx] & FLAGS) == gpc.LB_AFFINITY).all(), key
        assert all(ep_of(lb, i) == bound[key] for i in idx), key


class Steps:
    """One side under test (a runner) stepped beside the model."""

    def __init__(self, rules, clf, runner, dst_known=False):
        self.model = Model(rules, {}, clf)
        self.runner, self.dst_known = runner, dst_known

    def __call__(self, name, batch, now):
        cols4, cols = batch
        want = self.model.run(cols, now)
        v, lb, live, stats, n_all = self.runner(name, cols, now)
        check_step(name, cols4, (v, lb), want, self.model.pipe, live, stats, n_all, self.dst_known)
        assert len({(e[0], e[1]) for e in live}) == len(live) == n_all, name  # one entry per key
        return lb, stats, live


def case_collisions(wl, rules, clf, svcs, ks, runner, order, tab=None, dst_known=False):
    """Collisions in one batch: the shared and degenerate clusters and the background keys on an empty
    table; the same batch again at t + 1 is all hits, for the keys in their second bucket too.
    tab(): a host copy of the table's words (emulation only)."""
    keys = ks.exact_keys()
    ac.check_no_overflow(keys)
    batch = key_batch(wl, svcs, keys, 201, order)
    index = key_index(batch[1], svcs, keys)
    own = own_choices(clf, batch[1])
    step = Steps(rules, clf, runner, dst_known)
    lb0, st0, _ = step("t", batch, T0)
    bound = learned_endpoints(batch[1], lb0, index)
    for key, idx in index.items():
        assert bound[key] == ep_of(own, first_new(batch[1], idx))
    assert st0["learned"] == st0["live"] == len(keys) and st0["overflow"] == 0
    if tab is not None:
        assert all(len(slot_of(tab(), k)) == 1 and slot_of(tab(), k)[0] in k.c for k in keys)
        second = [k for k in keys if slot_of(tab(), k)[0] in k.c[2:] and k.c[0] != k.c[2]]
        assert len(second) >= 2, "no key had to use its second bucket"
    lb1, st1, _ = step("t+1", batch, T0 + 1)
    check_all_hits(lb1, index, bound)
    assert st1["learned"] == len(keys) and st1["hits"] - st0["hits"] == len(batch[1]["dport"])


def case_emptied_bucket(wl, rules, clf, svcs, ks, runner, order, tab=None, dst_known=False):
    """A live key behind an emptied bucket: a1, a2 fill the shared first bucket, b1, b2 spill to their
    second buckets, a1 and a2 expire and are swept; b1 and b2 must still be found, and a1, a2 come
    back into the freed bucket."""
    a1, a2, b1, b2 = ks.shared
    first = set(a1.c[:2])
    assert all(set(k.c[:2]) == first for k in ks.shared)
    step = Steps(rules, clf, runner, dst_known)
    ca = key_batch(wl, svcs, [a1, a2], 211, order)
    cb = key_batch(wl, svcs, [b1, b2], 212, order)
    ib = key_index(cb[1], svcs, [b1, b2])
    step("a1 a2", ca, T0)
    if tab is not None:
        assert {s for k in (a1, a2) for s in slot_of(tab(), k)} == first
    lb, st, _ = step("b1 b2 spill", cb, T0 + 1)
    bound = learned_endpoints(cb[1], lb, ib)
    assert st["live"] == 4 and st["learned"] == 4
    if tab is not None:
        assert all(slot_of(tab(), k)[0] in k.c[2:] for k in (b1, b2))
    cb2 = key_batch(wl, svcs, [b1, b2], 213, order, established=0.5)
    lb, st, live = step("behind the emptied bucket", cb2, T0 + P_TIMEOUTS[0])
    if tab is not None:
        assert not tab().reshape(-1, emu_aff6.SLOT_WORDS)[sorted(first), :2].any(), "the shared bucket must be empty"
    check_all_hits(lb, key_index(cb2[1], svcs, [b1, b2]), bound)
    assert st["learned"] == 4 and st["live"] == 2 and len(live) == 2
    lb, st, live = step("a1 a2 again", ca, T0 + P_TIMEOUTS[0] + 1)
    learned_endpoints(ca[1], lb, key_index(ca[1], svcs, [a1, a2]))
    assert st["learned"] == 6 and st["live"] == 4
    if tab is not None:
        assert {s for k in (a1, a2) for s in slot_of(tab(), k)} == first


def case_full_bucket_forced(wl, rules, clf, svcs, ks, runner, order):
    """Six keys with the same four candidate slots, in an order that forces who holds a slot
    (tests/affinity_cases.py case_full_bucket_forced): the model is given the packets of the keys that
    hold a slot; a packet of another key carries neither flag and its own choice, and the overflow
    counter equals the +new packets of those keys."""
    a1, a2, b1, b2, b3, b4 = ks.identical
    model = Model(rules, {}, clf)
    overflow = learned = 0
    script = [("t", T0, [a1, a2, b1, b2], [a1, a2, b1, b2], 4, 201),
              ("t+1", T0 + 1, [a1, a2, b1, b2, b3, b4], [a1, a2, b1, b2], 0, 202),
              ("t+40", T0 + P_TIMEOUTS[0], [b1, b2, b3, b4], [b1, b2, b3, b4], 2, 203),
              ("t+41", T0 + P_TIMEOUTS[0] + 1, [a1, a2, b1, b2, b3, b4], [b1, b2, b3, b4], 0, 204)]
    for name, now, keys, holders, n_learn, seed in script:
        cols4, cols = key_batch(wl, svcs, keys, seed, order)
        index = key_index(cols, svcs, keys)
        own_v, own = own_choices(clf, cols, verdicts=True)
        v, lb, live, stats, n_all = runner(name, cols, now)
        held = np.zeros(len(cols["dport"]), bool)
        for k in holders:
            held[index[k]] = True
        want_v, want_lb = model.run({c: np.ascontiguousarray(a[held]) for c, a in cols.items()}, now)
        _cmp(v[held], want_v, {c: a[held] for c, a in cols4.items()})
        assert (lb[held] == want_lb).all(), name
        assert ((lb["flags"][held] & gpc.LB_LEARNED) != 0).sum() == n_learn, name
        learned += n_learn
        assert ((lb["flags"][~held] & FLAGS) == 0).all() and (lb[~held] == own[~held]).all(), name
        _cmp(v[~held], own_v[~held], {c: a[~held] for c, a in cols4.items()})
        overflow += int(((cols["ct_state"][~held] & 1) != 0).sum())
        assert stats["overflow"] == overflow and stats["learned"] == learned == model.pipe.n_learned, (name, stats)
        assert stats["hits"] == model.pipe.n_hits and stats["live"] == n_all == len(holders), (name, stats)
        a, b = entry_sets(live, model.pipe.live())
        assert a == b, name
    assert overflow > 100


def case_sequence_wrap(wl, rules, clf, svcs, ks, runner, set_seq, order, dst_known=False):
    """The 32-bit launch sequence wraps (tests/affinity_cases.py case_sequence_wrap): 20 keys learn; the
    sequence is set to 0xfffffffc and two batches of ten further keys each leave bids of the sequences
    0xfffffffd and 0xfffffffe behind; the clock passes A's timeout, so the sweep frees all 40 slots
    with their bid words in place; the next batch (all 40 keys) wraps: the bid words must start over."""
    keys = ks.spread(0, 40)
    step = Steps(rules, clf, runner, dst_known)
    lb, st, _ = step("20 keys", key_batch(wl, svcs, keys[:20], 221, order), T0)
    assert st["learned"] == 20
    set_seq(0xfffffffc)
    for i, part in enumerate((keys[20:30], keys[30:])):
        lb, st, _ = step("before the wrap %d" % i, key_batch(wl, svcs, part, 222 + i, order), T0)
    assert st["learned"] == 40
    batch = key_batch(wl, svcs, keys, 224, order)
    index = key_index(batch[1], svcs, keys)
    own = own_choices(clf, batch[1])
    lb, st, _ = step("the wrap", batch, T0 + P_TIMEOUTS[0])
    bound = learned_endpoints(batch[1], lb, index)
    for key, idx in index.items():
        assert bound[key] == ep_of(own, first_new(batch[1], idx))
    assert st["learned"] == 80 and st["live"] == 40
    after = key_batch(wl, svcs, keys, 225, order)
    lb, st, _ = step("after the wrap", after, T0 + P_TIMEOUTS[0] + 1)
    check_all_hits(lb, key_index(after[1], svcs, keys), bound)
    assert st["learned"] == 80


def case_digest_collisions(wl, rules, clf, svcs, ks8, runner, order):
    """The digest narrowed to 8 bits (ks8: KeySet(clf, bits=8) of a product whose table has the same
    width): x and y are clients of Service A with equal digests, z a client of another digest.
      one batch      the first of x, y in caller order learns; the other's packets take their own
                     choices, carry no flag and its +new packets count as overflow
      a later batch  the same with the first learned earlier and live
      after expiry   the loser alone learns into the swept slot; the earlier winner, coming back while
                     that entry lives, is now the one that is not learned
    The model is told which key may not be learned; everything is compared exactly."""
    x, y = ks8.same_digest(0)
    z = next(k for k in (ks8.key(0, i) for i in range(64)) if k.d != x.d and not set(k.c) & set(x.c))
    assert x.d == y.d and x.src != y.src and x.c == y.c
    step = Steps(rules, clf, runner)
    pipe = step.model.pipe
    keys = [x, y, z]
    batch = key_batch(wl, svcs, keys, 231, order, established=0.2)
    index = key_index(batch[1], svcs, keys)
    own = own_choices(clf, batch[1])
    win, lose = (x, y) if first_new(batch[1], index[x]) < first_new(batch[1], index[y]) else (y, x)
    block = lambda k: {(6, 80, ip6(svcs[0][0]["ip"]), k.src)}
    pipe.blocked = block(lose)
    lb, st, live = step("one batch", batch, T0)
    assert ((lb["flags"][index[lose]] & FLAGS) == 0).all() and (lb[index[lose]] == own[index[lose]]).all()
    n_new = lambda b, idx: int(((b[1]["ct_state"][idx] & 1) != 0).sum())
    over = n_new(batch, index[lose])
    assert st["overflow"] == over > 0 and st["learned"] == 2 and st["live"] == 2
    bound = learned_endpoints(batch[1], lb, {win: index[win], z: index[z]})
    assert len({ep_of(own, i) for i in index[lose]}) >= 3, "the loser's own choices must spread"
    # a later batch: the winner is live, the loser still cannot learn and never gets the winner's Endpoint
    b2 = key_batch(wl, svcs, keys, 232, order, established=0.2)
    i2 = key_index(b2[1], svcs, keys)
    own2 = own_choices(clf, b2[1])
    lb, st, live = step("a later batch", b2, T0 + 1)
    check_all_hits(lb, {win: i2[win], z: i2[z]}, bound)
    assert ((lb["flags"][i2[lose]] & FLAGS) == 0).all() and (lb[i2[lose]] == own2[i2[lose]]).all()
    over += n_new(b2, i2[lose])
    assert st["overflow"] == over and st["learned"] == 2
    # past the timeout the slot is swept: the loser alone learns
    pipe.blocked = set()
    b3 = key_batch(wl, svcs, [lose], 233, order, established=0.2)
    lb, st, live = step("after expiry", b3, T0 + P_TIMEOUTS[0])
    learned_endpoints(b3[1], lb, key_index(b3[1], svcs, [lose]))
    assert st["learned"] == 3 and st["live"] == 1 and st["overflow"] == over
    pipe.blocked = block(win)
    b4 = key_batch(wl, svcs, [win, lose], 234, order, established=0.2)
    i4 = key_index(b4[1], svcs, [win, lose])
    lb, st, live = step("the earlier winner comes back", b4, T0 + P_TIMEOUTS[0] + 1)
    assert ((lb["flags"][i4[win]] & FLAGS) == 0).all() and ((lb["flags"][i4[lose]] & FLAGS) == gpc.LB_AFFINITY).all()
    assert st["overflow"] == over + n_new(b4, i4[win]) and st["learned"] == 3 and st["live"] == 1
