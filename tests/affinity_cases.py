"""Shared by tests/test_affinity.py (host emulation) and tests/test_gpu_affinity.py (device): the
session-affinity workload, its batches, the model over the realized text and the scripted
time / Endpoint-change / reinstall sequence. The sequence is run by a `runner(step name, columns,
clock) -> (verdicts, lb results, reachable live entries, stats, live entries in all)` of the side under
test and compared, step by step and exactly, with the model (tests/affinity_model.py). Reachable:
entries of an install id that is still realized -- a reinstalled or uninstalled Service's entries are
orphaned (no packet can match them any more, which is what delete_learned achieves) and stay in the
table until their timeout."""
import collections
import copy
import ipaddress

import numpy as np

from antrea_amd import gpc, workload
from oracle import compiler as oc
from tests import affinity_model, emu_aff
from tests.test_emu_parity import _cmp

T = 100       # affinity timeout of the workload's Services (seconds)
T0 = 1000     # clock of the first batch
LOG2 = 12     # table size of the equality tests: 4096 slots for a few hundred keys (no overflow)
SVC_TABLES = ("table=ServiceLB", "table=EndpointDNAT", "table=NodePortMark")


def make_workload(seed):
    """C1 + 60 Services: 40 % with session affinity, 30 % NodePort, 10 % without Endpoints."""
    wl = workload.config1(seed=seed)
    return workload.add_services(wl, 60, 4, seed=seed, noep_frac=0.1, local_policy_frac=0.2, nodeport_frac=0.3,
                                 affinity_frac=0.4, affinity_timeout=T)


def make_product(wl, log2=LOG2, **kw):
    c = gpc.Classifier(session_affinity=log2, **kw)
    c.initialize()
    c.batch_install_policy_rule_flows(copy.deepcopy(wl.rules))
    workload.install_services(c, wl)
    return c


def make_batch(wl, n, seed, clients=16, established=0.0):
    """n packets, most to a Service, from `clients` source addresses (so keys repeat inside a batch);
    `established` > 0: a ct_state column in which that share of the packets is +est instead of +new."""
    frac, wl.svc_frac = wl.svc_frac, 0.8
    cols = workload.gen_packets(wl, n, seed=seed)
    wl.svc_frac = frac
    rng = np.random.default_rng(seed + 1)
    pool = cols["src"][:clients].copy()
    cols["src"] = pool[rng.integers(0, clients, size=n)].astype(np.uint32)
    if established > 0:
        est = rng.random(n) < established
        cols["ct_state"] = np.where(est, gpc_ct("est"), gpc_ct("new")).astype(np.uint8)
    return cols


def gpc_ct(kind):
    return {"new": 0x01 | 0x20, "est": 0x02 | 0x20}[kind]


class Model:
    """The model over the product's realized Service text and the oracle compiler's NP flows."""

    def __init__(self, wl, clf):
        self.wl = wl
        self.rules = copy.deepcopy(wl.rules)
        self.pipe = None
        self.refresh(clf)

    def refresh(self, clf, reinstalled=()):
        fnp = oc.FeatureNetworkPolicy()
        fnp.initialize()
        fnp.batch_install_policy_rule_flows(copy.deepcopy(self.rules))
        svc_flows = [f for f in clf.dump_flows() if any(t in f for t in SVC_TABLES)]
        tiers = {r["flow_id"]: int(r.get("tier_priority") or 0) for r in self.rules}
        args = (fnp.dump_flows() + svc_flows, tiers, clf.dump_groups(), self.wl.pods)
        if self.pipe is None:
            self.pipe = affinity_model.AffinityPipeline(*args)
        else:
            self.pipe.set_flows(*args, reinstalled=reinstalled)

    def run(self, cols, now):
        self.pipe.now = now
        return affinity_model.run(self.pipe, cols)


def check_step(name, cols, got, want, model_live, got_live, model_counts, got_stats, n_live_all, dst_known=False):
    """Verdicts, LB results (the two affinity flag bits included), live entries, counters: exact."""
    v, lb = got
    wv, wlb = want
    _cmp(v, wv, cols)
    bad = np.nonzero(lb != wlb)[0]
    assert len(bad) == 0, (name, bad[:5], lb[bad[:3]], wlb[bad[:3]])
    # live entries: (src, endpoint ip, endpoint port | REMOTE, expires) of both sides (the model keys
    # by destination address, the table by install and address ids)
    assert sorted((e[0],) + tuple(e[2:]) for e in got_live) == sorted((e[0],) + tuple(e[2:]) for e in model_live), name
    if dst_known:  # gpc_debug_affinity_table names the destination: the learned flows' NXM_OF_IP_DST too
        assert sorted(got_live) == sorted(model_live), name
    assert got_stats["overflow"] == 0, (name, got_stats)
    assert (got_stats["learned"], got_stats["hits"]) == model_counts, (name, got_stats, model_counts)
    assert got_stats["live"] == n_live_all >= len(model_live), (name, got_stats, n_live_all, len(model_live))


def scripted_sequence(wl, clf, commit, runner, n=500, seed=7, established=0.0, dst_known=False):
    """batch at t; the same at t + 1 (all hits); at t + T - 1; at t + T (all re-learn); after removing
    one Endpoint of an affinity Service and committing (only its clients re-learn); after
    reinstalling one Service (its clients re-learn, no others); after a NetworkPolicy-only commit
    (nothing changes). `commit()` publishes clf's pending state; `runner` is the side under test."""
    commit()
    model = Model(wl, clf)
    cols = make_batch(wl, n, seed, established=established)
    learned_by_step = {}

    def step(name, now, c=cols):
        want = model.run(c, now)
        v, lb, live, stats, n_all = runner(name, c, now)
        check_step(name, c, (v, lb), want, model.pipe.live(), live, (model.pipe.n_learned, model.pipe.n_hits), stats, n_all,
                   dst_known)
        learned_by_step[name] = lb[(lb["flags"] & gpc.LB_LEARNED) != 0]
        return lb

    lb0 = step("t", T0)
    n_keys = len(learned_by_step["t"])
    assert n_keys > 20 and ((lb0["flags"] & gpc.LB_AFFINITY) != 0).sum() > n_keys, "keys must repeat inside the batch"
    assert (lb0["flags"] & gpc.LB_NO_ENDPOINT).any() and ((lb0["flags"] & (gpc.LB_HIT | gpc.LB_AFFINITY)) == gpc.LB_HIT).any()
    lb1 = step("t+1", T0 + 1)
    assert len(learned_by_step["t+1"]) == 0
    aff = (lb0["flags"] & gpc.LB_AFFINITY) != 0
    if established == 0.0:  # every packet of an affinity Service now takes its key's learned Endpoint
        assert (lb1["endpoint_ip"][aff] != 0).all() and ((lb1["flags"][aff] & gpc.LB_AFFINITY) != 0).all()
    step("t+T-1", T0 + T - 1)
    assert len(learned_by_step["t+T-1"]) == 0
    step("t+T", T0 + T)
    assert len(learned_by_step["t+T"]) == n_keys  # hard timeout: the hits did not refresh anything
    # --- one Endpoint of an affinity Service leaves its group
    groups = {int(g): cnt for g, cnt in zip(*np.unique(learned_by_step["t+T"]["group_id"], return_counts=True))}
    gid = next(g for g in sorted(groups, key=lambda g: -groups[g]) if len(wl.groups[g]) >= 2)
    gone = wl.groups[gid][0]
    wl.groups[gid] = wl.groups[gid][1:]
    clf.install_service_group(gid, wl.groups[gid], True)
    commit()
    model.refresh(clf)
    import ipaddress
    bound = learned_by_step["t+T"]
    n_bound = int(((bound["group_id"] == gid) & (bound["endpoint_ip"] == int(ipaddress.ip_address(gone["ip"]))) &
                   (bound["endpoint_port"] == gone["port"])).sum())
    assert n_bound > 0
    step("endpoint removed", T0 + T + 1)
    rl = learned_by_step["endpoint removed"]
    assert len(rl) == n_bound and (rl["group_id"] == gid).all(), (len(rl), n_bound)
    # --- one affinity Service installed again: a new install id, its learned flows are orphaned
    cfg = next(s for s in wl.services if s.get("affinity_timeout") and not s.get("is_nodeport") and
               (s["local_group_id"] if s["traffic_policy_local"] else s["cluster_group_id"]) in groups and
               (s["local_group_id"] if s["traffic_policy_local"] else s["cluster_group_id"]) != gid)
    gid2 = cfg["local_group_id"] if cfg["traffic_policy_local"] else cfg["cluster_group_id"]
    clf.install_service_flows(cfg)
    commit()
    model.refresh(clf, reinstalled=[(dict(workload.SVC_PROTOS)[cfg["protocol"]], int(ipaddress.ip_address(cfg["ip"])),
                                     cfg["port"])])
    step("reinstalled", T0 + T + 2)
    rl = learned_by_step["reinstalled"]
    assert len(rl) == groups[gid2] and (rl["group_id"] == gid2).all(), (len(rl), groups[gid2])
    # --- a NetworkPolicy-only commit: the table is not an epoch's
    extra = dict(copy.deepcopy(wl.rules[0]), flow_id=max(r["flow_id"] for r in wl.rules) + 1)
    clf.install_policy_rule_flows(copy.deepcopy(extra))
    model.rules.append(extra)
    commit()
    model.refresh(clf)
    step("np commit", T0 + T + 3)
    assert len(learned_by_step["np commit"]) == 0
    return model


# ------------------------------------------------------------------ the table under hash pressure
# A table of 2^8 slots (128 buckets of two) and keys chosen, with the product's own hash
# (emu_aff.candidates), to share buckets. Which slot a key lands in depends on the arrival order; the
# results do not, as long as every key lands in one. check_no_overflow() is the sufficient condition
# for that, whatever the order: so the device, the serial emulation and the model (which has no
# capacity at all) must agree exactly.
P_LOG2 = 8
P_TIMEOUTS = (40, 200)                # Service A, Service B
P_NETS = (0x0a640000, 0x0a650000)     # the /16 the clients of A / of B are searched in
P_PER_KEY = 64
P_CFG = {"ip": "10.96.0.100", "port": 80, "protocol": "TCP", "cluster_group_id": 100, "local_group_id": 101}
Key = collections.namedtuple("Key", "svc src c")  # Service (0: A, 1: B), client address, the four candidate slots


def make_pressure_product(**kw):
    """C1's rules + the affinity ClusterIP Services A (timeout 40) and B (timeout 200) of 8 remote
    Endpoints each over a table of 256 slots: (workload, product -- not committed yet, [(config, Endpoints)]).
    C1's rules name Pod addresses only, so one egress rule more applies to the two client networks and
    allows A's Endpoints and all but the last of B's: no batch's per-rule counters are empty, and some
    packets of B are dropped."""
    wl = workload.config1(seed=81)
    egress = next(r for r in wl.rules if r["direction"] == "Out" and not r.get("service"))
    wl.rules = copy.deepcopy(wl.rules) + [dict(copy.deepcopy(egress), flow_id=max(r["flow_id"] for r in wl.rules) + 1,
                                               **{"from": [{"ipnet": "10.100.0.0/15"}],
                                                  "to": [{"ipnet": "10.128.1.0/24"}, {"ipnet": "10.128.2.0/29"}]})]
    c = gpc.Classifier(session_affinity=P_LOG2, **kw)
    c.initialize()
    c.batch_install_policy_rule_flows(copy.deepcopy(wl.rules))
    svcs = []
    for s, timeout in enumerate(P_TIMEOUTS):
        eps = [{"ip": "10.128.%d.%d" % (s + 1, k + 1), "port": 8000 + k, "is_local": False, "node_name": "n%d" % k}
               for k in range(8)]
        cfg = dict(P_CFG, ip="10.96.0.%d" % (100 + s), cluster_group_id=100 + 2 * s, local_group_id=101 + 2 * s,
                   affinity_timeout=timeout)
        c.install_service_group(cfg["cluster_group_id"], eps, True)
        c.install_endpoint_flows("TCP", eps)
        c.install_service_flows(cfg)
        svcs.append((cfg, eps))
    wl.pods = {}
    return wl, c, svcs


def neighbours(k, keys):
    """The other keys of the set that share a candidate slot with k."""
    return [o for o in keys if o != k and set(o.c) & set(k.c)]


def no_overflow(keys):
    """Every key has more distinct candidate slots than neighbours: whatever the arrival order, when
    a key looks for a slot its neighbours hold fewer slots than it has candidates, so one is free."""
    return all(len(neighbours(k, keys)) < len(set(k.c)) for k in keys)


def check_no_overflow(keys):
    assert len(set(keys)) == len(keys)
    bad = [(k, len(neighbours(k, keys))) for k in keys if len(neighbours(k, keys)) >= len(set(k.c))]
    assert not bad, "key set may overflow, so no exact result exists: %r" % (bad[:3],)


class KeySet:
    """Clusters of colliding keys of the committed Services A and B, found by a search over 2^16
    client addresses per Service. Buckets: b1 = c[0] >> 1, b2 = c[2] >> 1. No bucket is used by two
    clusters or by a cluster and a background key.
      shared     a1, a2, b1, b2 with one common first bucket; the second buckets pairwise distinct
      degenerate a key of A with b1 == b2 (two distinct slots), a key of B whose first bucket that is
      chain      F (of A) whose second bucket is the first bucket of G (of B)
      identical  a1, a2, b1 .. b4 with the same bucket pair b1 != b2: six keys for four slots, the one
                 cluster that overflows (on purpose; never part of exact_keys())
      background 30 keys (pairs of one A and one B key with the same bucket pair) away from all of them"""
    N = 1 << 16

    def __init__(self, clf):
        by_group = {gid: inst for inst, gid, _ in emu_aff.affinity_services(clf)}
        self.install = [by_group[100], by_group[102]]
        self.cand = [emu_aff.candidates(inst, net, P_LOG2, n=self.N) for inst, net in zip(self.install, P_NETS)]
        self.b1 = [(c[:, 0] >> 1).astype(np.int64) for c in self.cand]
        self.b2 = [(c[:, 2] >> 1).astype(np.int64) for c in self.cand]
        assert all((c[:, 1] == c[:, 0] + 1).all() and (c[:, 3] == c[:, 2] + 1).all() and (c < (1 << P_LOG2)).all() for c in self.cand)
        self.used = set()
        self.identical = self._identical()
        self.shared = self._shared()
        self.degenerate = self._degenerate()
        self.chain = self._chain()
        self.background = self._background(30)
        check_no_overflow(self.exact_keys())
        assert not no_overflow(self.identical)
        cluster_buckets = lambda keys: {s >> 1 for k in keys for s in k.c}
        groups = [self.identical, self.shared, self.degenerate, self.chain, self.background]
        for i, g in enumerate(groups):  # no bucket belongs to two clusters
            for h in groups[i + 1:]:
                assert not cluster_buckets(g) & cluster_buckets(h)

    def key(self, svc, i):
        return Key(svc, P_NETS[svc] + int(i), tuple(int(x) for x in self.cand[svc][i]))

    def _free(self, b):
        return ~np.isin(b, sorted(self.used))

    def _take(self, keys):
        self.used |= {s >> 1 for k in keys for s in k.c}
        return keys

    def _where(self, svc, mask, what, n=1):
        idx = np.nonzero(mask)[0]
        assert len(idx) >= n, "no %s among the %d clients searched" % (what, self.N)
        return idx

    def _identical(self):
        pair = [self.b1[s] * 128 + self.b2[s] for s in (0, 1)]
        cnt = [np.bincount(p[self.b1[s] != self.b2[s]], minlength=128 * 128) for s, p in enumerate(pair)]
        p = self._where(0, (cnt[0] >= 2) & (cnt[1] >= 4), "bucket pair with 2 + 4 keys")[0]
        keys = [self.key(0, i) for i in np.nonzero(pair[0] == p)[0][:2]] + [self.key(1, i) for i in np.nonzero(pair[1] == p)[0][:4]]
        assert len({k.c for k in keys}) == 1 and len(set(keys[0].c)) == 4
        return self._take(keys)

    def _shared(self):
        x = min(set(range(128)) - self.used)
        keys, seconds = [], {x}
        for s in (0, 1):
            got = 0
            for i in self._where(s, (self.b1[s] == x) & self._free(self.b2[s]), "key with first bucket %d" % x, 2):
                if got < 2 and int(self.b2[s][i]) not in seconds:
                    seconds.add(int(self.b2[s][i]))
                    keys.append(self.key(s, i))
                    got += 1
            assert got == 2
        self.used.add(x)
        return self._take(keys)

    def _degenerate(self):
        for i in self._where(0, (self.b1[0] == self.b2[0]) & self._free(self.b1[0]), "key with b1 == b2"):
            d = self.b1[0][i]
            j = np.nonzero((self.b1[1] == d) & (self.b2[1] != d) & self._free(self.b2[1]))[0]
            if len(j):
                keys = [self.key(0, i), self.key(1, j[0])]
                assert len(set(keys[0].c)) == 2 and keys[1].c[0] == keys[0].c[0]
                return self._take(keys)
        raise AssertionError("no degenerate key with a neighbour")

    def _chain(self):
        for i in self._where(0, (self.b1[0] != self.b2[0]) & self._free(self.b1[0]) & self._free(self.b2[0]), "chain head"):
            p, q = self.b1[0][i], self.b2[0][i]
            j = np.nonzero((self.b1[1] == q) & self._free(self.b2[1]) & (self.b2[1] != p) & (self.b2[1] != q))[0]
            if len(j):
                return self._take([self.key(0, i), self.key(1, j[0])])
        raise AssertionError("no chain")

    def _background(self, n):
        keys = []
        pair1 = self.b1[1] * 128 + self.b2[1]
        for i in np.nonzero(self.b1[0] != self.b2[0])[0]:
            p, q = int(self.b1[0][i]), int(self.b2[0][i])
            if p in self.used or q in self.used:
                continue
            j = np.nonzero(pair1 == p * 128 + q)[0]
            if len(j):
                keys += self._take([self.key(0, i), self.key(1, j[0])])
            if len(keys) >= n:
                return keys
        raise AssertionError("only %d background keys" % len(keys))

    def exact_keys(self):
        return self.shared + self.degenerate + self.chain + self.background

    def spread(self, svc, n):
        """n keys of one Service with 2 n distinct buckets among them (an own key set: not to be mixed
        with the clusters)."""
        keys, used = [], set()
        for i in np.nonzero(self.b1[svc] != self.b2[svc])[0]:
            p, q = int(self.b1[svc][i]), int(self.b2[svc][i])
            if p not in used and q not in used:
                used |= {p, q}
                keys.append(self.key(svc, i))
                if len(keys) == n:
                    check_no_overflow(keys)
                    return keys
        raise AssertionError("only %d spread keys" % len(keys))

    def word(self, k):
        """The key word of k (core.hpp aff_key, NodePort address id 0)."""
        return (self.install[k.svc] << 40) | k.src

    def slot_of(self, table, k):
        """The slots of the emulated table (emu_aff.Table) that hold k's key word."""
        t = table.tab.reshape(-1, 8)
        words = t[:, 0].astype(np.uint64) | (t[:, 1].astype(np.uint64) << np.uint64(32))
        return [int(s) for s in np.nonzero(words == np.uint64(self.word(k)))[0]]


def key_batch(wl, svcs, keys, seed, order=0, per_key=P_PER_KEY, established=0.3):
    """per_key packets of every key to its Service, random source ports, `established` of them +est,
    the whole batch shuffled; `order` picks the shuffle of the same packets."""
    n = len(keys) * per_key
    assert n <= 8192
    rng = np.random.default_rng(seed)
    cols = workload.gen_packets(wl, n, seed=seed)
    k = np.repeat(np.arange(len(keys)), per_key)
    dst = [int(ipaddress.ip_address(svcs[key.svc][0]["ip"])) for key in keys]
    cols["src"] = np.array([key.src for key in keys], np.uint32)[k]
    cols["dst"] = np.array(dst, np.uint32)[k]
    cols["dport"] = np.full(n, 80, np.uint16)
    cols["proto"] = np.full(n, 6, np.uint8)
    cols["sport"] = rng.integers(1024, 65536, size=n).astype(np.uint16)
    cols["ct_state"] = np.where(rng.random(n) < established, gpc_ct("est"), gpc_ct("new")).astype(np.uint8)
    perm = np.random.default_rng([seed, order]).permutation(n)
    return {name: np.ascontiguousarray(v[perm]) for name, v in cols.items()}


def key_index(cols, svcs, keys):
    """{key: caller indexes of its packets, ascending}."""
    out = {}
    for key in keys:
        dst = int(ipaddress.ip_address(svcs[key.svc][0]["ip"]))
        out[key] = np.nonzero((cols["src"] == key.src) & (cols["dst"] == dst))[0]
        assert len(out[key])
    assert sum(len(v) for v in out.values()) == len(cols["src"])
    return out


def own_choices(clf, cols, verdicts=False):
    """Every packet's own hash choice (the plain Service stage), (n,) LB_DTYPE; with `verdicts`,
    (the verdicts of the packets so balanced, the choices)."""
    from tests import emu
    own = np.zeros(len(cols["src"]), gpc.LB_DTYPE)
    v = emu.classify(clf, cols, lb=own)
    return (v, own) if verdicts else own


def check_spread(own, index):
    """The keys' own choices spread over the Endpoints: without it "the key's learned Endpoint" and
    "the packet's own choice" could not be told apart."""
    for key, idx in index.items():
        assert len(idx) < 8 or len(set(own["endpoint_ip"][idx].tolist())) >= 4, key


def first_new(cols, idx):
    new = (cols["ct_state"][idx] & 1) != 0
    assert new.any()
    return int(idx[new][0])


FLAGS = gpc.LB_AFFINITY | gpc.LB_LEARNED


class Steps:
    """One side under test (a runner, see the module docstring) stepped beside the model."""

    def __init__(self, wl, clf, runner, dst_known=False):
        self.model = Model(wl, clf)
        self.runner, self.dst_known = runner, dst_known

    def __call__(self, name, cols, now):
        """Exact: verdicts, LB results, live entries, learned / hits, overflow == 0. -> (lb, stats, live)."""
        want = self.model.run(cols, now)
        v, lb, live, stats, n_all = self.runner(name, cols, now)
        p = self.model.pipe
        check_step(name, cols, (v, lb), want, p.live(), live, (p.n_learned, p.n_hits), stats, n_all, self.dst_known)
        assert len({(e[0], e[1]) for e in live}) == len(live) == n_all, name  # one entry per key
        return lb, stats, live


def learned_endpoints(cols, lb, index):
    """{key: (endpoint ip, endpoint port) of its one GPC_LB_LEARNED packet}, which must be the key's
    first +new packet by caller index."""
    out = {}
    for key, idx in index.items():
        l = idx[(lb["flags"][idx] & gpc.LB_LEARNED) != 0]
        assert list(l) == [first_new(cols, idx)], key
        out[key] = (int(lb["endpoint_ip"][l[0]]), int(lb["endpoint_port"][l[0]]))
    return out


def check_all_hits(lb, index, bound):
    """Every packet of every key: GPC_LB_AFFINITY without GPC_LB_LEARNED, the key's learned Endpoint."""
    for key, idx in index.items():
        assert ((lb["flags"][idx] & FLAGS) == gpc.LB_AFFINITY).all(), key
        assert (lb["endpoint_ip"][idx] == bound[key][0]).all() and (lb["endpoint_port"][idx] == bound[key][1]).all(), key


def case_collisions(wl, clf, svcs, ks, table, runner, order, dst_known=False):
    """Collisions in one batch: every cluster but `identical`, and the background keys, on an empty
    table; the same batch again at t + 1 is all hits, for the keys in their second bucket too."""
    keys = ks.exact_keys()
    check_no_overflow(keys)
    cols = key_batch(wl, svcs, keys, 201, order)
    assert 2000 <= len(cols["src"]) <= 6000
    index = key_index(cols, svcs, keys)
    own = own_choices(clf, cols)
    check_spread(own, index)
    step = Steps(wl, clf, runner, dst_known)
    lb0, st0, _ = step("t", cols, T0)
    bound = learned_endpoints(cols, lb0, index)
    for key, idx in index.items():
        f = first_new(cols, idx)
        assert bound[key] == (int(own["endpoint_ip"][f]), int(own["endpoint_port"][f]))
    assert st0["learned"] == st0["live"] == len(keys)
    second = [k for k in keys if set(ks.slot_of(table, k)) & set(k.c[2:]) and k.c[0] != k.c[2]]
    assert len(second) >= 2, "no key had to use its second bucket"
    assert all(len(ks.slot_of(table, k)) == 1 and ks.slot_of(table, k)[0] in k.c for k in keys)
    lb1, st1, _ = step("t+1", cols, T0 + 1)
    check_all_hits(lb1, index, bound)
    assert st1["learned"] == len(keys) and st1["hits"] - st0["hits"] == len(cols["src"])
    return second


def case_emptied_bucket(wl, clf, svcs, ks, table, runner, commit, order, dst_known=False):
    """A live key behind an emptied bucket: a1, a2 fill the shared first bucket, b1, b2 spill to their
    second buckets, a1 and a2 expire and are swept. b1 and b2 must still be found (a find must not stop
    at an empty slot), and a re-learn of b1 must reuse b1's slot (not claim the freed first bucket)."""
    a1, a2, b1, b2 = ks.shared
    check_no_overflow(ks.shared)
    first = set(a1.c[:2])
    assert all(set(k.c[:2]) == first for k in ks.shared)
    step = Steps(wl, clf, runner, dst_known)
    ca = key_batch(wl, svcs, [a1, a2], 211, order)
    for seed in range(2120, 2140):  # a batch in which b1's and b2's first +new packets choose different Endpoints
        cb = key_batch(wl, svcs, [b1, b2], seed, order)
        ib = key_index(cb, svcs, [b1, b2])
        own = own_choices(clf, cb)
        if own[first_new(cb, ib[b1])] != own[first_new(cb, ib[b2])]:
            break
    ia = key_index(ca, svcs, [a1, a2])
    check_spread(own, ib)
    lb, st, _ = step("a1 a2", ca, T0)
    assert {s for k in (a1, a2) for s in ks.slot_of(table, k)} == first
    lb, st, _ = step("b1 b2 spill", cb, T0 + 1)
    bound = learned_endpoints(cb, lb, ib)
    assert all(ks.slot_of(table, k)[0] in k.c[2:] for k in (b1, b2)) and st["live"] == 4 and st["learned"] == 4
    assert bound[b1] != bound[b2], "b1 and b2 must be bound to different Endpoints for what follows"
    # the sweep at t + 40 empties the shared bucket; b1 and b2 live on behind it
    cb2 = key_batch(wl, svcs, [b1, b2], 213, order, established=0.5)
    ib2 = key_index(cb2, svcs, [b1, b2])
    lb, st, live = step("behind the emptied bucket", cb2, T0 + P_TIMEOUTS[0])
    assert not (table.tab.reshape(-1, 8)[sorted(first), :2]).any(), "the shared bucket must be empty"
    check_all_hits(lb, ib2, bound)
    assert st["learned"] == 4 and st["live"] == 2 and len(live) == 2
    # the Endpoint b1 is bound to leaves B's group: b1 re-learns in place, b2 is untouched
    cfg, eps = svcs[1]
    left = [e for e in eps if (int(ipaddress.ip_address(e["ip"])), e["port"]) != bound[b1]]
    assert len(left) == len(eps) - 1
    clf.install_service_group(cfg["cluster_group_id"], left, True)
    commit()
    step.model.refresh(clf)
    cb3 = key_batch(wl, svcs, [b1, b2], 214, order, established=0.5)
    ib3 = key_index(cb3, svcs, [b1, b2])
    lb, st, live = step("b1 re-learns", cb3, T0 + P_TIMEOUTS[0] + 1)
    rebound = learned_endpoints(cb3, lb, {b1: ib3[b1]})
    assert rebound[b1] != bound[b1] and ((lb["flags"] & gpc.LB_LEARNED) != 0).sum() == 1
    check_all_hits(lb, {b2: ib3[b2]}, bound)
    assert st["learned"] == 5 and st["live"] == 2 and len(live) == 2
    assert all(len(ks.slot_of(table, k)) == 1 and ks.slot_of(table, k)[0] in k.c[2:] for k in (b1, b2))
    # a1 and a2 come back into the freed bucket
    lb, st, live = step("a1 a2 again", ca, T0 + P_TIMEOUTS[0] + 2)
    learned_endpoints(ca, lb, ia)
    assert st["learned"] == 7 and st["live"] == 4
    assert {s for k in (a1, a2) for s in ks.slot_of(table, k)} == first


def case_full_bucket_forced(wl, clf, svcs, ks, runner, order, dst_known=False):
    """Six keys with the same four candidate slots, in an order that forces who holds a slot:
    a1 a2 b1 b2 at t; all six at t + 1 (b3, b4 overflow); b1 .. b4 at t + 40, when A's entries have
    expired (b3, b4 learn); all six at t + 41 (a1, a2 overflow). The model has no capacity: it is given
    the packets of the keys that hold a slot after the step's learn pass, in their order in the batch,
    and compared on those packets alone; a packet of another key must carry neither affinity flag and
    its own hash choice, and the overflow counter must equal the +new packets of those keys."""
    a1, a2, b1, b2, b3, b4 = ks.identical
    model = Model(wl, clf)
    overflow = learned = 0
    script = [("t", T0, [a1, a2, b1, b2], [a1, a2, b1, b2], 4, 201),
              ("t+1", T0 + 1, [a1, a2, b1, b2, b3, b4], [a1, a2, b1, b2], 0, 202),
              ("t+40", T0 + P_TIMEOUTS[0], [b1, b2, b3, b4], [b1, b2, b3, b4], 2, 203),
              ("t+41", T0 + P_TIMEOUTS[0] + 1, [a1, a2, b1, b2, b3, b4], [b1, b2, b3, b4], 0, 204)]
    for name, now, keys, holders, n_learn, seed in script:
        cols = key_batch(wl, svcs, keys, seed, order)
        index = key_index(cols, svcs, keys)
        own_v, own = own_choices(clf, cols, verdicts=True)
        check_spread(own, index)
        v, lb, live, stats, n_all = runner(name, cols, now)
        held = np.zeros(len(cols["src"]), bool)
        for k in holders:
            held[index[k]] = True
        want_v, want_lb = model.run({c: np.ascontiguousarray(a[held]) for c, a in cols.items()}, now)
        _cmp(v[held], want_v, {c: a[held] for c, a in cols.items()})
        assert (lb[held] == want_lb).all(), name
        assert ((lb["flags"][held] & gpc.LB_LEARNED) != 0).sum() == n_learn, name
        learned += n_learn
        assert ((lb["flags"][~held] & FLAGS) == 0).all() and (lb[~held] == own[~held]).all(), name
        _cmp(v[~held], own_v[~held], {c: a[~held] for c, a in cols.items()})
        overflow += int(((cols["ct_state"][~held] & 1) != 0).sum())
        assert (~held).sum() == 0 or int(((cols["ct_state"][~held] & 1) != 0).sum()) > 0
        assert stats["overflow"] == overflow and stats["learned"] == learned == model.pipe.n_learned, (name, stats)
        assert stats["hits"] == model.pipe.n_hits and stats["live"] == n_all == len(holders), (name, stats)
        assert sorted((e[0],) + tuple(e[2:]) for e in live) == sorted((e[0],) + tuple(e[2:]) for e in model.pipe.live()), name
        if dst_known:
            assert sorted(live) == model.pipe.live(), name
    assert overflow > 100


def case_sequence_wrap(wl, clf, svcs, ks, table, runner, set_seq, order, dst_known=False):
    """The 32-bit launch sequence wraps: 20 keys learn; the sequence is set to 0xfffffffc and two
    batches of ten further keys each leave bids of the sequences 0xfffffffd and 0xfffffffe behind; the
    clock passes A's timeout, so the sweep frees all 40 slots with their bid words in place; the next
    batch (all 40 keys) is the one that wraps: the bid words must start over, or no bid of sequence 1
    could undercut them and nothing would be learned in those slots."""
    keys = ks.spread(0, 40)
    step = Steps(wl, clf, runner, dst_known)
    c0 = key_batch(wl, svcs, keys[:20], 221, order)
    lb, st, _ = step("20 keys", c0, T0)
    assert st["learned"] == 20
    set_seq(0xfffffffc)
    for i, part in enumerate((keys[20:30], keys[30:])):
        lb, st, _ = step("before the wrap %d" % i, key_batch(wl, svcs, part, 222 + i, order), T0)
    assert st["learned"] == 40 and table.seq == 0xfffffffe
    bids = table.tab.reshape(-1, 8)[[ks.slot_of(table, k)[0] for k in keys], 3]
    assert sorted(set(bids.tolist())) == [1, 2, 0xfffffffe], "bids of the sequences 1, 0xfffffffd and 0xfffffffe"
    cols = key_batch(wl, svcs, keys, 224, order)
    index = key_index(cols, svcs, keys)
    own = own_choices(clf, cols)
    lb, st, _ = step("the wrap", cols, T0 + P_TIMEOUTS[0])
    assert table.seq == 1
    bound = learned_endpoints(cols, lb, index)
    for key, idx in index.items():
        f = first_new(cols, idx)
        assert bound[key] == (int(own["endpoint_ip"][f]), int(own["endpoint_port"][f]))
    assert st["learned"] == 80 and st["live"] == 40
    lb, st, _ = step("after the wrap", key_batch(wl, svcs, keys, 225, order), T0 + P_TIMEOUTS[0] + 1)
    check_all_hits(lb, key_index(key_batch(wl, svcs, keys, 225, order), svcs, keys), bound)
    assert st["learned"] == 80 and table.seq == 2
