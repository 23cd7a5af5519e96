"""Shared by tests/test_commit_failure_cases.py (host: the cases against the oracle, no device) and
tests/test_gpu_commit_failure.py (device): what a gpc_commit / gpc_compact / gpc_replay that fails
at any of its device allocations, copies or synchronizes leaves behind, and how the next call recovers.

The context: dual-stack, two device slots on one device ([0, 0]), no background compaction; C1 rules in
both families (workload.to_ipv6 dual), 60 IPv4 and 60 IPv6 Services (40 % with session affinity, 30 %
NodePort, some without Endpoints), two logged rules (a packet-in image), one batch of N packets per
family from 48 clients, 30 % of them +est.

A scenario is one pending change over a pre-state (SCENARIOS). run_case(scenario, way, side, k):
  k is None  the reference run: pre-state, change, call, the way's further change; every batch equals
             the emulation of the context's own images AND the independent oracle of its rule and
             Service set (oracle compiler + ovs_cls, the realized Service text through
             tests/affinity_model.py / affinity6_model.py, tests/packet_in_model.py). Returns the
             upload points the call passed and the results.
  k = 0 ..   the same on a fresh context with gpc_debug_fail_upload_at(k) armed: the call fails, the
             slots still serve the snapshot taken before it, the recovery (WAYS) brings both slots to
             the reference run's results, the emulation's, and the counter model's.

Session affinity makes every batch depend on the slot's table. Both slots see the same batches in the
same order, one oracle run stands for both, and the pre-state classifies the batch once before anything
is compared: from then on every key has its entry (the clock stands still) and a repeated batch
changes nothing in the table, so the batches that only a failing run classifies do not part its table
from the reference run's.

Counters: a serial model by conj id in the style of tests/counter_lifecycle.py -- metrics read before
the call, plus each counted batch's own counts (the emulation's, of the epoch it ran on), a rule's
entry dropped when the commit that publishes its uninstall succeeds, everything dropped by a replay."""
import copy
import ipaddress

import numpy as np

from antrea_amd import gpc, workload
from oracle import compiler as oc
from tests import affinity6_model, affinity_cases as ac, affinity_model, emu, emu_aff, emu_aff6, emu_pin, svc6_model
from tests import packet_in_model as pin_model

N = 2000          # packets per family and batch
SEED = 91
NOW = ac.T0       # the affinity clock stands still
LOG2 = ac.LOG2
GID6 = 1000       # offset of the IPv6 Services' group ids
SVC_TABLES = ("table=ServiceLB", "table=EndpointDNAT", "table=NodePortMark")
SCENARIOS = ("first", "delta", "delta2", "v6prefix", "compact", "svc_only", "pin_only", "reuse", "pool_gc", "replay")
# Recovery: (a) the same call again, (b) gpc_commit after one further small change, (c) gpc_commit
# with nothing pending (replay only). The same call again after a failed replay is "gpc_replay again".
WAYS = {s: "ab" for s in SCENARIOS}
WAYS["replay"] = "abc"
# What the call must at least pass, over both slots (the unarmed run asserts it): per slot ...
MIN_POINTS = {
    "first": 16,     # both bases, three images, counter allocation + clearing, synchronize
    "delta": 10,     # two pools, two tails, synchronize
    "delta2": 6,     # two tails, synchronize
    "v6prefix": 6,
    "compact": 16,   # as "first"
    "svc_only": 6,   # two Service images, synchronize
    "pin_only": 4,   # the packet-in image, synchronize
    "reuse": 6,
    "pool_gc": 6,    # a fresh pool, its tail, synchronize
    "replay": 24,    # both bases, two pools and their copies, three images, counters (2), synchronize
}
FOLLOWED = ("delta", "delta2", "v6prefix")  # one more ordinary delta commit after the recovery
KEYS = ("v4", "lb4", "rec4", "v6", "lb6", "rec6")
TARGET = 101      # the rule the address deltas extend: the logged egress drop (more clients lose their remote Endpoints)


def _ip(v):
    return str(ipaddress.ip_address(int(v)))


def _ip6(v4):
    return str(ipaddress.IPv6Address(workload.v6_embed(int(v4))))


def anp_rule(fid, direction, action, frm, to, logging=False):
    out = direction == "Out"
    return {"direction": direction, "table": "AntreaPolicy%sRule" % ("Egress" if out else "Ingress"), "action": action,
            "flow_id": fid, "policy_type": "AntreaClusterNetworkPolicy", "policy_namespace": "",
            "policy_name": "cf-%d" % fid, "policy_uid": "uid-cf-%d" % fid, "name": "rule-%d" % fid, "tier_priority": 50,
            "priority": 64000 - fid, "service": None, "enable_logging": logging, "from": frm, "to": to}


def _dual(rules):
    w = workload.Workload("x")
    w.rules = rules
    return workload.to_ipv6(w, dual=True).rules


class World:
    """The rule and Service sets as installed: what the oracle is built from. Mutated together with
    the classifier by the helpers of Ctx."""

    def __init__(self, seed=SEED):
        wl = ac.make_workload(seed)
        self.cols = ac.make_batch(wl, N, seed, clients=48, established=0.3)
        self.cols6 = workload.service_packets_to_v6(self.cols)
        self.clients = [int(a) for a in self.cols["src"][:48]]
        self.remote = [{"ipnet": "10.128.0.0/9"}]  # the remote Endpoints (the policy stages see the DNATed packet)
        self.local = [{"ofport": int(p)} for p in wl.local_ports[:40]]
        logged = [anp_rule(101, "Out", "Drop", [_ip(self.clients[0])], self.remote, True),
                  anp_rule(102, "In", "Allow", [_ip(self.clients[1]), _ip(self.clients[2])], self.local, True)]
        self.rules = _dual(list(wl.rules) + logged)
        self.w4 = wl
        w6 = workload.services_to_ipv6(wl)
        w6.groups = {g + GID6: e for g, e in w6.groups.items()}
        w6.services = [dict(s, cluster_group_id=s["cluster_group_id"] + GID6, local_group_id=s["local_group_id"] + GID6)
                       for s in w6.services]
        w6.affinity_groups = {g + GID6 for g in w6.affinity_groups}
        self.w6 = w6

    def rule(self, fid):
        return next(r for r in self.rules if r["flow_id"] == fid)


_WORLD = []


def world():
    if not _WORLD:
        _WORLD.append(World())
    return copy.deepcopy(_WORLD[0])


class Oracle:
    """Both families' pipelines over the oracle compiler's NetworkPolicy flows and the realized Service
    text; their learned flows outlive refresh() as a switch's do."""

    def __init__(self):
        self.p4 = self.p6 = None

    def refresh(self, w, clf):
        fnp = oc.FeatureNetworkPolicy(ipv4=True, ipv6=True)
        fnp.initialize()
        fnp.batch_install_policy_rule_flows(copy.deepcopy(w.rules))
        self.ops = pin_model.ops_map(fnp)
        svc = [f for f in clf.dump_flows() if any(t in f for t in SVC_TABLES)]
        svc6 = [f for f in svc if svc6_model._is_v6_line(f)]
        svc4 = [f for f in svc if not svc6_model._is_v6_line(f)]
        groups = clf.dump_groups()
        groups4 = [g for g in groups if "->xxreg3" not in g]
        tiers = {r["flow_id"]: int(r.get("tier_priority") or 0) for r in w.rules}
        np_flows = fnp.dump_flows()
        a4 = (np_flows + svc4, tiers, groups4, w.w4.pods)
        a6 = (np_flows + svc6, tiers, groups, w.w6.pods)
        if self.p4 is None:
            self.p4, self.p6 = affinity_model.AffinityPipeline(*a4), affinity6_model.Affinity6Pipeline(*a6)
        else:
            self.p4.set_flows(*a4)
            self.p6.set_flows(*a6)

    def forget(self):  # gpc_replay: the tables are lost
        self.p4.learned, self.p6.learned = {}, {}

    def run(self, w):
        self.p4.now = NOW
        v4, lb4 = affinity_model.run(self.p4, w.cols)
        v6, lb6 = affinity6_model.run(self.p6, w.cols6, NOW)
        return {"v4": v4, "lb4": lb4, "rec4": pin_model.records(v4, self.ops), "v6": v6, "lb6": lb6,
                "rec6": pin_model.records(v6, self.ops)}


class EmuSlot:
    """The host emulation of one device slot: the context's own images, tables of its own."""

    def __init__(self):
        self.forget()

    def forget(self):
        self.t4, self.t6 = emu_aff.Table(LOG2), emu_aff6.Table6(LOG2)

    def skip(self):
        """A batch the slot classified on an epoch the host images have moved past: it cannot be
        emulated, and (see the module docstring) only advanced the tables' launch sequence."""
        for t in (self.t4, self.t6):
            if not t.fresh:
                t.seq += 1

    def run(self, clf, w, counters=None):
        n = len(w.cols["src"])
        lb4, lb6 = np.zeros(n, gpc.LB_DTYPE), np.zeros(n, gpc.LB6_DTYPE)
        v4 = self.t4.classify(clf, w.cols, NOW, counters, lb4)
        v6 = self.t6.classify6(clf, w.cols6, NOW, counters, lb6)
        return {"v4": v4, "lb4": lb4, "rec4": emu_pin.collect(clf, v4)[0], "v6": v6, "lb6": lb6,
                "rec6": emu_pin.collect(clf, v6)[0]}


def same(a, b, what):
    for k in KEYS:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.tobytes() != y.tobytes():
            n = min(len(x), len(y))
            bad = [i for i in range(n) if x[i].tobytes() != y[i].tobytes()][:3]
            raise AssertionError("%s: %s differs (%d vs %d entries) at %s: %s vs %s" % (
                what, k, len(x), len(y), bad, [x[i] for i in bad], [y[i] for i in bad]))


class HostSide:
    """No device: commits build the host images only and a batch is its emulation."""
    device = False

    def commit(self, ctx, how):
        emu.commit_host(ctx.c, full=how == "compact")

    def batch(self, ctx, slot, count):
        return None


class Ctx:
    def __init__(self, side):
        self.side, self.w = side, world()
        self.c = gpc.Classifier(ipv4=True, ipv6=True, devices=[0, 0], compact_after=-1, session_affinity=LOG2,
                                session_affinity6=LOG2)
        self.c.initialize()
        self.c.batch_install_policy_rule_flows(copy.deepcopy(self.w.rules))
        workload.install_services(self.c, self.w.w4)
        workload.install_services(self.c, self.w.w6)
        self.c.set_affinity_clock(NOW)
        self.emu = [EmuSlot(), EmuSlot()]
        self.released, self.pending_new = set(), set()
        self.totals = {}   # the counter model: conj -> [packets, bytes, sessions], summed over the slots

    def close(self):
        self.c.close()

    # --- changes: the classifier and the world together
    def add_addr(self, fid, side, addr):
        r = self.w.rule(fid)
        self.c.add_policy_rule_address(fid, side, [addr], r.get("priority"))
        r["from" if side == "src" else "to"].append(addr)

    def install(self, rule, dual=False):
        """rule: IPv4 addresses (mapped into both families here) unless it is `dual` already."""
        if not dual:
            rule, = _dual([rule])
        self.c.install_policy_rule_flows(copy.deepcopy(rule))
        self.w.rules.append(rule)
        self.pending_new.add(rule["flow_id"])

    def uninstall(self, fid):
        self.c.uninstall_policy_rule_flows(fid)
        self.w.rules = [r for r in self.w.rules if r["flow_id"] != fid]
        self.released.add(fid)
        self.pending_new.discard(fid)

    def set_group(self, gid, keep):
        """The Endpoints keep(list) of group gid, in both families."""
        for wl, g in ((self.w.w4, gid), (self.w.w6, gid + GID6)):
            wl.groups[g] = keep(wl.groups[g])
            self.c.install_service_group(g, wl.groups[g], g in wl.affinity_groups)

    # --- calls
    def call(self, how):
        """The call; on success the counter model and the emulation follow the publish."""
        if how == "replay":
            self.c.replay()
        else:
            self.side.commit(self, how)
        self.published(how == "replay")

    def published(self, replayed):
        if replayed:
            self.totals = {}
            for e in self.emu:
                e.forget()
        for fid in self.released:
            self.totals.pop(fid, None)
        self.released, self.pending_new = set(), set()

    def slots(self):
        return self.c.counters()[1]

    def batch(self, slot, count=False, emulate=True):
        """One batch of both families on a slot: the device's results (the emulation's on a host),
        checked against the emulation of the context's images when these are what the slot publishes."""
        got = self.side.batch(self, slot, count)
        if not emulate:
            self.emu[slot].skip()
            return got
        slots = self.slots()
        per = np.zeros((len(slots), 3), np.uint64) if count else None
        want = self.emu[slot].run(self.c, self.w, per)
        if got is None:
            got = want
        same(got, want, "slot %d against the emulation" % slot)
        if count:
            for s, conj in enumerate(slots):
                if conj and per[s].any():
                    t = self.totals.setdefault(conj, [0, 0, 0])
                    for j in range(3):
                        t[j] += int(per[s][j])
        return got

    def metrics(self):
        return {int(k): tuple(int(x) for x in v) for k, v in self.c.network_policy_metrics().items() if any(v)}

    def model_metrics(self):
        return {k: tuple(v) for k, v in self.totals.items() if any(v)}


# ------------------------------------------------------------------------------------ scenarios
def _net24(a):
    return {"ipnet": "%s/24" % _ip(int(a) & ~0xFF)}


def change_delta(ctx, i=20):
    """An address add on both families (the IPv4 one a block: a journaled rule, no point extension)."""
    for j in (i, i + 1):
        ctx.add_addr(TARGET, "src", _net24(ctx.w.clients[j]))
        ctx.add_addr(TARGET, "src", _ip6(ctx.w.clients[j]))


def small_change(ctx, i=30):
    ctx.add_addr(TARGET, "src", _ip(ctx.w.clients[i]))
    ctx.add_addr(TARGET, "src", _ip6(ctx.w.clients[i]))


def _affinity_group(w):
    """An IPv4 affinity group with several Endpoints that the batch reaches, and a plain one."""
    hit = set()
    for s in w.w4.services:
        gid = s["local_group_id"] if s["traffic_policy_local"] else s["cluster_group_id"]
        if len(w.w4.groups.get(gid, ())) >= 2 and not s.get("is_nodeport") and \
                (w.cols["dst"] == int(ipaddress.ip_address(s["ip"]))).sum() > 10:
            hit.add(gid)
    aff = sorted(g for g in hit if g in w.w4.affinity_groups)
    plain = sorted(g for g in hit if g not in w.w4.affinity_groups)
    assert aff and plain
    return aff[0], plain[0]


def _svc_change(ctx):
    """An Endpoint removed from an affinity Service, another Service left without Endpoints."""
    aff, plain = _affinity_group(ctx.w)
    ctx.set_group(aff, lambda eps: eps[1:])
    ctx.set_group(plain, lambda eps: [])


def _new_rules(ctx, fids, first_client):
    for j, fid in enumerate(fids):
        ctx.install(anp_rule(fid, "Out", "Allow" if j % 2 == 0 else "Drop", [_ip(ctx.w.clients[first_client + j])],
                             ctx.w.remote))


def _victims(ctx):
    """Two counted C1 rules with counts in the pre-state."""
    m = ctx.model_metrics()
    v = sorted(k for k in m if k < 100)[:2]
    assert len(v) == 2, m
    return v


def pre_state(scn, ctx, setenv):
    """The published epoch the scenario's change is pending over, then the batch once on every slot
    (the tables learn) and once counted."""
    if scn == "first":
        return
    ctx.call("commit")
    if scn in ("delta2", "replay"):
        change_delta(ctx, 22)
        ctx.call("commit")
    if scn == "pool_gc":  # versions of one rule: as many dead ones as 2 x the one live rule (the collection's bar)
        for i in range(3):
            ctx.add_addr(TARGET, "src", _net24(ctx.w.clients[12 + i]))
            ctx.call("commit")
        assert ctx.c.image_stats()["n_pool_collections"] == 0
    for count in (False, True):
        for slot in (0, 1):
            ctx.batch(slot, count)


def change(scn, ctx, setenv):
    """The pending change; returns the call that publishes it."""
    if scn == "delta":
        change_delta(ctx)
    elif scn == "delta2":
        change_delta(ctx, 26)
    elif scn == "v6prefix":  # a prefix length the IPv6 image has not seen, over every embedded client
        ctx.add_addr(TARGET, "src", {"ipnet": "fd00:10::/47"})
    elif scn == "compact":
        _svc_change(ctx)
        ctx.install(anp_rule(103, "Out", "Drop", [_ip(ctx.w.clients[3])], ctx.w.remote, True))
        _new_rules(ctx, (121, 122, 123, 124), 8)
        return "compact"
    elif scn == "svc_only":
        _svc_change(ctx)
    elif scn == "pin_only":  # the same rule without logging: the verdicts stay, its records go
        r = dict(copy.deepcopy(ctx.w.rule(TARGET)), enable_logging=False)
        ctx.uninstall(TARGET)
        ctx.install(r, dual=True)
        ctx.pending_new.discard(TARGET)
    elif scn == "reuse":
        for fid in _victims(ctx):
            ctx.uninstall(fid)
        _new_rules(ctx, (111, 112), 6)
    elif scn == "pool_gc":
        setenv("GPC_GC_DEAD_MIN", "1")
        ctx.add_addr(TARGET, "src", _net24(ctx.w.clients[15]))
    elif scn == "replay":
        return "replay"
    return "commit"


def recover(scn, way, how, ctx):
    """The recovery call of a way (also run, where it changes the final state, by the reference run)."""
    if way == "a":
        ctx.call(how)
    elif way == "b":
        small_change(ctx)
        ctx.call("commit")
    elif way == "c":
        ctx.call("commit")


def traces(ctx, slot):
    out = []
    for i in (0, 1, 2, 3, 4):
        v, steps, lb = ctx.c.trace({k: int(a[i]) for k, a in ctx.w.cols.items()}, slot=slot)
        v6, steps6, lb6, nets = ctx.c.trace6({k: (a[i] if a.ndim == 2 else int(a[i])) for k, a in ctx.w.cols6.items()},
                                             slot=slot)
        out.append((v.tobytes(), steps, lb.tobytes(), v6.tobytes(), steps6, lb6.tobytes(), str(nets)))
    return out


def refuses(ctx):
    """Every slot refuses to classify: nothing is published."""
    sub = {k: np.ascontiguousarray(a[:8]) for k, a in ctx.w.cols.items()}
    for slot in (0, 1):
        try:
            ctx.c.classify_host(sub, slot=slot)
        except gpc.GpcError as e:
            assert e.code == gpc.GPC_EINVAL, e
        else:
            raise AssertionError("slot %d classified with nothing published" % slot)
    try:
        ctx.c.classify6_host({k: np.ascontiguousarray(a[:8]) for k, a in ctx.w.cols6.items()})
    except gpc.GpcError as e:
        assert e.code == gpc.GPC_EINVAL, e
    else:
        raise AssertionError("IPv6 classified with nothing published")


def check_resident(ctx):
    """Host-side, and FIRST after a recovery, before any counted launch: every slot has a counter array
    that holds every slot of the published map, and the images the model calls for exist. (A context
    that published an epoch without counters fails here, on the host; a counted batch against it
    would make the kernel add through a null pointer.)"""
    n = ctx.c.image_stats()["n_counter_slots"]
    assert n >= 30
    for slot in (0, 1):
        cap, copies = ctx.c.debug_counter_layout(slot)
        assert cap >= n and copies >= 1, "slot %d: counter array of %d slots x %d copies for %d rules" % (slot, cap, copies, n)
    assert bool(ctx.c.debug_service_image()) == bool(ctx.w.w4.services), "IPv4 Service image"
    assert bool(ctx.c.debug_service_image6()) == bool(ctx.w.w6.services), "IPv6 Service image"
    logged = any(r.get("enable_logging") for r in ctx.w.rules)
    assert (ctx.c.debug_pin_image()[1] > 0) == logged, "packet-in image"


def final_checks(scn, ctx, oracle, ref):
    """After the (recovered) publish: layout first, then both slots counted against the emulation, the
    reference run (k is not None) or the oracle (the reference run itself), each other and the
    counter model; for the delta scenarios one more delta commit on top."""
    if ctx.side.device:
        check_resident(ctx)
    out = {}
    r = [ctx.batch(slot, count=True) for slot in (0, 1)]
    same(r[0], r[1], "slot 0 against slot 1")
    if oracle is not None:
        oracle.refresh(ctx.w, ctx.c)
        same(r[0], oracle.run(ctx.w), "against the oracle")
    else:
        same(r[0], ref["final"], "against the reference run")
    out["final"] = r[0]
    if ctx.side.device:
        assert ctx.metrics() == ctx.model_metrics()
        assert ctx.c.stream_epoch() == ctx.c.image_stats()["epoch"]
    if scn in FOLLOWED:
        small_change(ctx, 34)
        ctx.call("commit")
        r = [ctx.batch(slot) for slot in (0, 1)]
        same(r[0], r[1], "slot 0 against slot 1 after the follow-up delta")
        if oracle is not None:
            oracle.refresh(ctx.w, ctx.c)
            same(r[0], oracle.run(ctx.w), "follow-up delta against the oracle")
        else:
            same(r[0], ref["followup"], "follow-up delta against the reference run")
        out["followup"] = r[0]
    return out


def conditions(scn, ref_pre, ref):
    """The batch exercises what the scenario is about (asserted on the reference run, not assumed)."""
    f = ref["final"]
    for fam in ("4", "6"):
        lb = f["lb" + fam]["flags"]
        assert ((lb & gpc.LB_HIT) != 0).mean() > 0.3 and (lb & gpc.LB_NO_ENDPOINT).any() and (lb & gpc.LB_AFFINITY).any(), fam
        if scn != "pin_only":
            assert len(f["rec" + fam]) > 10, (fam, len(f["rec" + fam]))
    if ref_pre is None:
        return
    changed = [k for k in KEYS if np.ascontiguousarray(ref_pre[k]).tobytes() != np.ascontiguousarray(f[k]).tobytes()]
    if scn in ("delta", "delta2", "reuse", "pool_gc"):
        assert "v4" in changed, changed
    if scn in ("delta", "delta2", "v6prefix", "reuse"):
        assert "v6" in changed, changed
    if scn in ("compact", "svc_only"):
        assert "lb4" in changed and "lb6" in changed, changed
    if scn in ("compact", "pin_only"):
        assert "rec4" in changed and "rec6" in changed, changed
    if scn == "replay":  # the tables were lost: clients learn again
        for fam in ("4", "6"):
            assert not (ref_pre["lb" + fam]["flags"] & gpc.LB_LEARNED).any()
            assert (f["lb" + fam]["flags"] & gpc.LB_LEARNED).any()


def run_case(scn, way, side, env, k=None, ref=None):
    """See the module docstring; env: pytest's monkeypatch. Returns (points, results) for k None."""
    env.delenv("GPC_GC_DEAD_MIN", raising=False)
    setenv = env.setenv
    ctx = Ctx(side)
    try:
        oracle = Oracle() if k is None else None
        pre_state(scn, ctx, setenv)
        snap = None
        if scn != "first":
            snap = {"r": [ctx.batch(slot) for slot in (0, 1)], "m": ctx.metrics()}
            if side.device:
                snap.update(t=[traces(ctx, slot) for slot in (0, 1)], e=ctx.c.image_stats()["epoch"], se=ctx.c.stream_epoch())
            if oracle is not None:
                oracle.refresh(ctx.w, ctx.c)
                oracle.run(ctx.w)  # (the tables learn)
                same(snap["r"][0], oracle.run(ctx.w), "the pre-state against the oracle")
            if side.device:  # one counted batch on each slot
                assert snap["m"] == ctx.model_metrics() and all(x % 2 == 0 for v in snap["m"].values() for x in v)
        if k is not None:
            ctx.c.debug_fail_upload_at(k)
        how = change(scn, ctx, setenv)
        if k is None:
            if how == "replay":
                oracle.forget()
            ctx.call(how)
            points = ctx.c.debug_upload_points() if side.device else 0
            if scn == "pool_gc":
                assert ctx.c.image_stats()["n_pool_collections"] == 1
            if way == "b":
                recover(scn, way, how, ctx)
            out = final_checks(scn, ctx, oracle, None)
            conditions(scn, snap and snap["r"][0], out)
            return points, out
        try:
            ctx.call(how)
        except gpc.GpcError as e:
            assert e.code == gpc.GPC_EDEV, e
        else:
            raise AssertionError("point %d armed: the %s succeeded" % (k, how))
        assert ctx.c.debug_upload_points() == k + 1
        after_failure(scn, ctx, snap)
        recover(scn, way, how, ctx)
        final_checks(scn, ctx, None, ref)
        return None
    finally:
        ctx.close()


def after_failure(scn, ctx, snap):
    """What a failed call leaves: nothing published that was not, nothing lost that was."""
    if scn in ("first", "replay"):
        refuses(ctx)
        assert ctx.metrics() == {}
        for slot in (0, 1):
            assert ctx.c.debug_counter_layout(slot)[0] == 0
        ctx.totals = {}
        for e in ctx.emu:
            e.forget()
        return
    assert ctx.c.image_stats()["epoch"] == snap["e"]
    assert ctx.metrics() == snap["m"], "metrics after the failed call, before any further batch"
    for slot in (0, 1):
        same(ctx.batch(slot, emulate=False), snap["r"][slot], "slot %d after the failed call against its snapshot" % slot)
        assert traces(ctx, slot) == snap["t"][slot], "slot %d: traces after the failed call" % slot
    assert ctx.c.stream_epoch() == snap["se"] == snap["e"]
    # one more counted batch, on slot 0: exactly one batch's worth on the rules of the published epoch
    # (the snapshot holds one counted batch per slot), nothing on a rule that is only pending
    ctx.batch(0, count=True, emulate=False)
    m = ctx.metrics()
    assert m == {c: tuple(x + x // 2 for x in v) for c, v in snap["m"].items()}, "one batch's worth on the published epoch"
    assert not any(c in m for c in ctx.pending_new), (ctx.pending_new, m)
    ctx.totals = {c: list(v) for c, v in m.items()}
