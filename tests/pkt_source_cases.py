"""Shared by tests/test_pkt_source.py (host emulation) and tests/test_gpu_pkt_source.py (device): the
packet-source workload (external Services with externalTrafficPolicy: Local beside the other shapes),
its batches with a `source` column, and the model over the product's realized text
(tests/svc_source_model.py). A "side" is a function (columns, clock) -> (verdicts, lb results).

The workload is C1 + 40 Services of 4 Endpoints: 60 % short-circuit (LoadBalancer IPs and NodePort
Services; their Local group holds the local Endpoints, so about a quarter of them has an empty Local
group under a Cluster group with Endpoints, and the Services drawn without Endpoints have both
empty), 30 % NodePort, optionally half with session affinity. IPv6: the same under the /96
embedding (workload.services_to_ipv6)."""
import copy
import ipaddress

import numpy as np

from antrea_amd import gpc, workload
from oracle import compiler as oc
from tests import emu, emu_aff, emu_aff6, emu_src, svc_source_model
from tests.test_emu_parity import _cmp

T, T0, LOG2 = 100, 1000, 12
SVC_TABLES = ("table=ServiceLB", "table=EndpointDNAT", "table=NodePortMark")
# every gpc_source value, plus two that are none of them (not local)
SOURCES = (gpc.SOURCE_UNKNOWN, gpc.SOURCE_TUNNEL, gpc.SOURCE_GATEWAY, gpc.SOURCE_POD, gpc.SOURCE_UPLINK, gpc.SOURCE_BRIDGE,
           gpc.SOURCE_TC_RETURN, 7, 255)
SC = gpc.LB_SHORT_CIRCUIT


def make_workload(seed, affinity=False, short_circuit_frac=0.6):
    """(IPv4 workload, its IPv6 image)."""
    wl = workload.add_services(workload.config1(seed=seed), 40, 4, seed=seed, noep_frac=0.15, local_policy_frac=0.2,
                               nodeport_frac=0.3, affinity_frac=0.5 if affinity else 0.0, affinity_timeout=T,
                               short_circuit_frac=short_circuit_frac)
    return wl, workload.services_to_ipv6(wl)


def make_product(w, family=4, affinity=False, packet_source=1, install=True, **kw):
    """A context over workload `w` (the IPv4 workload for family 4, the IPv6 one for family 6)."""
    aff = {"session_affinity6" if family == 6 else "session_affinity": LOG2} if affinity else {}
    c = gpc.Classifier(ipv4=True, ipv6=family == 6, packet_source=packet_source, **aff, **kw)
    c.initialize()
    c.batch_install_policy_rule_flows(copy.deepcopy(w.rules))
    if install:
        workload.install_services(c, w)
    return c


def make_batch(wl, n, seed, family=4, clients=12, established=0.0, source=True):
    """n packets of the IPv4 workload, most to a Service, from `clients` source addresses (keys repeat
    inside a batch), with a `source` column over SOURCES (source=False: the NULL column); family 6:
    the same packets in IPv6."""
    frac, wl.svc_frac = wl.svc_frac, 0.85
    cols = workload.gen_packets(wl, n, seed=seed)
    wl.svc_frac = frac
    rng = np.random.default_rng(seed + 1)
    pool = cols["src"][:clients].copy()
    cols["src"] = pool[rng.integers(0, min(clients, n), size=n)].astype(np.uint32)
    cols["source"] = np.array(SOURCES, np.uint8)[rng.integers(0, len(SOURCES), size=n)]
    if not source:
        del cols["source"]
    if established > 0:
        cols["ct_state"] = np.where(rng.random(n) < established, 0x02 | 0x20, 0x01 | 0x20).astype(np.uint8)
    return workload.service_packets_to_v6(cols) if family == 6 else cols


def take(cols, idx):
    return {k: np.ascontiguousarray(v[idx]) for k, v in cols.items()}


class Model:
    """The model over the product's realized Service text and the oracle compiler's NP flows."""

    def __init__(self, w, clf, family=4):
        self.w, self.family = w, family
        self.rules = copy.deepcopy(w.rules)
        self.pipe = None
        self.refresh(clf)

    def refresh(self, clf, reinstalled=()):
        fnp = oc.FeatureNetworkPolicy(ipv4=True, ipv6=True) if self.family == 6 else oc.FeatureNetworkPolicy()
        fnp.initialize()
        fnp.batch_install_policy_rule_flows(copy.deepcopy(self.rules))
        svc_flows = [f for f in clf.dump_flows() if any(t in f for t in SVC_TABLES)]
        tiers = {r["flow_id"]: int(r.get("tier_priority") or 0) for r in self.rules}
        args = (fnp.dump_flows() + svc_flows, tiers, clf.dump_groups(), self.w.pods)
        if self.pipe is None:
            self.pipe = svc_source_model.SourcePipeline(*args, family=self.family)
        else:
            self.pipe.set_flows(*args, reinstalled=reinstalled)

    def run(self, cols, now=T0, learn=True):
        self.pipe.now = now
        return svc_source_model.run(self.pipe, cols, learn=learn)


class Emulation:
    """The host emulation side of a context (tests/emu_src.py), with the affinity table of its family
    when the context has one."""

    def __init__(self, clf, family=4, affinity=False):
        self.clf, self.family = clf, family
        self.table = None
        if affinity:
            self.table = emu_aff6.Table6(LOG2) if family == 6 else emu_aff.Table(LOG2)

    def run(self, cols, now=T0):
        n = len(cols["dst6" if self.family == 6 else "dst"])
        lb = np.zeros(n, gpc.LB6_DTYPE if self.family == 6 else gpc.LB_DTYPE)
        fn = emu_src.classify6 if self.family == 6 else emu_src.classify
        return fn(self.clf, cols, table=self.table, now=now, lb=lb), lb

    def live(self, now):
        """Live entries as sorted (client, Endpoint, Endpoint port | REMOTE << 16, expires)."""
        return sorted((e[0],) + tuple(e[2:]) for e in self.table.live(now))


def device_side(clf, family=4):
    def run(cols, now=T0):
        clf.set_affinity_clock(now)
        return clf.classify6_host(cols, lb=True) if family == 6 else clf.classify_host(cols, lb=True)
    return run


def device_live(clf, family=4):
    """The device table's live entries in the shape of Emulation.live / model_live."""
    if family == 6:
        big = lambda a: int.from_bytes(bytes(a), "big")
        return sorted((big(e["src"]), big(e["endpoint_ip"]), int(e["endpoint_port"]), int(e["expires"]))
                      for e in clf.affinity_table6())
    return sorted((int(e["src"]), int(e["endpoint_ip"]), int(e["endpoint_port"]), int(e["expires"]))
                  for e in clf.affinity_table())


def model_live(model):
    return sorted((e[0],) + tuple(e[2:]) for e in model.pipe.live())


def check(name, cols, got, want):
    """Verdicts and LB results (every flag bit, GPC_LB_SHORT_CIRCUIT included): exact."""
    v, lb = got
    wv, wlb = want
    view = {k: c for k, c in cols.items() if c.ndim == 1}
    _cmp(v, wv, view)
    bad = np.nonzero(lb != wlb)[0]
    assert len(bad) == 0, (name, bad[:5], lb[bad[:3]], wlb[bad[:3]], {k: c[bad[:3]] for k, c in view.items()})


def coverage(cols, lb, affinity=False):
    """The batch reaches what the cases are about: a local and a non-local source at a short-circuit
    Service, the reject of external packets under a served local one, and every source value."""
    f = lb["flags"]
    src = cols["source"]
    local = np.isin(src, (gpc.SOURCE_GATEWAY, gpc.SOURCE_POD))
    hit = (f & gpc.LB_HIT) != 0
    assert set(src.tolist()) == set(SOURCES)
    assert ((f & SC) != 0).any() and not ((f & SC) != 0)[~local].any()
    assert (hit & local & ((f & SC) == 0)).any(), "a local source at a Service without a short-circuit flow"
    groups_sc = set(lb["group_id"][(f & SC) != 0].tolist())
    rejected = hit & ~local & ((f & gpc.LB_NO_ENDPOINT) != 0)
    served = (f & SC) != 0
    served &= (f & gpc.LB_NO_ENDPOINT) == 0
    # Local group empty, Cluster group not: cluster gid = local gid - 1 (workload.add_services)
    assert set((lb["group_id"][rejected] - 1).tolist()) & set(lb["group_id"][served].tolist()), "Local empty, Cluster served"
    assert (((f & SC) != 0) & ((f & gpc.LB_NO_ENDPOINT) != 0)).any(), "both groups empty"
    assert groups_sc
    if affinity:
        assert ((f & gpc.LB_LEARNED) != 0).any() and ((f & (gpc.LB_AFFINITY | gpc.LB_LEARNED)) == gpc.LB_AFFINITY).any()
        assert ((f & SC) != 0)[(f & gpc.LB_AFFINITY) != 0].any()


def remote_affinity_case(w, family):
    """An affinity short-circuit Service whose Cluster group holds a remote Endpoint that its non-empty
    Local group lacks, and a client for which a Pod-source packet picks that Endpoint: (Service config,
    packet dict without `source`)."""
    for s in w.services:
        if not (s.get("affinity_timeout") and s.get("is_external") and s.get("traffic_policy_local")):
            continue
        if s.get("is_nodeport"):
            continue
        ceps, leps = w.groups[s["cluster_group_id"]], w.groups[s["local_group_id"]]
        if leps and any(not e["is_local"] for e in ceps):
            return s
    raise AssertionError("the workload holds no such Service")


def one_packet(s, family, src, sport, source, ct_new=True):
    """One packet to Service `s` as one-row columns."""
    proto = dict(workload.SVC_PROTOS)[s["protocol"]]
    cols = {"sport": np.array([sport], np.uint16), "dport": np.array([s["port"]], np.uint16),
            "proto": np.array([proto], np.uint8), "out_port": np.array([0], np.uint32),
            "source": np.array([source], np.uint8),
            "ct_state": np.array([(0x01 if ct_new else 0x02) | 0x20], np.uint8)}
    if family == 6:
        cols["src6"] = np.frombuffer(ipaddress.ip_address(src).packed, np.uint8).reshape(1, 16).copy()
        cols["dst6"] = np.frombuffer(ipaddress.ip_address(s["ip"]).packed, np.uint8).reshape(1, 16).copy()
    else:
        cols["src"] = np.array([int(ipaddress.ip_address(src))], np.uint32)
        cols["dst"] = np.array([int(ipaddress.ip_address(s["ip"]))], np.uint32)
    return cols


def concat(*batches):
    return {k: np.ascontiguousarray(np.concatenate([b[k] for b in batches])) for k in batches[0]}
