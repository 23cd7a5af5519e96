"""Shared by tests/test_packet_in.py (host emulation) and tests/test_gpu_packet_in.py (device): a small
rule set and one batch of 3 * PIN_TILE + 5 packets whose packet-in queue holds every kind of record,
with the expectation computed by tests/packet_in_model.py from the oracle alone.

Rules (hand-written, a few dozen flows): AntreaClusterNetworkPolicy rules of Pod 0 (egress, by
destination /16) and Pod 1 (ingress, by source /16) -- Allow + logging, Drop + logging, Reject,
Reject + logging, plain Allow, plain Drop, Pass + logging, in both directions; one more logged
ingress Allow for Pod 0's own address, so that one packet is logged in both stages; a K8s
NetworkPolicy that isolates Pod 2 (default-drop flows); the DNS conjunction for Pod 3; a Service
without Endpoints and one with a local Endpoint. Variants: "plain", "deny_tracking"
(gpc_config.enable_deny_tracking: every ACNP Drop / Reject stores the deny) and "quiet" (no rule logs
or rejects, no DNS, no Service: no packet-in flow at all).

check_conditions() states on the expectation alone that the batch exercises what it is meant to:
it is a condition on the cases, not on the product."""
import copy
import ipaddress

import numpy as np

from antrea_amd import gpc, workload
from oracle import compiler as oc
from oracle import ovs_cls
from oracle import service as osvc
from tests import packet_in_model as model
from tests import svc6_model

T = gpc.PIN_TILE
N = 3 * T + 5
SIZES = (1, 63, 64, 65, T - 1, T, T + 1, N)
VARIANTS = ("plain", "deny_tracking", "quiet")
DNS_CONJ = 9000
POD = lambda i: int(ipaddress.ip_address("10.0.0.1")) + i  # Pod i: address, ofport 3 + i
OFPORT = lambda i: 3 + i
SVC_NOEP = {"ip": "10.96.0.10", "port": 80, "protocol": "TCP", "cluster_group_id": 1, "local_group_id": 2,
            "traffic_policy_local": False}
SVC_EP = {"ip": "10.96.0.11", "port": 80, "protocol": "TCP", "cluster_group_id": 3, "local_group_id": 4,
          "traffic_policy_local": False}
EP = {"ip": "10.0.0.5", "port": 8080, "is_local": True, "node_name": "node0"}
# (kind, action, logging): rule k of a direction matches the /16 number k + 1
KINDS = (("allow_log", "Allow", True), ("drop_log", "Drop", True), ("reject", "Reject", False),
         ("reject_log", "Reject", True), ("allow", "Allow", False), ("drop", "Drop", False), ("pass_log", "Pass", True))
EGRESS_NET, INGRESS_NET = 20, 30  # 20.k.0.0/16 destinations, 30.k.0.0/16 sources
FID = {}  # "e_<kind>" / "i_<kind>" / "i_self" / "iso" -> flow id


def _ip(v):
    return str(ipaddress.ip_address(int(v)))


def make_rules(variant="plain"):
    quiet = variant == "quiet"
    rules = []
    for d, (direction, net, base) in enumerate((("Out", EGRESS_NET, 100), ("In", INGRESS_NET, 200))):
        for k, (kind, action, logging) in enumerate(KINDS):
            if quiet and (logging or action == "Reject"):
                action, logging = ("Pass" if action == "Pass" else "Allow"), False
            fid = base + k + 1
            FID[("e_" if direction == "Out" else "i_") + kind] = fid
            r = {"direction": direction, "table": "AntreaPolicy%sRule" % ("Egress" if direction == "Out" else "Ingress"),
                 "action": action, "flow_id": fid, "policy_type": "AntreaClusterNetworkPolicy", "policy_namespace": "",
                 "policy_name": "pin-%s" % direction, "policy_uid": "uid-pin-%s" % direction, "name": "rule-%d" % k,
                 "tier_priority": 50, "priority": 64000 - 10 * k - d, "service": None, "enable_logging": logging}
            peer = [{"ipnet": "%d.%d.0.0/16" % (net, k + 1)}]
            if direction == "Out":
                r["from"], r["to"] = [_ip(POD(0))], peer
            else:
                r["from"], r["to"] = peer, [{"ofport": OFPORT(1)}]
            rules.append(r)
    FID["i_self"] = 210  # Pod 0 -> Pod 1, logged: with e_allow_log a packet logged in both stages
    rules.append({"direction": "In", "table": "AntreaPolicyIngressRule", "action": "Allow", "flow_id": 210,
                  "policy_type": "AntreaClusterNetworkPolicy", "policy_namespace": "", "policy_name": "pin-In",
                  "policy_uid": "uid-pin-In", "name": "rule-self", "tier_priority": 50, "priority": 64100, "service": None,
                  "enable_logging": not quiet, "from": [_ip(POD(0))], "to": [{"ofport": OFPORT(1)}]})
    FID["iso"] = 301  # K8s NetworkPolicy of Pod 2: everything but 40.0.0.1 falls to its default-drop flow
    rules.append({"direction": "Out", "table": "EgressRule", "flow_id": 301, "policy_type": "K8sNetworkPolicy",
                  "policy_namespace": "ns", "policy_name": "iso", "policy_uid": "uid-iso", "name": "rule0",
                  "from": [_ip(POD(2))], "to": ["40.0.0.1"], "service": None})
    return rules


def make_workload(variant="plain"):
    wl = workload.Workload("pin-" + variant)
    wl.rules = make_rules(variant)
    wl.local_ips = np.array([POD(i) for i in range(8)], np.uint32)
    wl.local_ports = np.array([OFPORT(i) for i in range(8)], np.uint32)
    wl.pods = {POD(i): OFPORT(i) for i in range(8)}
    wl.services, wl.groups, wl.endpoint_flows = [], {}, []
    if variant != "quiet":
        wl.services = [dict(SVC_NOEP), dict(SVC_EP)]
        wl.groups = {1: [], 3: [dict(EP)]}
        wl.endpoint_flows = [("TCP", [dict(EP)])]
    wl.svc_meta, wl.svc_frac = {}, 0.0
    wl.dns = [] if variant == "quiet" else [_ip(POD(3))]
    return wl


def make_batch(n=N, seed=5):
    """The batch: its first wave has no record, its second one in every packet, then one packet of
    every kind, records on both sides of every tile boundary and at the batch's end, and a random
    sprinkle of all kinds over the rest."""
    rng = np.random.default_rng(seed)
    c = {"src": (0x3C000000 + rng.integers(1, 1 << 16, N)).astype(np.uint32),   # 60.0.x.x -> 61.0.x.x: no rule
         "dst": (0x3D000000 + rng.integers(1, 1 << 16, N)).astype(np.uint32),
         "sport": rng.integers(1024, 65536, N).astype(np.uint16), "dport": rng.integers(1024, 65536, N).astype(np.uint16),
         "proto": np.full(N, 6, np.uint8), "out_port": np.full(N, OFPORT(6), np.uint32),
         "ct_state": np.full(N, 0x21, np.uint8), "len": rng.integers(64, 1500, N).astype(np.uint16)}
    host = lambda: int(rng.integers(1, 1 << 16))

    def egress(i, k):
        c["src"][i], c["dst"][i] = POD(0), (EGRESS_NET << 24) | ((k + 1) << 16) | host()

    def ingress(i, k):
        c["src"][i], c["out_port"][i] = (INGRESS_NET << 24) | ((k + 1) << 16) | host(), OFPORT(1)

    def both(i):  # e_allow_log, then i_self
        egress(i, 0)
        c["out_port"][i] = OFPORT(1)

    def dns(i):
        c["dst"][i], c["out_port"][i], c["proto"][i], c["sport"][i], c["ct_state"][i] = POD(3), OFPORT(3), 17, 53, 0x28

    def svc(i, cfg):
        c["dst"][i], c["dport"][i] = int(ipaddress.ip_address(cfg["ip"])), cfg["port"]

    def iso(i):
        c["src"][i] = POD(2)

    kinds = [lambda i, k=k: egress(i, k) for k in range(7)] + [lambda i, k=k: ingress(i, k) for k in range(7)] + \
            [both, dns, lambda i: svc(i, SVC_NOEP), lambda i: svc(i, SVC_EP), iso]
    for i in range(64, 128):
        egress(i, 0)
    for j, f in enumerate(kinds):
        f(130 + 2 * j)
    for t in (T, 2 * T, 3 * T):
        both(t - 1)
        ingress(t, 1)
    both(N - 2)
    egress(N - 1, 3)
    free = np.array([i for i in range(256, N - 2) if min(abs(i - t) for t in (T, 2 * T, 3 * T)) > 1])
    for i in rng.choice(free, size=len(free) // 8, replace=False):
        kinds[int(rng.integers(len(kinds)))](int(i))
    return {k: v[:n].copy() for k, v in c.items()}


def to_v6(cols):
    return workload.service_packets_to_v6(cols)


def install(side_np, wl, dns=True):
    side_np.batch_install_policy_rule_flows(copy.deepcopy(wl.rules))
    if dns and wl.dns:
        side_np.new_dns_packet_in_conjunction(DNS_CONJ)
        side_np.add_address_to_dns_conjunction(DNS_CONJ, list(wl.dns))


def make_product(variant="plain", v6=False, **kw):
    """(classifier -- not committed yet, workload as installed)."""
    wl = make_workload(variant)
    if v6:
        dns = wl.dns
        wl = workload.services_to_ipv6(wl)
        wl.dns = [workload._v6_addr(a) for a in dns]
    c = gpc.Classifier(ipv4=True, ipv6=v6, enable_deny_tracking=variant == "deny_tracking", **kw)
    c.initialize()
    install(c, wl)
    if wl.services:
        workload.install_services(c, wl)
    return c, wl


class Oracle:
    """The oracle side of one variant: compiler state, {conj id: ops}, pipeline."""

    def __init__(self, wl, variant="plain", v6=False, clf=None):
        self.wl, self.v6 = wl, v6
        self.fnp = oc.FeatureNetworkPolicy(ipv4=True, ipv6=v6, enable_deny_tracking=variant == "deny_tracking")
        self.fnp.initialize()
        install(self.fnp, wl)
        self.clf = clf
        self.tiers = {r["flow_id"]: int(r.get("tier_priority") or 0) for r in wl.rules}
        self.refresh()

    def install(self, rule):
        """A rule installed after the first commit (the caller installs it in the product)."""
        self.fnp.install_policy_rule_flows(copy.deepcopy(rule))
        self.tiers[rule["flow_id"]] = int(rule.get("tier_priority") or 0)

    def refresh(self):
        tiers = self.tiers
        self.ops = model.ops_map(self.fnp)
        if self.v6:  # (the oracle restates no IPv6 Service flows: the realized text, walked by tests/svc6_model.py)
            svc_flows = [f for f in self.clf.dump_flows() if any("table=%s," % t in f for t in svc6_model.SVC_TABLES)]
            self.pipe = svc6_model.Pipeline6(self.fnp.dump_flows() + svc_flows, tiers, self.clf.dump_groups(), self.wl.pods)
        else:
            svc = osvc.FeatureService()
            if self.wl.services:
                osvc.install_services(svc, self.wl)
            self.pipe = ovs_cls.Pipeline(self.fnp.dump_flows() + svc.dump_flows(), tiers, svc.dump_groups(), self.wl.pods)

    def expect(self, cols):
        """(verdicts (n, 2), records) of a batch."""
        v = model.verdicts(self.pipe, cols, self.v6)
        return v, model.records(v, self.ops)


def check_conditions(variant, v, recs):
    """On the oracle-derived expectation of the whole batch alone."""
    n = len(v)
    assert n == N
    per_pkt = np.bincount(recs["index"], minlength=n) if len(recs) else np.zeros(n, int)
    if variant == "quiet":
        assert len(recs) == 0
        return
    np_ = recs[recs["category"] == model.CAT_NP]
    has = lambda m: bool(m.any())
    if variant == "plain":
        assert has((np_["disposition"] == 0) & (np_["operations"] == model.OP_LOGGING))
        assert has((np_["disposition"] == 1) & (np_["operations"] == model.OP_LOGGING))
        assert has((np_["operations"] & model.OP_REJECT) != 0) and has(np_["operations"] == model.OP_REJECT | model.OP_LOGGING)
        assert not has((np_["operations"] & model.OP_STORE_DENY) != 0)
    else:
        assert has(np_["operations"] == model.OP_STORE_DENY), "STORE_DENY without logging"
        assert has(np_["operations"] == model.OP_STORE_DENY | model.OP_REJECT)
    assert has(recs["category"] == model.CAT_DNS) and has(recs["category"] == model.CAT_SVC_REJECT)
    assert has(np_["stage"] == 0) and has(np_["stage"] == 1) and set(np_["table"]) == {1, 4}
    assert (per_pkt == 2).sum() >= 4 and per_pkt.max() == 2
    waves = per_pkt[:n - n % 64].reshape(-1, 64)
    assert (waves.sum(axis=1) == 0).any() and (waves > 0).all(axis=1).any()
    for t in (T, 2 * T, 3 * T):
        assert per_pkt[t - 1] and per_pkt[t], "records on both sides of a tile boundary"
    assert per_pkt[n - 1], "the last packet of the partial tile has a record"
    iso = v[:, 0]["action"] == ovs_cls.ACT_ISOLATION_DROP
    passed = ((v[:, 0]["flags"] | v[:, 1]["flags"]) & ovs_cls.FLAG_PASS) != 0
    assert iso.any() and not per_pkt[iso].any()
    assert passed.any() and not per_pkt[passed].any()
    # (a packet DNATed by the Service with an Endpoint gives nothing either)
    assert len(recs) > n // 16
