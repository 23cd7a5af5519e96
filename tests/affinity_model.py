"""Test-side executor of session affinity (sessionAffinity: ClientIP of IPv4 Services). A subclass of
the oracle Pipeline that reads the *realized* flow and group text: the priority-190 learn flows of
ServiceLB (serviceLearnFlow, pipeline.go:2316-2371) are parsed here with one regex -- their
hard_timeout, match and loads -- and executed as OVS would: a dict of learned flows keyed as the
learned flow matches (nw_proto, tp_dst, nw_dst, nw_src), applied to a batch serially in caller order.
Everything after the Service stage (the NO_ENDPOINT reject, both policy stages) is the unmodified
oracle. The bucket choice is the oracle's lb_hash restatement (parity unpinned, as everywhere).

Per packet to a Service whose ServiceLB flow loads EpToLearnRegMark (reg4[16..18] = 3):
  1. a live learned flow (now < expires) whose Endpoint is still a bucket of the Service's group
     loads that Endpoint (a learned Endpoint that left the group counts as a miss: the documented
     divergence from OVS);
  2. else a +new packet takes the group's bucket, resubmits to ServiceLB, hits the learn flow, which
     adds (or replaces) the learned flow with hard_timeout;
  3. else the packet takes the bucket and learns nothing (documented: the stage has no conntrack).
Lines it cannot parse raise: nothing is skipped quietly."""
import ipaddress
import re

import numpy as np

from antrea_amd import gpc
from oracle import ovs_cls

EP_STATE_MASK, EP_TO_LEARN, EP_SELECTED, TO_NODE_PORT = 0x70000, 0x30000, 0x20000, 0x80000
_PROTO = {"tcp": 6, "udp": 17, "sctp": 132}
_LEARN = re.compile(
    r"cookie=0x([0-9a-f]+), table=ServiceLB, priority=190,(tcp|udp|sctp),reg4=0x([0-9a-f]+)/0x([0-9a-f]+)"
    r"(?:,nw_dst=([0-9.]+))?,tp_dst=(\d+) actions=learn\(table=SessionAffinity,hard_timeout=(\d+),priority=200,"
    r"delete_learned,cookie=0x([0-9a-f]+),eth_type=0x800,nw_proto=0x([0-9a-f]+),OXM_OF_(TCP|UDP|SCTP)_DST\[\],"
    r"NXM_OF_IP_DST\[\],NXM_OF_IP_SRC\[\],load:NXM_NX_REG4\[0\.\.15\]->NXM_NX_REG4\[0\.\.15\],"
    r"load:NXM_NX_REG4\[26\]->NXM_NX_REG4\[26\],load:NXM_NX_REG3\[\]->NXM_NX_REG3\[\],load:0x2->NXM_NX_REG4\[16\.\.18\],"
    r"load:0x1->NXM_NX_REG0\[9\](,load:0x1->NXM_NX_REG4\[21\])?\),set_field:0x20000/0x70000->reg4,goto_table:EndpointDNAT$")


def _apply(regs, acts):
    for a in acts:
        if a[0] == "set_reg":
            _, r, v, m = a
            m = 0xFFFFFFFF if m is None else m
            regs[r] = (regs.get(r, 0) & ~m) | (v & m)


class AffinityPipeline(ovs_cls.Pipeline):
    """`learned` survives set_flows (the table belongs to the switch, not to a flow bundle)."""

    def __init__(self, flow_lines, tiers=None, group_lines=None, pods=None):
        self.learned = {}  # (nw_proto, tp_dst, nw_dst, nw_src) -> {"reg3", "port", "expires", "cookie"}
        self.now = 0
        self.n_learned = self.n_hits = 0
        self.set_flows(flow_lines, tiers, group_lines, pods)

    def set_flows(self, flow_lines, tiers=None, group_lines=None, pods=None, reinstalled=()):
        """A new realized state. `reinstalled`: (protocol number, Service IP as int or None for a
        NodePort Service, port) of the Services installed again since the last state: their learn flow
        was replaced, which deletes what it learned (delete_learned). Learned flows whose learn flow
        is gone are deleted for the same reason."""
        rest = [l for l in flow_lines if "actions=learn(" not in l]
        super().__init__(rest, tiers, group_lines, pods)
        self.learn = []
        for l in flow_lines:
            if "actions=learn(" not in l:
                continue
            m = _LEARN.search(l)
            if not m or m.group(1) != m.group(8) or int(m.group(9), 16) != _PROTO[m.group(2)] or \
                    m.group(10).lower() != m.group(2):
                raise ValueError("unparsed learn flow: " + l)
            self.learn.append({"proto": _PROTO[m.group(2)], "r4v": int(m.group(3), 16), "r4m": int(m.group(4), 16),
                               "dst": int(ipaddress.ip_address(m.group(5))) if m.group(5) else None,
                               "port": int(m.group(6)), "timeout": int(m.group(7)), "cookie": int(m.group(8), 16)})
        gone = set(reinstalled)

        def keeps(key):
            proto, port, dst, _ = key
            return any(lf["proto"] == proto and lf["port"] == port and (proto, lf["dst"], port) not in gone and
                       (lf["dst"] == dst or (lf["dst"] is None and self._is_node_port_addr(dst))) for lf in self.learn)

        self.learned = {k: v for k, v in self.learned.items() if keeps(k)}

    def _is_node_port_addr(self, dst):
        st = {"regs": {4: 0}, "ct_label": 0, "conj_id": 0}
        m, _ = ovs_cls.classifier_lookup(self.tables.get("NodePortMark", []), {"dst": dst, "src": 0, "proto": 6}, st,
                                         allow_conj=False)
        return m is not None

    def live(self):
        """Live learned flows as sorted (src, dst, endpoint ip, endpoint port | REMOTE << 16, expires)."""
        return sorted((k[3], k[2], v["reg3"], v["port"] | ((gpc.LB_REMOTE << 16) if v["remote"] else 0), v["expires"])
                      for k, v in self.learned.items() if self.now < v["expires"])

    def service_stage(self, pkt, learn=True):
        if pkt["proto"] not in (6, 17, 132) or not self.tables.get("ServiceLB"):
            return pkt, 0, None
        st = {"regs": {4: ovs_cls.EP_TO_SELECT}, "ct_label": 0, "conj_id": 0}
        m, _ = ovs_cls.classifier_lookup(self.tables.get("NodePortMark", []), pkt, st, allow_conj=False)
        _apply(st["regs"], m["actions"] if m is not None else [])
        f, _ = ovs_cls.classifier_lookup(self.tables["ServiceLB"], pkt, st, allow_conj=False)
        if f is None:
            return pkt, 0, None
        p = dict(pkt)
        p.setdefault("ct_dst", pkt["dst"])
        flags = ovs_cls.LB_HIT
        _apply(st["regs"], f["actions"])
        gid = next(a[1] for a in f["actions"] if a[0] == "group")
        if 7 in st["regs"]:
            p["svc_group"] = st["regs"][7]
        res = {"group_id": gid, "endpoint_ip": 0, "endpoint_port": 0, "out_port": 0}
        g = self.groups.get(gid)
        if g is None or not g["buckets"]:
            return p, flags | ovs_cls.LB_NO_ENDPOINT, res
        affinity = (st["regs"][4] & EP_STATE_MASK) == EP_TO_LEARN
        own = ovs_cls.select_bucket(g["buckets"], pkt)
        noep_regs = {}
        _apply(noep_regs, own["actions"])
        if noep_regs.get(0, 0) & ovs_cls.SVC_NO_EP:
            return p, flags | ovs_cls.LB_NO_ENDPOINT, res
        bucket = own
        if affinity:
            key = (pkt["proto"], pkt.get("dport", 0), pkt["dst"], pkt["src"])
            e = self.learned.get(key)
            hit = None
            if e is not None and self.now < e["expires"]:
                for b in g["buckets"]:  # still an Endpoint of the Service?
                    r = {}
                    _apply(r, b["actions"])
                    if r.get(3) == e["reg3"] and (r.get(4, 0) & 0xFFFF) == e["port"]:
                        hit = b
                        break
            if hit is not None:
                bucket = hit
                flags |= gpc.LB_AFFINITY
                if learn:
                    self.n_hits += 1
            elif learn and (pkt.get("ct_state", ovs_cls.CT_NEW | ovs_cls.CT_TRK) & ovs_cls.CT_NEW):
                if not any(a == ("goto_table", "ServiceLB") for a in own["actions"]):
                    raise ValueError("affinity Service whose bucket does not resubmit to ServiceLB: group %d" % gid)
                _apply(st["regs"], own["actions"])
                lf = [l for l in self.learn if l["proto"] == pkt["proto"] and l["port"] == pkt.get("dport", 0) and
                      (st["regs"][4] & l["r4m"]) == l["r4v"] and (l["dst"] is None or l["dst"] == pkt["dst"])]
                if len(lf) != 1:
                    raise ValueError("no learn flow for an EpToLearn packet: %r" % (key,))
                self.learned[key] = {"reg3": st["regs"].get(3, 0), "port": st["regs"][4] & 0xFFFF,
                                     "remote": bool(st["regs"][4] & ovs_cls.REMOTE_EP),
                                     "expires": self.now + lf[0]["timeout"], "cookie": lf[0]["cookie"]}
                flags |= gpc.LB_AFFINITY | gpc.LB_LEARNED
                self.n_learned += 1
        _apply(st["regs"], bucket["actions"])
        st["regs"][4] = (st["regs"][4] & ~EP_STATE_MASK) | EP_SELECTED  # the learn flow's / learned flow's load
        if st["regs"].get(4, 0) & ovs_cls.REMOTE_EP:
            flags |= ovs_cls.LB_REMOTE
        ep_ip, ep_port = st["regs"].get(3, 0), st["regs"].get(4, 0) & 0xFFFF
        res.update(endpoint_ip=ep_ip, endpoint_port=ep_port)
        d, _ = ovs_cls.classifier_lookup(self.tables.get("EndpointDNAT", []), pkt, st, allow_conj=False)
        if d is not None:
            for a in d["actions"]:
                if a[0] == "ct_commit" and len(a) > 3 and a[3] is not None:
                    p["dst"], p["dport"] = a[3]
                    flags |= ovs_cls.LB_DNAT
        if ep_ip in self.pods:
            p["out_port"], p["dest"] = self.pods[ep_ip], ovs_cls.DEST_POD
        else:
            p["out_port"], p["dest"] = 0, ovs_cls.DEST_TUNNEL if flags & ovs_cls.LB_REMOTE else ovs_cls.DEST_GATEWAY
        res["out_port"] = p["out_port"]
        return p, flags, res


def run(pipe, cols, n=None):
    """The batch through `pipe` serially in caller order at pipe.now: (verdicts (n, 2), lb (n,) LB_DTYPE)."""
    n = len(cols["src"]) if n is None else n
    out = np.zeros((n, 2), dtype=gpc.VERDICT_DTYPE)
    lb = np.zeros(n, dtype=gpc.LB_DTYPE)
    for i in range(n):
        rec = []
        e, g = pipe.classify({k: int(v[i]) for k, v in cols.items()}, lb=rec)
        for j, v in enumerate((e, g)):
            out[i, j] = (v[1], v[0], v[2], v[3], v[4])
        flags, r = rec[0]
        if flags:
            lb[i] = (r["endpoint_ip"], r["endpoint_port"], flags, 0, r["group_id"], r["out_port"])
    return out, lb
