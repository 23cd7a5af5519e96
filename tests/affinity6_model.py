"""Test-side executor of session affinity of IPv6 Services. A subclass of the IPv6 Service executor
(tests/svc6_model.py Pipeline6) that reads the *realized* text: the priority-190 IPv6 learn flows of
ServiceLB (serviceLearnFlow, pipeline.go:2316-2371) are parsed here with one strict regex and
executed as OVS would: a dict of learned flows keyed as the learned flow matches (nw_proto, tp_dst,
ipv6_dst, ipv6_src), hard timeout, applied to a batch serially in caller order; delete_learned on a
reinstall. The rules per packet are those of tests/affinity_model.py. Lines it cannot parse raise.

`blocked`: keys the side under test cannot learn because their claim digest collides with another
key's (tests narrow the digest; the model has no table): a +new packet of such a key that would
learn takes its own choice, carries neither affinity flag and is counted in n_overflow."""
import ipaddress
import re

import numpy as np

from antrea_amd import gpc
from oracle import ovs_cls
from tests import svc6_model
from tests.svc6_model import _apply, fold

EP_STATE_MASK, EP_TO_LEARN, EP_SELECTED = 0x70000, 0x30000, 0x20000
_PROTO = {"tcp6": 6, "udp6": 17, "sctp6": 132}
_LEARN = re.compile(
    r"cookie=0x([0-9a-f]+), table=ServiceLB, priority=190,(tcp6|udp6|sctp6),reg4=0x([0-9a-f]+)/0x([0-9a-f]+)"
    r"(?:,ipv6_dst=([0-9a-f:]+))?,tp_dst=(\d+) actions=learn\(table=SessionAffinity,hard_timeout=(\d+),priority=200,"
    r"delete_learned,cookie=0x([0-9a-f]+),eth_type=0x86dd,nw_proto=0x([0-9a-f]+),OXM_OF_(TCP|UDP|SCTP)_DST\[\],"
    r"NXM_NX_IPV6_DST\[\],NXM_NX_IPV6_SRC\[\],load:NXM_NX_REG4\[0\.\.15\]->NXM_NX_REG4\[0\.\.15\],"
    r"load:NXM_NX_REG4\[26\]->NXM_NX_REG4\[26\],load:NXM_NX_XXREG3\[\]->NXM_NX_XXREG3\[\],load:0x2->NXM_NX_REG4\[16\.\.18\],"
    r"load:0x1->NXM_NX_REG0\[9\](,load:0x1->NXM_NX_REG4\[21\])?\),set_field:0x20000/0x70000->reg4,goto_table:EndpointDNAT$")


class Affinity6Pipeline(svc6_model.Pipeline6):
    """`learned` survives set_flows (the table belongs to the switch, not to a flow bundle)."""

    def __init__(self, flow_lines, tiers=None, group_lines=None, pods=None):
        self.learned = {}  # (nw_proto, tp_dst, ipv6_dst, ipv6_src) -> {"xx", "port", "remote", "expires", "cookie"}
        self.now = 0
        self.n_learned = self.n_hits = self.n_overflow = 0
        self.blocked = set()
        self.set_flows(flow_lines, tiers, group_lines, pods)

    def set_flows(self, flow_lines, tiers=None, group_lines=None, pods=None, reinstalled=()):
        """A new realized state. `reinstalled`: (protocol number, Service address as int or None for a
        NodePort Service, port) of the Services installed again since the last state (delete_learned).
        Learned flows whose learn flow is gone are deleted for the same reason."""
        rest = [l for l in flow_lines if "actions=learn(" not in l]
        svc6_model.Pipeline6.__init__(self, rest, tiers, group_lines, pods)
        self.learn = []
        for l in flow_lines:
            if "actions=learn(" not in l or ",nw_dst=" in l or "eth_type=0x800," in l:  # (IPv4 learn flows: not ours)
                continue
            m = _LEARN.search(l)
            if not m or m.group(1) != m.group(8) or int(m.group(9), 16) != _PROTO[m.group(2)] or \
                    m.group(10).lower() + "6" != m.group(2):
                raise ValueError("unparsed IPv6 learn flow: " + l)
            self.learn.append({"proto": _PROTO[m.group(2)], "r4v": int(m.group(3), 16), "r4m": int(m.group(4), 16),
                               "dst": int(ipaddress.IPv6Address(m.group(5))) if m.group(5) else None,
                               "port": int(m.group(6)), "timeout": int(m.group(7)), "cookie": int(m.group(8), 16)})
        gone = set(reinstalled)

        def keeps(key):
            proto, port, dst, _ = key
            return any(lf["proto"] == proto and lf["port"] == port and (proto, lf["dst"], port) not in gone and
                       (lf["dst"] == dst or (lf["dst"] is None and dst in self.np_addrs)) for lf in self.learn)

        self.learned = {k: v for k, v in self.learned.items() if keeps(k)}

    def live(self):
        """Live learned flows as sorted (src, dst, endpoint address, endpoint port | REMOTE << 16, expires)."""
        return sorted((k[3], k[2], v["xx"], v["port"] | ((gpc.LB_REMOTE << 16) if v["remote"] else 0), v["expires"])
                      for k, v in self.learned.items() if self.now < v["expires"])

    def service_stage(self, pkt):
        if pkt["proto"] not in (6, 17, 132) or not self.lb:
            return pkt, 0, None
        regs = {4: ovs_cls.EP_TO_SELECT}
        if pkt["dst"] in self.np_addrs:
            regs[4] |= 0x80000  # ToNodePortAddressRegMark
        hit = [f for f in self.lb if f["proto"] == pkt["proto"] and f["port"] == pkt.get("dport", 0) and
               (regs[4] & f["r4m"]) == f["r4v"] and (f["dst"] is None or f["dst"] == pkt["dst"])]
        if not hit:
            return pkt, 0, None
        assert len(hit) == 1, hit
        p = dict(pkt)
        p.setdefault("ct_dst", pkt["dst"])
        flags = ovs_cls.LB_HIT
        _apply(regs, hit[0]["acts"])
        gid = next(a[1] for a in hit[0]["acts"] if a[0] == "group")
        if 7 in regs:
            p["svc_group"] = regs[7]
        res = {"group_id": gid, "endpoint_ip": 0, "endpoint_port": 0, "out_port": 0}
        buckets = self.groups6.get(gid)
        if not buckets:
            return p, flags | ovs_cls.LB_NO_ENDPOINT, res
        own = ovs_cls.select_bucket(buckets, dict(pkt, src=fold(pkt["src"]), dst=fold(pkt["dst"])))
        own_regs = {}
        _apply(own_regs, own["actions"])
        if own_regs.get(0, 0) & ovs_cls.SVC_NO_EP:
            return p, flags | ovs_cls.LB_NO_ENDPOINT, res
        bucket = own
        if (regs[4] & EP_STATE_MASK) == EP_TO_LEARN:
            key = (pkt["proto"], pkt.get("dport", 0), pkt["dst"], pkt["src"])
            e = self.learned.get(key)
            found = None
            if e is not None and self.now < e["expires"]:
                for b in buckets:  # still an Endpoint of the Service?
                    r = {}
                    _apply(r, b["actions"])
                    if r.get("xxreg3") == e["xx"] and (r.get(4, 0) & 0xFFFF) == e["port"]:
                        found = b
                        break
            if found is not None:
                bucket = found
                flags |= gpc.LB_AFFINITY
                self.n_hits += 1
            elif pkt.get("ct_state", ovs_cls.CT_NEW | ovs_cls.CT_TRK) & ovs_cls.CT_NEW:
                if ("resubmit", "ServiceLB") not in own["actions"]:
                    raise ValueError("affinity Service whose bucket does not resubmit to ServiceLB: group %d" % gid)
                if key in self.blocked:
                    self.n_overflow += 1
                else:
                    r = dict(regs)
                    _apply(r, own["actions"])
                    lf = [l for l in self.learn if l["proto"] == pkt["proto"] and l["port"] == pkt.get("dport", 0) and
                          (r[4] & l["r4m"]) == l["r4v"] and (l["dst"] is None or l["dst"] == pkt["dst"])]
                    if len(lf) != 1:
                        raise ValueError("no learn flow for an EpToLearn packet: %r" % (key,))
                    self.learned[key] = {"xx": r.get("xxreg3", 0), "port": r[4] & 0xFFFF, "remote": bool(r[4] & ovs_cls.REMOTE_EP),
                                         "expires": self.now + lf[0]["timeout"], "cookie": lf[0]["cookie"]}
                    flags |= gpc.LB_AFFINITY | gpc.LB_LEARNED
                    self.n_learned += 1
        _apply(regs, bucket["actions"])
        regs[4] = (regs[4] & ~EP_STATE_MASK) | EP_SELECTED  # the learn flow's / learned flow's load
        if regs.get(4, 0) & ovs_cls.REMOTE_EP:
            flags |= ovs_cls.LB_REMOTE
        ep_ip, ep_port = regs.get("xxreg3", 0), regs.get(4, 0) & 0xFFFF
        res.update(endpoint_ip=ep_ip, endpoint_port=ep_port)
        for d in self.dnat:
            if d["proto"] == pkt["proto"] and d["xx"] == ep_ip and (regs.get(4, 0) & d["r4m"]) == d["r4v"]:
                p["dst"], p["dport"] = d["nat"]
                flags |= ovs_cls.LB_DNAT
        if ep_ip in self.pods:
            p["out_port"], p["dest"] = self.pods[ep_ip], ovs_cls.DEST_POD
        else:
            p["out_port"], p["dest"] = 0, ovs_cls.DEST_TUNNEL if flags & ovs_cls.LB_REMOTE else ovs_cls.DEST_GATEWAY
        res["out_port"] = p["out_port"]
        return p, flags, res


def run(pipe, cols6, now):
    """The batch through `pipe` serially in caller order at clock `now`: (verdicts (n, 2), lb (n,) LB6_DTYPE)."""
    pipe.now = now
    return svc6_model.run(pipe, cols6, len(cols6["dst6"]))
