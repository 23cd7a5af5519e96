"""Test-side executor of the IPv6 AntreaProxy flows. The oracle's flow parser (oracle/flowtext.py)
and Service restatement (oracle/service.py) know no xxreg3, so this subclass of the oracle Pipeline
keeps the IPv6 Service / group lines itself, parses them with its own few regexes and overrides
service_stage: NodePortMark -> ServiceLB -> select_bucket over the folded addresses -> EndpointDNAT
match on xxreg3 + reg4 -> nat -> Pod map. Everything after that (the NO_ENDPOINT reject, both
policy stages) is the unmodified oracle. Lines it cannot parse raise: nothing is skipped quietly."""
import ipaddress
import re

import numpy as np

from antrea_amd import gpc
from oracle import ovs_cls

SVC_TABLES = ("ServiceLB", "EndpointDNAT", "NodePortMark", "SNATMark")
_PROTO = {"tcp6": 6, "udp6": 17, "sctp6": 132}
_NPM = re.compile(r"table=NodePortMark, priority=200,ipv6,ipv6_dst=([0-9a-f:]+) actions=set_field:0x80000/0x80000->reg4$")
_LB = re.compile(r"table=ServiceLB, priority=200,(tcp6|udp6|sctp6),reg4=0x([0-9a-f]+)/0x([0-9a-f]+)"
                 r"(?:,ipv6_dst=([0-9a-f:]+))?,tp_dst=(\d+) actions=(.+)$")
_DNAT = re.compile(r"table=EndpointDNAT, priority=200,(tcp6|udp6|sctp6),reg4=0x([0-9a-f]+)/0x([0-9a-f]+),xxreg3=0x([0-9a-f]+) "
                   r"actions=ct\(commit,table=\w+,zone=65510,nat\(dst=\[([0-9a-f:]+)\]:(\d+)\),exec\(")
_SETREG = re.compile(r"set_field:0x([0-9a-f]+)(?:/0x([0-9a-f]+))?->(reg\d+|xxreg3)$")


def _is_v6_line(line):
    return bool(re.search(r",(ipv6|tcp6|udp6|sctp6)[, ]", line))


def _actions(text):
    """[("set", field, value, mask|None) | ("group", id) | ("resubmit", table)]"""
    out = []
    for a in text.split(","):
        m = _SETREG.match(a)
        if m:
            out.append(("set", m.group(3), int(m.group(1), 16), int(m.group(2), 16) if m.group(2) else None))
        elif a.startswith("group:"):
            out.append(("group", int(a[6:])))
        elif a.startswith("resubmit:"):
            out.append(("resubmit", a[9:]))
        else:
            raise ValueError("unparsed action %r" % a)
    return out


def _apply(regs, acts):
    for a in acts:
        if a[0] != "set":
            continue
        _, f, v, m = a
        if f == "xxreg3":
            regs["xxreg3"] = v
        else:
            r = int(f[3:])
            m = 0xFFFFFFFF if m is None else m
            regs[r] = (regs.get(r, 0) & ~m) | (v & m)


def fold(a):
    """XOR of the four big-endian 32-bit words of a 128-bit address."""
    return (a ^ (a >> 32) ^ (a >> 64) ^ (a >> 96)) & 0xFFFFFFFF


class Pipeline6(ovs_cls.Pipeline):
    def __init__(self, flow_lines, tiers=None, group_lines=None, pods=None):
        mine = [l for l in flow_lines if any("table=%s," % t in l for t in SVC_TABLES) and _is_v6_line(l)]
        rest = [l for l in flow_lines if not any("table=%s," % t in l for t in SVC_TABLES)]
        super().__init__(rest, tiers, [], pods)
        self.np_addrs, self.lb, self.dnat, self.groups6 = set(), [], [], {}
        for l in mine:
            if "table=SNATMark" in l:
                continue  # hairpin SNAT: after the policy stages
            m = _NPM.search(l)
            if m:
                self.np_addrs.add(int(ipaddress.IPv6Address(m.group(1))))
                continue
            m = _LB.search(l)
            if m:
                self.lb.append({"proto": _PROTO[m.group(1)], "r4v": int(m.group(2), 16), "r4m": int(m.group(3), 16),
                                "dst": int(ipaddress.IPv6Address(m.group(4))) if m.group(4) else None,
                                "port": int(m.group(5)), "acts": _actions(m.group(6))})
                continue
            m = _DNAT.search(l)
            if m:
                self.dnat.append({"proto": _PROTO[m.group(1)], "r4v": int(m.group(2), 16), "r4m": int(m.group(3), 16),
                                  "xx": int(m.group(4), 16), "nat": (int(ipaddress.IPv6Address(m.group(5))), int(m.group(6)))})
                continue
            raise ValueError("unparsed IPv6 Service flow: " + l)
        for l in group_lines or []:
            m = re.match(r"group_id=(\d+),type=select(.*)$", l)
            buckets = []
            for b in m.group(2).split(",bucket=")[1:]:
                bm = re.match(r"bucket_id:(\d+),weight:100,actions=(.+)$", b)
                buckets.append({"id": int(bm.group(1)), "actions": _actions(bm.group(2))})
            if not any(a[0] == "set" and a[1] == "reg3" for b in buckets for a in b["actions"]):  # (IPv4 groups: not ours)
                self.groups6[int(m.group(1))] = buckets

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
        p.setdefault("ct_dst", pkt["dst"])  # ct_ipv6_dst: the pre-NAT (Service) address
        flags = ovs_cls.LB_HIT
        _apply(regs, hit[0]["acts"])
        gid = next(a[1] for a in hit[0]["acts"] if a[0] == "group")
        if 7 in regs:
            p["svc_group"] = regs[7]
        res = {"group_id": gid, "endpoint_ip": 0, "endpoint_port": 0, "out_port": 0}
        buckets = self.groups6.get(gid)
        if not buckets:
            return p, flags | ovs_cls.LB_NO_ENDPOINT, res
        b = ovs_cls.select_bucket(buckets, dict(pkt, src=fold(pkt["src"]), dst=fold(pkt["dst"])))
        _apply(regs, b["actions"])
        if regs.get(0, 0) & ovs_cls.SVC_NO_EP:
            return p, flags | ovs_cls.LB_NO_ENDPOINT, res
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


def run(pipe, cols6, n):
    """(verdicts (n, 2), lb (n,) LB6_DTYPE) of the first n packets of an IPv6 batch."""
    out = np.zeros((n, 2), dtype=gpc.VERDICT_DTYPE)
    lb = np.zeros(n, dtype=gpc.LB6_DTYPE)
    for i in range(n):
        pkt = {k: int(v[i]) for k, v in cols6.items() if v.ndim == 1}
        for k in ("src6", "dst6", "ct_src6", "ct_dst6"):
            if k in cols6:
                pkt[k[:-1]] = int.from_bytes(bytes(cols6[k][i]), "big")
        pkt["eth"] = 0x86DD
        rec = []
        e, g = pipe.classify(pkt, lb=rec)
        for j, v in enumerate((e, g)):
            out[i, j] = (v[1], v[0], v[2], v[3], v[4])
        flags, r = rec[0]
        if flags:
            lb[i] = (list(int(r["endpoint_ip"]).to_bytes(16, "big")), r["endpoint_port"], flags, 0, r["group_id"],
                     r["out_port"], 0)
    return out, lb
