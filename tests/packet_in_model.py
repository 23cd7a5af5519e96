"""Test-side model of the packet-in queue, from the oracle alone: the verdicts come from the oracle's
OVS classifier restatement (oracle/ovs_cls.py) over the oracle compiler's flows, the
PacketInOperationField of a conjunction from the oracle compiler's own action flows -- the
("set_reg", 0, ops << 25, 0xFE000000) action of the rule-table flow matching conj_id. Nothing here
reads the product's image or calls its compiler.

What OVS sends to the agent (packetin.go) for a packet with verdicts v = (egress, ingress):
  * a Service without Endpoints (v[0] = REJECT at EndpointDNAT): one SvcReject record, nothing else;
  * per stage, the DNS interception flow (controller action: FLAG_PACKETIN): one DNS record;
  * per stage, ALLOW / DROP / REJECT by a conjunction whose action flow loads a non-zero
    PacketInOperationField: one NP record carrying that value, the table and the disposition.
Records are ordered by packet, egress before ingress."""
import numpy as np

from antrea_amd import gpc
from oracle import ovs_cls

RULE_TABLES = ("AntreaPolicyEgressRule", "EgressRule", "EgressDefaultRule", "AntreaPolicyIngressRule", "IngressRule",
               "IngressDefaultRule")
CAT_NP, CAT_DNS, CAT_SVC_REJECT = 1, 2, 4       # packetin.go:45-55
OP_LOGGING, OP_STORE_DENY, OP_REJECT = 1, 2, 4  # as oracle/compiler.py conjunction_deny_flow assigns them


def ops_map(fnp):
    """{conj id: PacketInOperationField} of the oracle compiler's realized flows."""
    out = {}
    for f in fnp.installed.values():
        if f.table not in RULE_TABLES or "conj_id" not in f.match:
            continue
        cid = f.match["conj_id"][0]
        for a in f.actions:
            if a[0] == "set_reg" and a[1] == 0 and a[3] == 0xFE000000 and a[2]:
                assert out.get(cid, a[2] >> 25) == a[2] >> 25, "two action flows of one id disagree"
                out[cid] = a[2] >> 25
    return out


def verdicts(pipe, cols, v6=False):
    """(n, 2) VERDICT_DTYPE of the batch through the oracle pipeline, serially."""
    n = len(cols["sport"])
    out = np.zeros((n, 2), dtype=gpc.VERDICT_DTYPE)
    for i in range(n):
        pkt = {k: int(v[i]) for k, v in cols.items() if v.ndim == 1}
        if v6:
            for k in ("src6", "dst6", "ct_src6", "ct_dst6"):
                if k in cols:
                    pkt[k[:-1]] = int.from_bytes(bytes(cols[k][i]), "big")
            pkt["eth"] = 0x86DD
        e, g = pipe.classify(pkt)
        for j, v in enumerate((e, g)):
            out[i, j] = (v[1], v[0], v[2], v[3], v[4])
    return out


def records(v, ops):
    """The expected queue of (n, 2) verdicts: PACKET_IN_DTYPE, in order."""
    out = []
    for i in range(len(v)):
        e = v[i, 0]
        if e["action"] == ovs_cls.ACT_REJECT and e["table"] == ovs_cls.TABLE_ENDPOINT_DNAT:
            out.append((i, 0, CAT_SVC_REJECT, 0, 0, 2, 0, (0, 0, 0)))
            continue
        for s in (0, 1):
            x = v[i, s]
            table = 3 * s + int(x["table"])
            if x["flags"] & ovs_cls.FLAG_PACKETIN:
                out.append((i, int(x["conj_id"]), CAT_DNS, 0, table, 0, s, (0, 0, 0)))
            elif x["action"] in (ovs_cls.ACT_ALLOW, ovs_cls.ACT_DROP, ovs_cls.ACT_REJECT) and ops.get(int(x["conj_id"])):
                disposition = {ovs_cls.ACT_ALLOW: 0, ovs_cls.ACT_DROP: 1, ovs_cls.ACT_REJECT: 2}[int(x["action"])]
                out.append((i, int(x["conj_id"]), CAT_NP, ops[int(x["conj_id"])], table, disposition, s, (0, 0, 0)))
    return np.array(out, dtype=gpc.PACKET_IN_DTYPE) if out else np.zeros(0, dtype=gpc.PACKET_IN_DTYPE)
