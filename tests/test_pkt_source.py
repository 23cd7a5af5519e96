"""Packet source column (gpc_pkt_soa.source, gpc_config.packet_source) and the short-circuit flow of
external Services with externalTrafficPolicy: Local, CPU tier: the flow text against the reference's
own expected strings (client_test.go "Service NodePort,SessionAffinity,Short-circuiting" and "Service
LoadBalancer,SessionAffinity,Short-circuiting", transcribed in
tests/golden/service_flows_short_circuit.json), the gate, the Service image's identity without such a
Service, and the host emulation of the stage's core.hpp bodies (tests/emu_src.py) against the model
over the realized text (tests/svc_source_model.py), both families, with and without session affinity."""
import ctypes as C
import ipaddress
import re

import numpy as np
import pytest

from antrea_amd import gpc
from tests import emu, emu_src
from tests import pkt_source_cases as pc
from tests.util import load_golden

GOLD = load_golden("service_flows_short_circuit.json")
A, L, SC = gpc.LB_AFFINITY, gpc.LB_LEARNED, gpc.LB_SHORT_CIRCUIT
EXT_LOCAL = {"ip": "10.96.0.100", "port": 80, "protocol": "TCP", "cluster_group_id": 100, "local_group_id": 101,
             "is_external": True, "traffic_policy_local": True}
EXT_LOCAL6 = dict(EXT_LOCAL, ip="fd00:96::100")


def _lb_lines(c):
    return [l for l in c.dump_flows() if "table=ServiceLB" in l]


def _image(c, family=4):
    b = C.POINTER(C.c_uint32)()
    n = C.c_size_t()
    fn = c.lib.gpc_debug_service_image6 if family == 6 else c.lib.gpc_debug_service_image
    gpc._check(fn(c.h, C.byref(b), C.byref(n)), "gpc_debug_service_image")
    return np.ctypeslib.as_array(b, (n.value,)).copy() if n.value else np.zeros(0, np.uint32)


@pytest.mark.parametrize("case", GOLD["service_flows"], ids=[c["name"] for c in GOLD["service_flows"]])
def test_golden_flows(case):
    c = gpc.Classifier(cookie=0x1010000000000, session_affinity=10, packet_source=1)
    c.initialize()
    before = c.dump_flows()
    c.install_service_flows(case["config"])
    assert _lb_lines(c) == case["expected"]  # text and order, as the reference lists them
    cfg = case["config"]
    c.uninstall_service_flows(cfg["ip"], cfg["port"], cfg["protocol"])
    assert c.dump_flows() == before and not _lb_lines(c)


def _derived_210(line200, cluster_gid):
    """The short-circuit line by the reference's rule (serviceLBFlows, pipeline.go:2417-2422), from the
    priority-200 line: priority 210, FromLocalRegMark (reg4[28]) merged into the one reg4= term, reg7
    and group = the Cluster group; every other match and load identical."""
    m = re.search(r"reg4=0x([0-9a-f]+)/0x([0-9a-f]+)", line200)
    out = line200.replace("priority=200,", "priority=210,")
    out = out.replace(m.group(0), "reg4=0x%x/0x%x" % (int(m.group(1), 16) | 1 << 28, int(m.group(2), 16) | 1 << 28))
    out = re.sub(r"set_field:0x[0-9a-f]+->reg7", "set_field:0x%x->reg7" % cluster_gid, out)
    return re.sub(r"group:\d+$", "group:%d" % cluster_gid, out)


def test_derived_rule_reproduces_the_goldens():
    for case in GOLD["service_flows"]:
        assert _derived_210(case["expected"][1], case["config"]["cluster_group_id"]) == case["expected"][0]


@pytest.mark.parametrize("cfg,kw", [(EXT_LOCAL, {}), (dict(EXT_LOCAL, is_nodeport=True, ip="169.254.0.252"), {}),
                                    (EXT_LOCAL6, {"ipv6": True}), (dict(EXT_LOCAL6, affinity_timeout=30), {"ipv6": True})],
                         ids=["v4", "v4-nodeport", "v6", "v6-affinity"])
def test_unpinned_shapes_follow_the_rule(cfg, kw):
    """The reference holds no short-circuit case without affinity or in IPv6: those 210 lines are not
    pinned; they are derived from the 200 line by the rule the two goldens obey (above)."""
    c = gpc.Classifier(session_affinity=10, session_affinity6=10, packet_source=1, **kw)
    c.initialize()
    c.install_service_flows(cfg)
    lines = _lb_lines(c)
    assert len(lines) == (3 if cfg.get("affinity_timeout") else 2)
    assert "priority=210," in lines[0] and "priority=200," in lines[1]
    assert lines[0] == _derived_210(lines[1], cfg["cluster_group_id"])
    assert "group:%d" % cfg["local_group_id"] in lines[1]
    if cfg.get("affinity_timeout"):  # one learn flow, cookie | TrafficPolicyGroupID
        assert "priority=190," in lines[2] and lines[2].startswith("cookie=0x%x," % (0x1030000000000 | cfg["local_group_id"]))


@pytest.mark.parametrize("family", [4, 6])
def test_gate(family):
    cfg = EXT_LOCAL6 if family == 6 else EXT_LOCAL
    off = gpc.Classifier(ipv6=True)
    with pytest.raises(gpc.GpcError):
        off.install_service_flows(cfg)
    assert not _lb_lines(off)
    for ps in (0, 1):  # DSR and nested Services: rejected in either context
        c = gpc.Classifier(ipv6=True, packet_source=ps)
        for extra in ({"is_dsr": True}, {"is_nested": True}):
            for base in (cfg, dict(cfg, traffic_policy_local=False)):
                with pytest.raises(gpc.GpcError):
                    c.install_service_flows(dict(base, **extra))
        assert not _lb_lines(c)
    on = gpc.Classifier(ipv6=True, packet_source=1)
    on.install_service_flows(cfg)
    assert len(_lb_lines(on)) == 2


@pytest.mark.parametrize("family", [4, 6])
def test_image_identity_without_short_circuit(family):
    """With the gate on, a Service image without a short-circuit Service is the one a packet_source=0
    context builds, word for word; with one it differs and says so in its header."""
    wl, w6 = pc.make_workload(3, affinity=True, short_circuit_frac=0.0)
    w = w6 if family == 6 else wl
    imgs = []
    for ps in (0, 1):
        c = pc.make_product(w, family, affinity=True, packet_source=ps)
        emu.commit_host(c)
        imgs.append(_image(c, family))
        assert emu_src.short_circuit_services(c, family) == 0
    assert len(imgs[0]) and np.array_equal(imgs[0], imgs[1])
    wl, w6 = pc.make_workload(3, affinity=True)
    c = pc.make_product(w6 if family == 6 else wl, family, affinity=True)
    emu.commit_host(c)
    assert emu_src.short_circuit_services(c, family) > 0 and not np.array_equal(_image(c, family), imgs[0])


@pytest.mark.parametrize("affinity", [False, True], ids=["plain", "affinity"])
@pytest.mark.parametrize("family", [4, 6])
def test_emulation_equals_model(family, affinity):
    """Every gpc_source value plus 7 and 255, LoadBalancer IPs and NodePort Services, empty Local
    groups under served Cluster groups, Services with both empty; then the same batch without the
    column (NULL: UNKNOWN, nobody is local)."""
    wl, w6 = pc.make_workload(5, affinity)
    w = w6 if family == 6 else wl
    c = pc.make_product(w, family, affinity)
    emu.commit_host(c)
    model, side = pc.Model(w, c, family), pc.Emulation(c, family, affinity)
    cols = pc.make_batch(wl, 300, 11, family, established=0.3 if affinity else 0.0)
    got = side.run(cols)
    pc.check("batch", cols, got, model.run(cols))
    pc.coverage(cols, got[1], affinity)
    if affinity:
        assert side.live(pc.T0) == pc.model_live(model) and side.live(pc.T0)
        got = side.run(cols, pc.T0 + 1)  # the entries of the first batch, judged per source
        pc.check("batch, t + 1", cols, got, model.run(cols, pc.T0 + 1))
        assert side.live(pc.T0 + 1) == pc.model_live(model)
    bare = pc.make_batch(wl, 300, 11, family, established=0.3 if affinity else 0.0, source=False)
    got = side.run(bare, pc.T0 + 2)
    pc.check("NULL column", bare, got, model.run(bare, pc.T0 + 2))
    assert not (got[1]["flags"] & SC).any() and (got[1]["flags"] & gpc.LB_HIT).any()


@pytest.mark.parametrize("family", [4, 6])
def test_affinity_across_sources(family):
    """An entry learned by a Pod-source packet onto a remote Endpoint (from the Cluster group), then an
    uplink packet of the same client: in the same batch it takes its own bucket of the Local group and
    learns nothing (one write per key and batch); in the next batch the entry's Endpoint is not the
    Local group's, so the +new uplink packet overwrites it."""
    wl, w6 = pc.make_workload(2, affinity=True)
    w = w6 if family == 6 else wl
    c = pc.make_product(w, family, affinity=True)
    emu.commit_host(c)
    model, side = pc.Model(w, c, family), pc.Emulation(c, family, affinity=True)
    s = pc.remote_affinity_case(w, family)
    client = "fd00:10::c0a8:105" if family == 6 else "192.168.1.5"
    local_eps = {(int(ipaddress.ip_address(e["ip"])), e["port"]) for e in w.groups[s["local_group_id"]]}
    for sport in range(2000, 2400):  # a Pod-source packet whose bucket is an Endpoint the Local group lacks
        pod = pc.one_packet(s, family, client, sport, gpc.SOURCE_POD)
        _, lb = model.run(pod, pc.T0, learn=False)
        if (as_int(lb["endpoint_ip"][0]), int(lb["endpoint_port"][0])) not in local_eps:
            break
    else:
        raise AssertionError("no source port picks a remote Endpoint")
    up = pc.one_packet(s, family, client, 4000, gpc.SOURCE_UPLINK)
    est = pc.one_packet(s, family, client, 4001, gpc.SOURCE_UPLINK, ct_new=False)
    batch = pc.concat(pod, up, pod, est)
    got = side.run(batch, pc.T0)
    pc.check("same batch", batch, got, model.run(batch, pc.T0))
    f = got[1]["flags"]
    assert f[0] & (A | L | SC) == (A | L | SC) and f[2] & (A | L | SC) == (A | SC)
    assert f[1] & (A | L | SC) == 0 and f[3] & (A | L | SC) == 0  # the Local group lacks the Endpoint: own bucket
    assert got[1]["group_id"][0] == s["cluster_group_id"] and got[1]["group_id"][1] == s["local_group_id"]
    assert side.live(pc.T0) == pc.model_live(model) and len(side.live(pc.T0)) == 1
    assert side.live(pc.T0)[0][1] == int(as_int(got[1]["endpoint_ip"][0]))
    nxt = pc.concat(est, up, pod)
    got = side.run(nxt, pc.T0 + 1)
    pc.check("next batch", nxt, got, model.run(nxt, pc.T0 + 1))
    f = got[1]["flags"]
    assert f[0] & (A | L) == 0          # not +new: misses against the Local group, learns nothing
    assert f[1] & (A | L | SC) == A | L  # the +new uplink packet overwrites the entry
    assert f[2] & (A | L | SC) == A | SC  # the Cluster group holds the Local Endpoint: the Pod follows it
    assert (got[1]["endpoint_ip"][2] == got[1]["endpoint_ip"][1]).all()
    assert side.live(pc.T0 + 1) == pc.model_live(model) and len(side.live(pc.T0 + 1)) == 1
    assert side.live(pc.T0 + 1)[0][1] == int(as_int(got[1]["endpoint_ip"][1]))


def as_int(ep):
    return int.from_bytes(bytes(ep), "big") if np.ndim(ep) else int(ep)


@pytest.mark.parametrize("family", [4, 6])
def test_reinstall_as_plain_external(family):
    """A short-circuit Service installed again as a plain external one (Cluster policy), then a delta
    commit: its priority-210 flow and its second record are gone, local and external packets alike take
    the Cluster group, and the emulation still equals the model."""
    wl, w6 = pc.make_workload(5)
    w = w6 if family == 6 else wl
    c = pc.make_product(w, family)
    emu.commit_host(c)
    n_before = emu_src.short_circuit_services(c, family)
    s = next(x for x in w.services if x.get("is_external") and x.get("traffic_policy_local") and not x.get("is_nodeport")
             and w.groups[x["cluster_group_id"]])
    c.install_service_flows(dict(s, traffic_policy_local=False))
    emu.commit_host(c)
    assert emu_src.short_circuit_services(c, family) == n_before - 1
    model, side = pc.Model(w, c, family), pc.Emulation(c, family)
    cols = pc.make_batch(wl, 300, 13, family)
    got = side.run(cols)
    pc.check("after the reinstall", cols, got, model.run(cols))
    to_s = (got[1]["group_id"] == s["cluster_group_id"]) | (got[1]["group_id"] == s["local_group_id"])
    assert to_s.any() and (got[1]["group_id"][to_s] == s["cluster_group_id"]).all() and not (got[1]["flags"][to_s] & SC).any()
    assert (got[1]["flags"] & SC).any()  # the other short-circuit Services keep theirs
