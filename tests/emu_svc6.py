"""Loader for the TEST-ONLY host run of the IPv6 Service stage (tests/csrc/emu_svc6.cpp) and the
emulated IPv6 classification with Services: lb_stage6 over the batch, packets of a Service without
Endpoints set aside (rejected in EndpointDNAT), the existing emu.classify6 on the rewritten columns."""
import ctypes as C
import os
import subprocess

import numpy as np

from antrea_amd import gpc
from tests import emu

LIB = os.path.join(emu.OUT, "libgpc_emu_svc6.so")
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    src = os.path.join(emu.HERE, "csrc", "emu_svc6.cpp")
    deps = [src, os.path.join(emu.ROOT, "antrea_amd", "csrc", "core.hpp"), os.path.join(emu.ROOT, "include", "gpc.h")]
    os.makedirs(emu.OUT, exist_ok=True)
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in deps):
        tmp = "%s.%d.tmp" % (LIB, os.getpid())  # renamed into place: parallel workers never load a half-written file
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + os.path.join(emu.ROOT, "include"),
                        "-I" + os.path.join(emu.ROOT, "antrea_amd", "csrc"), src, "-o", tmp], check=True)
        os.replace(tmp, LIB)
    _lib = C.CDLL(LIB)
    _lib.emu_lb6.argtypes = [C.c_void_p, C.POINTER(gpc.gpc_pkt_soa), C.c_size_t] + [C.c_void_p] * 7
    return _lib


def lb_stage(clf, cols):
    """The Service stage alone: (rewritten columns, lb results (n,) LB6_DTYPE, no-Endpoint mask)."""
    svc6 = clf.debug_service_image6()
    assert svc6, "no IPv6 Service image committed"
    soa, keep, n = gpc.pkt_soa_host(cols)
    dst6 = np.zeros((n, 16), np.uint8)
    dport, out_port = np.zeros(n, np.uint16), np.zeros(n, np.uint32)
    svc_group, dest = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    lb = np.zeros(n, gpc.LB6_DTYPE)
    noep = np.zeros(n, np.uint8)
    load().emu_lb6(svc6, C.byref(soa), n, *[a.ctypes.data for a in (dst6, dport, out_port, svc_group, dest, lb, noep)])
    out = dict(cols, dst6=dst6, dport=dport, out_port=out_port, svc_group=svc_group, dest=dest)
    out.setdefault("ct_dst6", np.ascontiguousarray(cols["dst6"]))  # ct_ipv6_dst: the pre-NAT destination
    return out, lb, noep.astype(bool)


def classify6(clf, cols, counters=None, lb=None):
    """Emulated IPv6 verdicts (n, 2) of the epoch last committed by `clf`, Service stage included
    when an IPv6 Service image is committed. `lb`: optional LB6_DTYPE array receiving its results."""
    n = len(cols["dst6"])
    if not clf.debug_service_image6():
        if lb is not None:
            lb[:n] = np.zeros(n, gpc.LB6_DTYPE)
        return emu.classify6(clf, cols, counters)
    rw, res, noep = lb_stage(clf, cols)
    if lb is not None:
        lb[:n] = res
    out = np.zeros((n, 2), dtype=gpc.VERDICT_DTYPE)
    out[noep, 0] = (0, gpc.ACT_NAMES.index("REJECT"), gpc.VTABLE_ENDPOINT_DNAT, 0, 0)
    live = ~noep
    if live.any():
        out[live] = emu.classify6(clf, {k: np.ascontiguousarray(v[live]) for k, v in rw.items()}, counters)
    return out
