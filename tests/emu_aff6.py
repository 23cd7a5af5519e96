"""Loader for the TEST-ONLY host run of the IPv6 session-affinity passes (tests/csrc/emu_aff6.cpp) and
the emulated IPv6 classification with affinity Services: a host table driven exactly as the library
drives the device one (api.cpp aff6_prepare: reset on first use, a sweep of the expired entries
whenever the clock has moved since the last one, one launch sequence number per batch, the bid words
reset when the 32-bit sequence would wrap), the learn and resolve bodies of core.hpp over the batch,
packets of a Service without Endpoints set aside (rejected in EndpointDNAT), the existing IPv6
emulation of the policy stages on the rewritten columns."""
import ctypes as C
import ipaddress
import os
import subprocess

import numpy as np

from antrea_amd import gpc
from tests import emu
from tests.emu_aff import HITS, LEARNED, LIVE, OVERFLOW, SWEEP_BIDS, SWEEP_COUNT, SWEEP_EXPIRED, SWEEP_RESET

LIB = os.path.join(emu.OUT, "libgpc_emu_aff6.so")
SLOT_WORDS = 16  # core.hpp kAff6SlotWords
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    src = os.path.join(emu.HERE, "csrc", "emu_aff6.cpp")
    deps = [src, os.path.join(emu.ROOT, "antrea_amd", "csrc", "core.hpp"), os.path.join(emu.ROOT, "include", "gpc.h")]
    os.makedirs(emu.OUT, exist_ok=True)
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in deps):
        tmp = "%s.%d.tmp" % (LIB, os.getpid())  # renamed into place: parallel workers never load a half-written file
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + os.path.join(emu.ROOT, "include"),
                        "-I" + os.path.join(emu.ROOT, "antrea_amd", "csrc"), src, "-o", tmp], check=True)
        os.replace(tmp, LIB)
    _lib = C.CDLL(LIB)
    _lib.emu_aff6_sweep.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32]
    _lib.emu_aff6_image.argtypes = [C.c_void_p]
    _lib.emu_aff6_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int,
                                    C.POINTER(gpc.gpc_pkt_soa), C.c_size_t] + [C.c_void_p] * 7
    _lib.emu_aff6_candidates.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                         C.c_void_p]
    _lib.emu_aff6_fold.argtypes = [C.c_void_p]
    _lib.emu_aff6_fold.restype = C.c_uint32
    return _lib


def addr_bytes(addrs):
    """(n, 16) uint8 of IPv6 addresses given as strings, ints or an (n, 16) array."""
    if isinstance(addrs, np.ndarray):
        return np.ascontiguousarray(addrs, np.uint8).reshape(-1, 16)
    return np.array([list(ipaddress.IPv6Address(a).packed) for a in addrs], np.uint8).reshape(-1, 16)


def candidates(install, srcs, log2, np_id=0, bits=64):
    """core.hpp aff6_digest / aff_candidates of the keys (install id, NodePort address id, client
    address) for every address of `srcs`: (digests (n,) uint64, candidate slots in scan order (n, 4))."""
    a = addr_bytes(srcs)
    dig = np.zeros(len(a), np.uint64)
    out = np.zeros((len(a), 4), np.uint32)
    load().emu_aff6_candidates(install, np_id, a.ctypes.data, len(a), log2, bits, dig.ctypes.data, out.ctypes.data)
    return dig, out


def fold(addr):
    """core.hpp fold6 of one address."""
    return int(load().emu_aff6_fold(addr_bytes([addr]).ctypes.data))


def affinity_services(clf):
    """The affinity Services of the committed IPv6 Service image as (install id, group id, timeout), in
    the order of the Service records (tests/emu_aff.py affinity_services)."""
    b = C.POINTER(C.c_uint32)()
    n = C.c_size_t()
    gpc._check(clf.lib.gpc_debug_service_image6(clf.h, C.byref(b), C.byref(n)), "gpc_debug_service_image6")
    if not n.value or not b[11]:
        return []
    rec = lambda i: b[2] + 4 * i
    return [(int(b[b[10] + i]), int(b[rec(i) + 2]), int(b[rec(i) + 3]) >> 16) for i in range(b[3]) if b[b[10] + i]]


def install_ids(clf):
    return {s[0] for s in affinity_services(clf)}


def _be(words):
    return b"".join(int(w).to_bytes(4, "big") for w in words)


class Table6:
    """The IPv6 affinity table of one device slot, on the host."""

    def __init__(self, log2, stale_find=False, bits=64):
        """bits: gpc_debug_set_affinity6_digest_bits; stale_find: the learn pass's plain loads see the
        table as it was before the pass (emu_aff6.cpp AffOpsStale); the results must not differ."""
        self.log2, self.bits = log2, bits
        self.stale_find = stale_find
        self.tab = np.zeros(SLOT_WORDS << log2, np.uint32)
        self.ctr = np.zeros(4, np.uint64)
        self.seq = self.swept = self.sweeps = 0
        self.fresh = True

    def _sweep(self, now, mode):
        load().emu_aff6_sweep(self.tab.ctypes.data, self.log2, self.ctr.ctypes.data, now, mode)

    def set_seq(self, seq):
        """gpc_debug_set_affinity_seq6."""
        assert not self.fresh, "a table's first use restarts the sequence"
        self.seq = seq & 0xffffffff

    def stage(self, clf, cols6, now):
        """The Service stage alone: (rewritten columns, lb results (n,) LB6_DTYPE, no-Endpoint mask)."""
        svc = clf.debug_service_image6()
        assert svc and load().emu_aff6_image(svc), "no IPv6 Service image with an affinity Service committed"
        if self.fresh:
            self._sweep(now, SWEEP_RESET)
            self.fresh, self.swept = False, now
        elif self.seq >= 0xfffffffe:  # the sequence wraps: the bid words start over
            self._sweep(now, SWEEP_BIDS)
            self.seq = 0
        if now > self.swept:
            self._sweep(now, SWEEP_EXPIRED)
            self.swept = now
            self.sweeps += 1
        self.seq += 1
        soa, keep, n = gpc.pkt_soa_host(cols6)
        dst6 = np.zeros((n, 16), np.uint8)
        dport, out_port = np.zeros(n, np.uint16), np.zeros(n, np.uint32)
        svc_group, dest = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
        lb = np.zeros(n, gpc.LB6_DTYPE)
        noep = np.zeros(n, np.uint8)
        load().emu_aff6_batch(svc, self.tab.ctypes.data, self.log2, self.bits, self.ctr.ctypes.data, now, self.seq,
                              int(self.stale_find), C.byref(soa), n,
                              *[a.ctypes.data for a in (dst6, dport, out_port, svc_group, dest, lb, noep)])
        out = dict(cols6, dst6=dst6, dport=dport, out_port=out_port, svc_group=svc_group, dest=dest)
        out.setdefault("ct_dst6", np.ascontiguousarray(cols6["dst6"]))  # ct_ipv6_dst: the pre-NAT destination
        return out, lb, noep.astype(bool)

    def classify6(self, clf, cols6, now, counters=None, lb=None):
        """Emulated IPv6 verdicts (n, 2) of the epoch last committed by `clf` at clock `now`. An image
        without an affinity Service takes the plain emulation, as the library takes its plain launches."""
        from tests import emu_svc6
        n = len(cols6["dst6"])
        svc = clf.debug_service_image6()
        if not (svc and load().emu_aff6_image(svc)):
            return emu_svc6.classify6(clf, cols6, counters, lb)
        rw, res, noep = self.stage(clf, cols6, now)
        if lb is not None:
            lb[:n] = res
        out = np.zeros((n, 2), dtype=gpc.VERDICT_DTYPE)
        out[noep, 0] = (0, gpc.ACT_NAMES.index("REJECT"), gpc.VTABLE_ENDPOINT_DNAT, 0, 0)
        live = ~noep
        if live.any():
            out[live] = emu.classify6(clf, {k: np.ascontiguousarray(v[live]) for k, v in rw.items()}, counters)
        return out

    def live(self, now):
        """Live entries as sorted (client address, id word, endpoint address, endpoint port | flags,
        expires), addresses as ints -- the id word is (install id << 8 | NodePort address id)."""
        t = self.tab.reshape(-1, SLOT_WORDS)
        m = ((t[:, 0] | t[:, 1]) != 0) & (t[:, 15] != 0) & (now < t[:, 13])
        return sorted((int.from_bytes(_be(r[4:8]), "big"), int(r[15]), int.from_bytes(_be(r[8:12]), "big"), int(r[12]), int(r[13]))
                      for r in t[m])

    def stats(self, now):
        self.ctr[LIVE] = 0
        self._sweep(now, SWEEP_COUNT)
        return {"slots": 1 << self.log2, "live": int(self.ctr[LIVE]), "learned": int(self.ctr[LEARNED]),
                "hits": int(self.ctr[HITS]), "overflow": int(self.ctr[OVERFLOW]), "sweeps": self.sweeps}
