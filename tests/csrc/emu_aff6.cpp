// TEST-ONLY single-threaded host run of the IPv6 session-affinity passes (core.hpp aff6_sweep_slot,
// aff6_learn, lb_stage6_aff: the bodies of classify.hip aff6_sweep_kernel / aff6_learn_kernel /
// aff6_resolve_kernel) over a host table and the IPv6 Service image the product library built
// (gpc_debug_service_image6). Writes the columns the stage rewrites; the caller then runs the
// existing IPv6 emulation (emu.cpp emu_classify6) on them. Never linked into libgpc.so.
#include <cstddef>
#include <cstdint>
#include <vector>

#include "core.hpp"
#include "gpc.h"

using namespace gpc;

namespace {
struct AffOpsHost {  // the atomics shim of a single thread
  static uint64_t cas(uint64_t* p, uint64_t expect, uint64_t v) {
    const uint64_t old = *p;
    if (old == expect) *p = v;
    return old;
  }
  static void min(uint64_t* p, uint64_t v) {
    if (v < *p) *p = v;
  }
  static void count(unsigned long long* c, bool pred) { *c += pred ? 1 : 0; }
};

// The same single thread, but the learn pass's plain loads (aff6_find, the slot's key and entry
// words) see the table as it was before the pass (tests/csrc/emu_aff.cpp AffOpsStale): aff6_learn
// runs over a snapshot and the atomics are redirected to the table itself. Only the claim and bid
// words change during a learn pass, so the result must be that of the plain run.
struct AffOpsStale {
  static inline uintptr_t snapshot = 0, table = 0;  // addresses of the two copies
  static uint64_t* real(uint64_t* p) { return reinterpret_cast<uint64_t*>(table + (reinterpret_cast<uintptr_t>(p) - snapshot)); }
  static uint64_t cas(uint64_t* p, uint64_t expect, uint64_t v) { return AffOpsHost::cas(real(p), expect, v); }
  static void min(uint64_t* p, uint64_t v) { AffOpsHost::min(real(p), v); }
  static void count(unsigned long long* c, bool pred) { AffOpsHost::count(c, pred); }
};

uint64_t mask_of(uint32_t bits) { return bits >= 64 ? ~0ull : (1ull << bits) - 1ull; }
}  // namespace

// The claim digest of the key (install id, NodePort address id, client address: 16 network-order
// bytes) under a mask of `bits` low bits, and its four candidate slots in a table of 2^log2 slots, in
// scan order: the product's own hash, for tests that build colliding keys. n consecutive keys:
// client address i of `src` (n x 16 bytes); digest[n], out[4 * n].
extern "C" int emu_aff6_candidates(uint32_t install, uint32_t np_id, const uint8_t* src, uint32_t n, uint32_t log2, uint32_t bits,
                                   uint64_t* digest, uint32_t* out) {
  for (uint32_t i = 0; i < n; i++) {
    uint32_t a[4];
    v6_words(src + 16 * size_t(i), a);
    const uint64_t d = aff6_digest((install << 8) | (np_id & 0xffu), a, mask_of(bits));
    if (digest) digest[i] = d;
    aff_candidates(d, log2, out + 4 * size_t(i));
  }
  return 0;
}

extern "C" uint32_t emu_aff6_fold(const uint8_t* a16) {
  uint32_t a[4];
  v6_words(a16, a);
  return fold6(a);
}

extern "C" int emu_aff6_sweep(uint32_t* tab, uint32_t log2, unsigned long long* ctr, uint32_t now, uint32_t mode) {
  const Aff6Table t{tab, log2, ctr, ~0ull};
  for (uint32_t s = 0; s < (1u << log2); s++) aff6_sweep_slot<AffOpsHost>(t, s, now, mode);
  return 0;
}

// Whether the IPv6 Service image holds a session-affinity Service.
extern "C" int emu_aff6_image(const uint32_t* svc) { return svc && reinterpret_cast<const SvcHdr*>(svc)->n_aff != 0; }

// The learn pass over the whole batch, then the resolve pass (as the two kernels run). dst6_out: n x
// 16 network-order bytes; lb_out: n gpc_lb_result6 (may be null); noep: n flags. stale_find: the
// learn pass with AffOpsStale.
extern "C" int emu_aff6_batch(const uint32_t* svc, uint32_t* tab, uint32_t log2, uint32_t bits, unsigned long long* ctr,
                              uint32_t now, uint32_t seq, int stale_find, const gpc_pkt_soa* pk, size_t n, uint8_t* dst6_out,
                              uint16_t* dport_out, uint32_t* out_port_out, uint32_t* svc_group_out, uint8_t* dest_out,
                              gpc_lb_result6* lb_out, uint8_t* noep) {
  const Aff6Table t{tab, log2, ctr, mask_of(bits)};
  const Aff6Cols cols{pk->src6, pk->dst6, pk->sport, pk->dport, pk->proto, pk->ct_state, n};
  if (stale_find) {
    std::vector<uint32_t> snap(tab, tab + (size_t(kAff6SlotWords) << log2));
    const Aff6Table before{snap.data(), log2, ctr, t.mask};
    AffOpsStale::snapshot = reinterpret_cast<uintptr_t>(snap.data());
    AffOpsStale::table = reinterpret_cast<uintptr_t>(tab);
    for (size_t i = 0; i < n; i++) aff6_learn<AffOpsStale>(svc, before, now, seq, uint32_t(i), cols);
  } else {
    for (size_t i = 0; i < n; i++) aff6_learn<AffOpsHost>(svc, t, now, seq, uint32_t(i), cols);
  }
  for (size_t i = 0; i < n; i++) {
    uint32_t dst[4];
    v6_words(pk->dst6 + 16 * i, dst);
    uint32_t dport = pk->dport[i], out_port = pk->out_port[i];
    uint32_t svc_group = pk->svc_group ? pk->svc_group[i] : 0u, dest = pk->dest ? pk->dest[i] : 0u;
    uint32_t lb[8];
    bool collided;
    const uint32_t f = lb_stage6_aff(svc, t, now, seq, uint32_t(i), cols, dst, dport, pk->proto[i], svc_group, out_port, dest, lb,
                                     &collided);
    AffOpsHost::count(ctr + kAffLearned, (f & GPC_LB_LEARNED) != 0u);
    AffOpsHost::count(ctr + kAffHits, (f & (GPC_LB_AFFINITY | GPC_LB_LEARNED)) == GPC_LB_AFFINITY);
    AffOpsHost::count(ctr + kAffOverflow, collided);
    for (int k = 0; k < 4; k++)
      for (int b = 0; b < 4; b++) dst6_out[16 * i + 4 * k + b] = uint8_t(dst[k] >> (24 - 8 * b));
    dport_out[i] = uint16_t(dport);
    out_port_out[i] = out_port;
    svc_group_out[i] = svc_group;
    dest_out[i] = uint8_t(dest);
    noep[i] = (f & GPC_LB_NO_ENDPOINT) ? 1 : 0;
    if (lb_out) {
      gpc_lb_result6& r = lb_out[i];
      for (int k = 0; k < 4; k++)
        for (int b = 0; b < 4; b++) r.endpoint_ip[4 * k + b] = uint8_t(lb[k] >> (24 - 8 * b));
      r.endpoint_port = uint16_t(lb[4] & 0xffffu);
      r.flags = uint8_t(lb[4] >> 16);
      r.reserved = 0;
      r.group_id = lb[5];
      r.out_port = lb[6];
      r.reserved2 = 0;
    }
  }
  return 0;
}
