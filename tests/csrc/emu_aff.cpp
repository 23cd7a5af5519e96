// TEST-ONLY single-threaded host run of the session-affinity passes (core.hpp aff_sweep_slot,
// aff_learn, lb_stage_aff: the bodies of classify.hip aff_sweep_kernel / aff_learn_kernel /
// aff_resolve_kernel) over a host table and the IPv4 Service image the product library built
// (gpc_debug_service_image). Writes the columns the stage rewrites; the caller then runs the existing
// emulation (emu.cpp emu_classify, no Service image) on them. Never linked into libgpc.so.
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

// The same single thread, but every packet's plain loads of the learn pass (aff_find, the entry's
// validity) see the table as it was before the pass, as a device lane may whose neighbours' claims
// have not become visible yet: aff_learn runs over a snapshot of the table, and the atomics -- whose
// addresses it derives from the snapshot -- are redirected to the table itself. Entries do not change
// during the learn pass, so only the key words differ between the two. The result must be that of
// the plain run: ownership is decided from what the compare-and-swap returns, never from the loads.
struct AffOpsStale {
  static inline uintptr_t snapshot = 0, table = 0;  // addresses of the two copies
  static uint64_t* real(uint64_t* p) { return reinterpret_cast<uint64_t*>(table + (reinterpret_cast<uintptr_t>(p) - snapshot)); }
  static uint64_t cas(uint64_t* p, uint64_t expect, uint64_t v) { return AffOpsHost::cas(real(p), expect, v); }
  static void min(uint64_t* p, uint64_t v) { AffOpsHost::min(real(p), v); }
  static void count(unsigned long long* c, bool pred) { AffOpsHost::count(c, pred); }
};
}  // namespace

// The four candidate slots of the key (install id, NodePort address id, client address) in a table
// of 2^log2 slots, in scan order: the product's own hash, for tests that build colliding keys.
extern "C" int emu_aff_candidates(uint32_t install, uint32_t np_id, uint32_t src, uint32_t log2, uint32_t* out) {
  aff_candidates(aff_key(install, np_id, src), log2, out);
  return 0;
}
// The same for n consecutive client addresses from `src` on: out[4 * n].
extern "C" int emu_aff_candidates_range(uint32_t install, uint32_t np_id, uint32_t src, uint32_t n, uint32_t log2, uint32_t* out) {
  for (uint32_t i = 0; i < n; i++) aff_candidates(aff_key(install, np_id, src + i), log2, out + 4 * size_t(i));
  return 0;
}

extern "C" int emu_aff_sweep(uint32_t* tab, uint32_t log2, unsigned long long* ctr, uint32_t now, uint32_t mode) {
  const AffTable t{tab, log2, ctr};
  for (uint32_t s = 0; s < (1u << log2); s++) aff_sweep_slot<AffOpsHost>(t, s, now, mode);
  return 0;
}

// Whether the Service image holds a session-affinity Service.
extern "C" int emu_aff_image(const uint32_t* svc) { return svc && reinterpret_cast<const SvcHdr*>(svc)->n_aff != 0; }

// The learn pass over the whole batch, then the resolve pass (as the two kernels run). lb_out: n
// gpc_lb_result (may be null); noep: n flags. stale_find: the learn pass with AffOpsStale.
extern "C" int emu_aff_batch(const uint32_t* svc, uint32_t* tab, uint32_t log2, unsigned long long* ctr, uint32_t now,
                             uint32_t seq, int read_only, int stale_find, const gpc_pkt_soa* pk, size_t n, uint32_t* dst_out,
                             uint16_t* dport_out, uint32_t* out_port_out, uint32_t* svc_group_out, uint8_t* dest_out,
                             uint32_t* lb_out, uint8_t* noep) {
  const AffTable t{tab, log2, ctr};
  if (!read_only && stale_find) {
    std::vector<uint32_t> snap(tab, tab + (size_t(kAffSlotWords) << log2));
    const AffTable before{snap.data(), log2, ctr};
    AffOpsStale::snapshot = reinterpret_cast<uintptr_t>(snap.data());
    AffOpsStale::table = reinterpret_cast<uintptr_t>(tab);
    for (size_t i = 0; i < n; i++)
      aff_learn<AffOpsStale>(svc, before, now, seq, uint32_t(i), pk->src[i], pk->dst[i], pk->dport[i], pk->proto[i],
                             pk->ct_state ? pk->ct_state[i] : uint32_t(GPC_CT_NEW | GPC_CT_TRK));
  } else if (!read_only) {
    for (size_t i = 0; i < n; i++)
      aff_learn<AffOpsHost>(svc, t, now, seq, uint32_t(i), pk->src[i], pk->dst[i], pk->dport[i], pk->proto[i],
                            pk->ct_state ? pk->ct_state[i] : uint32_t(GPC_CT_NEW | GPC_CT_TRK));
  }
  for (size_t i = 0; i < n; i++) {
    uint32_t dst = pk->dst[i], dport = pk->dport[i], out_port = pk->out_port[i];
    uint32_t svc_group = pk->svc_group ? pk->svc_group[i] : 0u, dest = pk->dest ? pk->dest[i] : 0u;
    uint32_t lb[4];
    const uint32_t f = lb_stage_aff(svc, t, now, seq, read_only != 0, uint32_t(i), pk->src[i], dst, pk->sport[i], pk->sport, dport,
                                    pk->proto[i], svc_group, out_port, dest, lb);
    if (!read_only) {
      AffOpsHost::count(ctr + kAffLearned, (f & GPC_LB_LEARNED) != 0u);
      AffOpsHost::count(ctr + kAffHits, (f & (GPC_LB_AFFINITY | GPC_LB_LEARNED)) == GPC_LB_AFFINITY);
    }
    dst_out[i] = dst;
    dport_out[i] = uint16_t(dport);
    out_port_out[i] = out_port;
    svc_group_out[i] = svc_group;
    dest_out[i] = uint8_t(dest);
    noep[i] = (f & GPC_LB_NO_ENDPOINT) ? 1 : 0;
    if (lb_out)
      for (int k = 0; k < 4; k++) lb_out[4 * i + k] = lb[k];
  }
  return 0;
}
