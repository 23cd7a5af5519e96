// TEST-ONLY single-threaded host run of the Service stage with the packet source column
// (gpc_pkt_soa.source, gpc_config.packet_source): the bodies of classify.hip's Service-stage kernels
// -- lb_stage (classify_kernel), lb_stage6 (v6_lb_kernel), aff_learn / lb_stage_aff and aff6_learn /
// lb_stage6_aff (the affinity passes) -- called through their source-taking signatures over the
// Service images the product library built (gpc_debug_service_image / _image6). Writes the columns
// the stage rewrites; the caller then runs the existing emulation of the policy stages on them.
// Never linked into libgpc.so.
#include <cstddef>
#include <cstdint>

#include "core.hpp"
#include "gpc.h"

using namespace gpc;

namespace {
struct AffOpsHost {  // the atomics shim of a single thread (emu_aff.cpp)
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
uint32_t source_of(const gpc_pkt_soa* pk, size_t i) { return pk->source ? uint32_t(pk->source[i]) : uint32_t(GPC_SOURCE_UNKNOWN); }
void store6(const uint32_t* lb, gpc_lb_result6* r) {
  for (int k = 0; k < 4; k++)
    for (int b = 0; b < 4; b++) r->endpoint_ip[4 * k + b] = uint8_t(lb[k] >> (24 - 8 * b));
  r->endpoint_port = uint16_t(lb[4] & 0xffffu);
  r->flags = uint8_t(lb[4] >> 16);
  r->reserved = 0;
  r->group_id = lb[5];
  r->out_port = lb[6];
  r->reserved2 = 0;
}
}  // namespace

// Short-circuit Services of a Service image (SvcHdr.n_sc).
extern "C" int emu_src_image(const uint32_t* svc) { return svc ? int(reinterpret_cast<const SvcHdr*>(svc)->n_sc) : 0; }

// IPv4, no affinity table: lb_out n x 4 words (gpc_lb_result), noep n flags.
extern "C" int emu_src_lb4(const uint32_t* svc, const gpc_pkt_soa* pk, size_t n, uint32_t* dst_out, uint16_t* dport_out,
                           uint32_t* out_port_out, uint32_t* svc_group_out, uint8_t* dest_out, uint32_t* lb_out, uint8_t* noep) {
  for (size_t i = 0; i < n; i++) {
    uint32_t dst = pk->dst[i], dport = pk->dport[i], out_port = pk->out_port[i];
    uint32_t svc_group = pk->svc_group ? pk->svc_group[i] : 0u, dest = pk->dest ? pk->dest[i] : 0u;
    uint32_t lb[4];
    const uint32_t f = lb_stage(svc, pk->src[i], dst, pk->sport[i], dport, pk->proto[i], svc_group, out_port, dest, lb, source_of(pk, i));
    dst_out[i] = dst;
    dport_out[i] = uint16_t(dport);
    out_port_out[i] = out_port;
    svc_group_out[i] = svc_group;
    dest_out[i] = uint8_t(dest);
    noep[i] = (f & GPC_LB_NO_ENDPOINT) ? 1 : 0;
    for (int k = 0; k < 4; k++) lb_out[4 * i + k] = lb[k];
  }
  return 0;
}

// IPv4 with the affinity table: the learn pass over the whole batch, then the resolve pass.
extern "C" int emu_src_aff4(const uint32_t* svc, uint32_t* tab, uint32_t log2, unsigned long long* ctr, uint32_t now, uint32_t seq,
                            int read_only, const gpc_pkt_soa* pk, size_t n, uint32_t* dst_out, uint16_t* dport_out,
                            uint32_t* out_port_out, uint32_t* svc_group_out, uint8_t* dest_out, uint32_t* lb_out, uint8_t* noep) {
  const AffTable t{tab, log2, ctr};
  if (!read_only)
    for (size_t i = 0; i < n; i++)
      aff_learn<AffOpsHost>(svc, t, now, seq, uint32_t(i), pk->src[i], pk->dst[i], pk->dport[i], pk->proto[i],
                            pk->ct_state ? pk->ct_state[i] : uint32_t(GPC_CT_NEW | GPC_CT_TRK), source_of(pk, i));
  for (size_t i = 0; i < n; i++) {
    uint32_t dst = pk->dst[i], dport = pk->dport[i], out_port = pk->out_port[i];
    uint32_t svc_group = pk->svc_group ? pk->svc_group[i] : 0u, dest = pk->dest ? pk->dest[i] : 0u;
    uint32_t lb[4];
    const uint32_t f = lb_stage_aff(svc, t, now, seq, read_only != 0, uint32_t(i), pk->src[i], dst, pk->sport[i], pk->sport, dport,
                                    pk->proto[i], svc_group, out_port, dest, lb, source_of(pk, i), pk->source);
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
    for (int k = 0; k < 4; k++) lb_out[4 * i + k] = lb[k];
  }
  return 0;
}

// IPv6: tab == null: lb_stage6 (v6_lb_kernel); else the affinity passes over the IPv6 table (digest
// mask all ones). read_only: lb_stage6_aff<true>, as gpc_trace6 reads the table.
extern "C" int emu_src_lb6(const uint32_t* svc6, uint32_t* tab, uint32_t log2, unsigned long long* ctr, uint32_t now, uint32_t seq,
                           int read_only, const gpc_pkt_soa* pk, size_t n, uint8_t* dst6_out, uint16_t* dport_out,
                           uint32_t* out_port_out, uint32_t* svc_group_out, uint8_t* dest_out, gpc_lb_result6* lb_out,
                           uint8_t* noep) {
  const Aff6Table t{tab, log2, ctr, ~0ull};
  const Aff6Cols cols{pk->src6, pk->dst6, pk->sport, pk->dport, pk->proto, pk->ct_state, n, pk->source};
  if (tab && !read_only)
    for (size_t i = 0; i < n; i++) aff6_learn<AffOpsHost>(svc6, t, now, seq, uint32_t(i), cols);
  for (size_t i = 0; i < n; i++) {
    uint32_t dst[4];
    v6_words(pk->dst6 + 16 * i, dst);
    uint32_t dport = pk->dport[i], out_port = pk->out_port[i];
    uint32_t svc_group = pk->svc_group ? pk->svc_group[i] : 0u, dest = pk->dest ? pk->dest[i] : 0u;
    uint32_t lb[8], f;
    if (tab) {
      bool collided = false;
      if (read_only)
        f = lb_stage6_aff<true>(svc6, t, now, 0u, uint32_t(i), cols, dst, dport, pk->proto[i], svc_group, out_port, dest, lb, &collided);
      else
        f = lb_stage6_aff(svc6, t, now, seq, uint32_t(i), cols, dst, dport, pk->proto[i], svc_group, out_port, dest, lb, &collided);
      if (!read_only) {
        AffOpsHost::count(ctr + kAffLearned, (f & GPC_LB_LEARNED) != 0u);
        AffOpsHost::count(ctr + kAffHits, (f & (GPC_LB_AFFINITY | GPC_LB_LEARNED)) == GPC_LB_AFFINITY);
        AffOpsHost::count(ctr + kAffOverflow, collided);
      }
    } else {
      f = lb_stage6(
          svc6,
          [&]() {
            uint32_t s[4];
            v6_words(pk->src6 + 16 * i, s);
            return Svc6Src{fold6(s), uint32_t(pk->sport[i])};
          },
          dst, dport, pk->proto[i], svc_group, out_port, dest, lb, source_of(pk, i));
    }
    for (int k = 0; k < 4; k++)
      for (int b = 0; b < 4; b++) dst6_out[16 * i + 4 * k + b] = uint8_t(dst[k] >> (24 - 8 * b));
    dport_out[i] = uint16_t(dport);
    out_port_out[i] = out_port;
    svc_group_out[i] = svc_group;
    dest_out[i] = uint8_t(dest);
    noep[i] = (f & GPC_LB_NO_ENDPOINT) ? 1 : 0;
    if (lb_out) store6(lb, &lb_out[i]);
  }
  return 0;
}
