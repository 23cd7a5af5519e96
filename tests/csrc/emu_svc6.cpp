// TEST-ONLY host run of the IPv6 Service stage (core.hpp lb_stage6, the body of classify.hip
// v6_lb_kernel) over the IPv6 Service image the product library built (gpc_debug_service_image6).
// Writes the columns the stage rewrites; the caller then runs the existing IPv6 emulation
// (emu.cpp emu_classify6) on them. Never linked into libgpc.so.
#include <cstddef>
#include <cstdint>

#include "core.hpp"
#include "gpc.h"

using namespace gpc;

// dst6_out: n x 16 network-order bytes; lb_out: n gpc_lb_result6 (may be null); noep: n flags.
extern "C" int emu_lb6(const uint32_t* svc6, const gpc_pkt_soa* pk, size_t n, uint8_t* dst6_out, uint16_t* dport_out,
                       uint32_t* out_port_out, uint32_t* svc_group_out, uint8_t* dest_out, gpc_lb_result6* lb_out,
                       uint8_t* noep) {
  for (size_t i = 0; i < n; i++) {
    uint32_t dst[4];
    v6_words(pk->dst6 + 16 * i, dst);
    uint32_t dport = pk->dport[i];
    uint32_t out_port = pk->out_port[i], svc_group = pk->svc_group ? pk->svc_group[i] : 0u;
    uint32_t dest = pk->dest ? pk->dest[i] : 0u;
    uint32_t lb[8];
    const uint32_t f = lb_stage6(
        svc6,
        [&]() {
          uint32_t s[4];
          v6_words(pk->src6 + 16 * i, s);
          return Svc6Src{fold6(s), uint32_t(pk->sport[i])};
        },
        dst, dport, pk->proto[i], svc_group, out_port, dest, lb);
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
