// Internal launch entry of the classification kernel (classify.hip).
#pragma once

#include <hip/hip_runtime.h>

#include "core.hpp"
#include "gpc.h"

namespace gpc {
// Device pointers of one published epoch (core.hpp View): base image, optional journal.
struct EpochArgs {
  const ImageHdr* hdr;
  const uint32_t* blob;
  const uint32_t* pool;   // journal pool (null: base image alone)
  uint32_t jhdr;          // JournalHdr word offset of this epoch
  const uint32_t* svc;    // null: no Services (AntreaProxy stage skipped)
  uint32_t v6_lpm;        // IPv6 image: word offset of its V6Lpm block (host copy of ImageHdr.v6_lpm)
  uint8_t sort_table[2];  // per policy stage launch: table (1-6) whose scan length groups lanes, 0 = none
  uint32_t ctr_stride;    // per-rule counters: words per copy (counter_cap * kCounterWords)
  uint32_t ctr_mask;      // number of striped copies - 1 (a block updates copy blockIdx & mask)
  uint32_t mode;          // with a pool: kModeExt = only point extensions over the base, else the journal
};
// One packet (index 0 of the device columns) through the table walk with a per-table trace.
int launch_trace(const EpochArgs& ep, const gpc_pkt_soa& pk, uint4* out, uint4* lb_out, TraceStep* steps, uint32_t* n_steps,
                 hipStream_t stream);
// Drains the accumulator copies 0..copies-1 ({packets, bytes, non-session packets} per slot, stride
// words per copy) into the published copy `copies` ({packets, bytes, sessions}): core.hpp count_stage.
int launch_fold_counters(unsigned long long* counters, uint64_t stride, uint32_t copies, hipStream_t stream);
// dst[w] += sum over r < copies of src[r * src_stride + w], w < n_words (device-scope atomics: launches
// on other streams may be adding to dst concurrently). Used when the counter array grows.
int launch_merge_counters(unsigned long long* dst, const unsigned long long* src, uint64_t src_stride, uint32_t copies,
                          uint64_t n_words, hipStream_t stream);
// Packet grouping of a batch (classify.hip group_tiles_kernel): the batch is classified in the
// order of an 8-bit key (scan lengths or address bits) within every tile of 16384 packets, from a grouped copy in
// `scratch` (group_scratch_bytes(pk, n, lb) bytes of device memory, live until the launches have run:
// stream-ordered).
struct GroupArgs {
  uint8_t* scratch;
  uint32_t key;        // GPC_GROUP_KEY_ADDR or GPC_GROUP_KEY_SCAN
  uint32_t axes;       // SCAN: bit a = axis a is read by a sub-index of the image (group_axes)
  uint32_t src_bits;   // ADDR: key = top src_bits of nw_src, then the top 8 - src_bits of nw_dst
  uint32_t xcd_order;  // block order (classify.hip logical_block): 1 = the blocks of one tile run on one XCD
  uint32_t unpermute;  // 1: the ingress launch stores in grouped order, unpermute_kernel restores caller order
  uint32_t lb;         // 1: a Service batch with lb_out: its LB results are un-permuted too (scratch for them)
};
uint64_t group_scratch_bytes(const gpc_pkt_soa& pk, uint64_t n, bool lb);
// Launch timing (gpc_set_launch_timing): an event is recorded on the launch stream before every
// kernel of one gpc_classify* call and after the last, named by the kernel that follows it.
struct LaunchMarks {
  static constexpr int kMax = 16;
  hipEvent_t ev[kMax];
  uint8_t kind[kMax];  // LaunchKind of the kernel starting at ev[i] (kLaunchEnd: the closing event)
  int n;
};
enum LaunchKind : uint8_t {
  kLaunchGroup, kLaunchEgress, kLaunchIngress, kLaunchBoth, kLaunchUnpermute, kLaunchCodes, kLaunchV6Lb, kLaunchAffLearn, kLaunchAffResolve,
  kLaunchAffSweep, kLaunchAff6Learn, kLaunchAff6Resolve, kLaunchAff6Sweep, kLaunchPinCount, kLaunchPinScan, kLaunchPinScatter,
  kLaunchKinds, kLaunchEnd
};
inline void launch_mark(LaunchMarks* m, uint8_t kind, hipStream_t s) {
  if (!m || m->n >= LaunchMarks::kMax) return;
  if (hipEventRecord(m->ev[m->n], s) == hipSuccess) m->kind[m->n++] = kind;
}
// park: with Services (ep.svc), 16 B per packet of device scratch for the fields the Service stage
// rewrites, handed from the egress launch to the ingress launch; null: one launch does both stages.
int launch_classify(const EpochArgs& ep, const gpc_pkt_soa& pk, uint64_t n, gpc_verdict* out, uint4* lb_out,
                    unsigned long long* counters, int count, const GroupArgs* group, hipStream_t stream,
                    LaunchMarks* marks = nullptr, uint4* park = nullptr, bool resolved = false);
// IPv6 batch (pk.src6 / dst6 [/ ct_src6 / ct_dst6]) against the IPv6 image `ep` (base or delta
// epoch): v6_code_kernel maps the addresses to codes in `codes` (v6_code_columns(pk) * n words of
// device memory, live until the launches have run), then launch_classify runs over the code columns
// (`group`: sized by group_scratch_bytes of that IPv4-shaped batch).
// svc6: the IPv6 Service image bound to the epoch (null: none, the launches above and nothing else).
// With it v6_lb_kernel runs first (core.hpp lb_stage6) and writes the columns the Service stage
// rewrites into lb_scratch (v6_lb_scratch_bytes(n) bytes) and the optional LB results (two uint4 per
// packet, gpc_lb_result6) to lb_out6; the code pass then codes {src6, post-DNAT dst6, ct_src6?,
// ct_dst6 or the original dst6}, and the policy launches run as `resolved` over those columns.
// al: svc6 holds session-affinity Services and the slot has an IPv6 affinity table (core.hpp "IPv6
// affinity table"): aff6_learn_kernel and aff6_resolve_kernel run in place of v6_lb_kernel and write
// the same columns; al->done is recorded after them (the next such batch of the slot waits for it).
struct Aff6Launch {
  Aff6Table tab;
  uint32_t now, seq;
  hipEvent_t done;
};
uint32_t v6_code_columns(const gpc_pkt_soa& pk, bool svc = false);
uint64_t v6_lb_scratch_bytes(uint64_t n);
int launch_classify6(const EpochArgs& ep, const gpc_pkt_soa& pk, uint64_t n, gpc_verdict* out,
                     unsigned long long* counters, int count, const GroupArgs* group, uint32_t* codes, hipStream_t stream,
                     LaunchMarks* marks = nullptr, const uint32_t* svc6 = nullptr, uint8_t* lb_scratch = nullptr,
                     uint4* lb_out6 = nullptr, const Aff6Launch* al = nullptr);
// gpc_trace6: packet 0 of the device columns `pk` (src6 / dst6 [/ ct_src6 / ct_dst6], 16-B aligned)
// through the IPv6 epoch `ep` in one launch (classify.hip trace6_kernel): Service stage, LPM coding,
// traced walk.
struct Trace6Args {
  const uint32_t* svc6;  // the IPv6 Service image bound to the epoch (null: none)
  Aff6Table tab;         // tab.w != null: the slot's IPv6 affinity table is read (never written)
  uint32_t now;          // affinity clock
  uint4* out;            // the verdict pair
  uint4* lb_out;         // gpc_lb_result6 (two uint4; all zero: no Service hit)
  uint32_t* codes;       // [0..3] codes of src, dst, ct_src, ct_dst; [4..7] their GPC_T6_* bits
  TraceStep* steps;      // kMaxTraceSteps
  uint32_t* n_steps;
};
int launch_trace6(const EpochArgs& ep, const gpc_pkt_soa& pk, const Trace6Args& t, hipStream_t stream);
// One pass over the IPv6 affinity table's slots (core.hpp aff6_sweep_slot modes).
int launch_aff6_sweep(const Aff6Table& t, uint32_t now, uint32_t mode, hipStream_t stream, LaunchMarks* marks = nullptr);
// IPv4 batch against a Service image with session-affinity Services (ep.svc) and the slot's affinity
// table (core.hpp "Affinity table"): aff_learn_kernel and aff_resolve_kernel run the Service stage
// with the learned flows and write the columns it rewrites into lb_scratch
// (aff_lb_scratch_bytes(n) bytes) and the optional LB results to lb_out; `done` is recorded after
// them (the next affinity batch of the slot waits for it); the policy launches then run as
// `resolved` over those columns with ct_dst = the caller's column or the original dst (`group`:
// sized for a batch that has ct_dst, svc_group and dest columns). out == null: the stage alone;
// *rewritten (optional) = the batch as the policy launches read it.
// read_only (gpc_trace): no learn pass, the table is only read.
struct AffLaunch {
  AffTable tab;
  uint32_t now, seq, read_only;
  uint8_t* lb_scratch;
  hipEvent_t done;
};
uint64_t aff_lb_scratch_bytes(uint64_t n);
// One pass over the table's slots (core.hpp aff_sweep_slot modes), in front of a learn pass on the
// same stream or on its own.
int launch_aff_sweep(const AffTable& t, uint32_t now, uint32_t mode, hipStream_t stream, LaunchMarks* marks = nullptr);
int launch_classify_aff(const EpochArgs& ep, const gpc_pkt_soa& pk, uint64_t n, gpc_verdict* out, uint4* lb_out,
                        unsigned long long* counters, int count, const GroupArgs* group, hipStream_t stream,
                        LaunchMarks* marks, const AffLaunch& al, gpc_pkt_soa* rewritten = nullptr);
// Packet-in collection (packetin.hip): an ordered stream compaction of the batch's controller-bound
// records (core.hpp pin_records over the verdict pairs `out` and the epoch's packet-in image `img`,
// null: none) in three launches on `stream` -- pin_count_kernel (per wave the two lane masks, per
// tile of kPinTile packets the record count), pin_scan_kernel (one workgroup: exclusive 64-bit scan
// of the tile counts, the total to *count), pin_scatter_kernel (records[position] for positions
// < cap). No workgroup waits for another and nothing is atomic: the order is the packet order.
// scratch: pin_scratch_bytes(n) bytes, 16-byte aligned. n > 0.
uint64_t pin_scratch_bytes(uint64_t n);
int launch_pin(const uint32_t* img, const gpc_verdict* out, uint64_t n, gpc_packet_in* records, uint64_t cap,
               unsigned long long* count, void* scratch, hipStream_t stream, LaunchMarks* marks);
}
