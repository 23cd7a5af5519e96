// Packet-in collection (gfx950): the controller-bound records of a classified batch, compacted in
// packet order behind the classify launches (launch.hpp launch_pin; core.hpp pin_records).
//
// Three launches on the caller's stream, wave64 throughout:
//   pin_count_kernel    one lane per packet, one workgroup per tile of kPinTile packets: each lane
//                       loads its verdict pair (16 B) and evaluates pin_records; two ballots per wave
//                       (egress record, ingress record) go to the scratch as one 16-B store, the
//                       popcounts are summed through LDS into the tile's count;
//   pin_scan_kernel     one workgroup: exclusive scan of the tile counts, in place and in 64 bits,
//                       the grand total to *count;
//   pin_scatter_kernel  same grid as the count pass: a wave's base is its tile's offset plus the counts
//                       of the earlier waves of the tile (LDS), a lane's rank the set bits of both masks
//                       below it; only lanes with a record load their verdict again and store.
// No workgroup waits for another inside a launch (the stream orders the passes), nothing is atomic,
// and the output order is the packet order, egress before ingress.
// Scratch: waves x {egress mask, ingress mask} (uint64 each), then tiles x uint64 counts / offsets.
#include <hip/hip_runtime.h>

#include "launch.hpp"

namespace gpc {
namespace {

constexpr uint32_t kPinWaves = kPinTile / 64;
static_assert(kPinTile % 64 == 0 && kPinTile <= 1024, "a tile is one workgroup of whole waves");
static_assert(sizeof(gpc_packet_in) == 16 && sizeof(PinRec) == 16, "one 128-bit store per record");

__device__ __forceinline__ uint32_t lane_records(const uint32_t* img, const uint4* out, uint64_t i, PinRec r[2]) {
  const uint4 q = out[i];
  const uint32_t v[4] = {q.x, q.y, q.z, q.w};
  return pin_records(uint32_t(i), v, img, r);
}

__global__ __launch_bounds__(kPinTile) void pin_count_kernel(const uint32_t* __restrict__ img, const uint4* __restrict__ out,
                                                             uint64_t n, ulonglong2* __restrict__ masks,
                                                             unsigned long long* __restrict__ tiles) {
  __shared__ uint32_t wcnt[kPinWaves];
  const uint64_t i = uint64_t(blockIdx.x) * kPinTile + threadIdx.x;
  const uint32_t wave = threadIdx.x >> 6;
  uint32_t m = 0;
  if (i < n) {
    PinRec r[2];
    m = lane_records(img, out, i, r);
  }
  const unsigned long long b0 = __ballot(m & 1u), b1 = __ballot(m & 2u);
  if ((threadIdx.x & 63u) == 0) {
    // (waves past the batch's end have no mask slot: the scratch holds ceil(n / 64) of them)
    if (i < n) masks[uint64_t(blockIdx.x) * kPinWaves + wave] = make_ulonglong2(b0, b1);
    wcnt[wave] = uint32_t(__popcll(b0) + __popcll(b1));
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
#pragma unroll
    for (uint32_t w = 0; w < kPinWaves; w++) t += wcnt[w];
    tiles[blockIdx.x] = t;
  }
}

constexpr uint32_t kScanBlock = 1024, kScanWaves = kScanBlock / 64;

// In place: tiles[t] = sum of tiles[0..t), *count = the sum of all; rounds of kScanBlock tiles with a
// running carry (a wave scans its 64 values with shuffles, the wave totals meet in LDS; the LDS
// array alternates between rounds, so one barrier per round is enough).
__global__ __launch_bounds__(kScanBlock) void pin_scan_kernel(unsigned long long* __restrict__ tiles, uint64_t n_tiles,
                                                              unsigned long long* __restrict__ count) {
  __shared__ unsigned long long wsum[2][kScanWaves];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  unsigned long long carry = 0;
  uint32_t par = 0;
  for (uint64_t base = 0; base < n_tiles; base += kScanBlock, par ^= 1u) {
    const uint64_t t = base + threadIdx.x;
    const unsigned long long own = t < n_tiles ? tiles[t] : 0ull;
    unsigned long long x = own;  // inclusive scan over the wave
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
      const unsigned long long y = __shfl_up(x, d, 64);
      if (lane >= d) x += y;
    }
    if (lane == 63) wsum[par][wave] = x;
    __syncthreads();
    unsigned long long before = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < kScanWaves; w++) {
      const unsigned long long s = wsum[par][w];
      before += w < wave ? s : 0ull;
      all += s;
    }
    if (t < n_tiles) tiles[t] = carry + before + x - own;
    carry += all;
  }
  if (threadIdx.x == 0) *count = carry;
}

__global__ __launch_bounds__(kPinTile) void pin_scatter_kernel(const uint32_t* __restrict__ img, const uint4* __restrict__ out,
                                                               uint64_t n, const ulonglong2* __restrict__ masks,
                                                               const unsigned long long* __restrict__ tiles,
                                                               uint4* __restrict__ records, uint64_t cap) {
  __shared__ uint32_t wcnt[kPinWaves];
  const uint64_t i = uint64_t(blockIdx.x) * kPinTile + threadIdx.x;
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  // the wave's first packet decides whether it has a mask slot (wave-uniform)
  const bool has = i - lane < n;
  const ulonglong2 mk = has ? masks[uint64_t(blockIdx.x) * kPinWaves + wave] : make_ulonglong2(0ull, 0ull);
  if (lane == 0) wcnt[wave] = uint32_t(__popcll(mk.x) + __popcll(mk.y));
  __syncthreads();
  const uint32_t mine = uint32_t((mk.x >> lane) & 1ull) | uint32_t((mk.y >> lane) & 1ull) << 1;
  if (!mine || i >= n) return;
  uint64_t pos = tiles[blockIdx.x];
  for (uint32_t w = 0; w < wave; w++) pos += wcnt[w];
  const unsigned long long below = (1ull << lane) - 1ull;
  pos += uint32_t(__popcll(mk.x & below) + __popcll(mk.y & below));
  PinRec r[2];
  (void)lane_records(img, out, i, r);
  if (mine & 1u) {
    if (pos < cap) records[pos] = make_uint4(r[0].w[0], r[0].w[1], r[0].w[2], r[0].w[3]);
    pos++;
  }
  if ((mine & 2u) && pos < cap) records[pos] = make_uint4(r[1].w[0], r[1].w[1], r[1].w[2], r[1].w[3]);
}

}  // namespace

uint64_t pin_scratch_bytes(uint64_t n) {
  const uint64_t waves = (n + 63) / 64, tiles = (n + kPinTile - 1) / kPinTile;
  return waves * 16 + ((tiles * 8 + 15) & ~uint64_t(15));
}

int launch_pin(const uint32_t* img, const gpc_verdict* out, uint64_t n, gpc_packet_in* records, uint64_t cap,
               unsigned long long* count, void* scratch, hipStream_t stream, LaunchMarks* marks) {
  if (n == 0 || n > GPC_MAX_BATCH) return -GPC_EINVAL;
  const uint64_t waves = (n + 63) / 64, tiles = (n + kPinTile - 1) / kPinTile;
  ulonglong2* const masks = static_cast<ulonglong2*>(scratch);
  unsigned long long* const tcnt = reinterpret_cast<unsigned long long*>(masks + waves);
  const uint4* const v = reinterpret_cast<const uint4*>(out);
  // the closing event of the classify launches is the opening event of the count pass
  if (marks && marks->n > 0 && marks->kind[marks->n - 1] == kLaunchEnd) marks->kind[marks->n - 1] = kLaunchPinCount;
  else launch_mark(marks, kLaunchPinCount, stream);
  hipLaunchKernelGGL(pin_count_kernel, dim3(uint32_t(tiles)), dim3(kPinTile), 0, stream, img, v, n, masks, tcnt);
  launch_mark(marks, kLaunchPinScan, stream);
  hipLaunchKernelGGL(pin_scan_kernel, dim3(1), dim3(kScanBlock), 0, stream, tcnt, tiles, count);
  launch_mark(marks, kLaunchPinScatter, stream);
  hipLaunchKernelGGL(pin_scatter_kernel, dim3(uint32_t(tiles)), dim3(kPinTile), 0, stream, img, v, n, masks, tcnt,
                     reinterpret_cast<uint4*>(records), cap);
  launch_mark(marks, kLaunchEnd, stream);
  return hipGetLastError() == hipSuccess ? 0 : -GPC_EDEV;
}

}  // namespace gpc
