// rs_rebuild_kernels.hip — the kernels of the general form of rs_rebuild_batch_dev (rs_rebuild.cpp,
// DESIGN.md §3.12): every lost shard of a stripe comes back, recovery shards included.
//
// Per slice of stripes, around the library's own per-stripe reconstruct and encode:
//  * k_rebuild_prepare: one thread per stripe reads its present row and writes the stripe's meta
//    block (rs_internal.hpp rebuild_meta_words: the recovery slots to write, e_o, the restored slot
//    of every original, the missing recovery rows Q) and the final status.
//  * k_rebuild_gather: the stripe's k originals into a packed scratch, shard j from d_original where
//    it is present and from its restored slot of d_rebuilt otherwise. A missing slot of d_original
//    is never read.
//  * k_rebuild_pick: rows Q of the scratch's encode into slots [e_o, min(e_s, max_e)) of d_rebuilt.
// The copies are flattened over (stripe, row, 16 KiB segment), grid-stride, with the access width
// of rs_device_lanes.hpp's three modes: 16-byte vectors, dwords or bytes, by what every buffer,
// stride and shard_bytes allow. A skipped stripe (meta[0] == 0) costs one word per work item.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rs_internal.hpp"

namespace rs {
namespace {

constexpr uint32_t kRebuildSeg = 16384;  // a multiple of 16

__global__ __launch_bounds__(64) void k_rebuild_prepare(const uint8_t *__restrict__ present, uint64_t present_stride,
                                                        uint32_t k, uint32_t m, uint32_t max_e, uint64_t n,
                                                        uint32_t *__restrict__ meta, int32_t *__restrict__ status) {
  const uint64_t s = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const uint8_t *pr = present + s * present_stride;
  uint32_t *mt = meta + s * rebuild_meta_words(k, m);
  uint32_t eo = 0, er = 0;
  for (uint32_t j = 0; j < k; j++) mt[2 + j] = pr[j] ? kRebuildPresent : eo++;
  for (uint32_t r = 0; r < m; r++)
    if (!pr[k + r]) mt[2 + k + er++] = r;
  const uint64_t es = static_cast<uint64_t>(eo) + er;
  if (status) status[s] = es > m ? 2 : (es > max_e ? 14 : 0);
  const uint32_t ne = static_cast<uint32_t>(es < max_e ? es : max_e);
  // fewer than k present: nothing of the stripe; ne <= e_o: no slot is left for a recovery shard
  mt[0] = (es > m || ne <= eo) ? 0u : ne - eo;
  mt[1] = eo;
}

// bytes [lo, hi) of one shard, by the workgroup. MODE 2: lo, hi and both pointers are multiples of
// 16; 1: of 4; 0: anything.
template <int MODE>
__device__ __forceinline__ void copy_range(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, uint64_t lo,
                                           uint64_t hi) {
  if constexpr (MODE == 2) {
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    for (uint64_t b = lo + 16ull * threadIdx.x; b < hi; b += 16ull * 256)
      __builtin_nontemporal_store(__builtin_nontemporal_load(reinterpret_cast<const v4u *>(src + b)),
                                  reinterpret_cast<v4u *>(dst + b));
  } else if constexpr (MODE == 1) {
    for (uint64_t b = lo + 4ull * threadIdx.x; b < hi; b += 4ull * 256)
      *reinterpret_cast<uint32_t *>(dst + b) = *reinterpret_cast<const uint32_t *>(src + b);
  } else {
    for (uint64_t b = lo + threadIdx.x; b < hi; b += 256) dst[b] = src[b];
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void k_rebuild_gather(const uint8_t *__restrict__ orig, uint64_t orig_stride,
                                                        const uint8_t *__restrict__ rebuilt, uint64_t rebuilt_stride,
                                                        uint64_t sb, uint64_t n, uint32_t k, uint64_t mw, uint64_t segs,
                                                        const uint32_t *__restrict__ meta, uint8_t *__restrict__ data) {
  const uint64_t per_stripe = segs * k, total = n * per_stripe;
  for (uint64_t w = blockIdx.x; w < total; w += gridDim.x) {
    const uint64_t s = w / per_stripe, rem = w % per_stripe;
    const uint32_t *mt = meta + s * mw;
    if (mt[0] == 0) continue;
    const uint64_t j = rem / segs, lo = rem % segs * kRebuildSeg, hi = lo + kRebuildSeg < sb ? lo + kRebuildSeg : sb;
    const uint32_t slot = mt[2 + j];
    const uint8_t *src = slot == kRebuildPresent ? orig + s * orig_stride + j * sb
                                                 : rebuilt + s * rebuilt_stride + static_cast<uint64_t>(slot) * sb;
    copy_range<MODE>(src, data + (s * k + j) * sb, lo, hi);
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void k_rebuild_pick(const uint8_t *__restrict__ par, uint64_t sb, uint64_t n,
                                                      uint32_t k, uint32_t m, uint32_t max_e, uint64_t mw, uint64_t segs,
                                                      const uint32_t *__restrict__ meta, uint8_t *__restrict__ rebuilt,
                                                      uint64_t rebuilt_stride) {
  const uint64_t per_stripe = segs * max_e, total = n * per_stripe;
  for (uint64_t w = blockIdx.x; w < total; w += gridDim.x) {
    const uint64_t s = w / per_stripe, rem = w % per_stripe;
    const uint32_t *mt = meta + s * mw;
    const uint64_t i = rem / segs, lo = rem % segs * kRebuildSeg, hi = lo + kRebuildSeg < sb ? lo + kRebuildSeg : sb;
    if (i >= mt[0]) continue;  // e_o + i < max_e and i < e_r from here
    const uint64_t q = mt[2 + k + i];
    copy_range<MODE>(par + (s * m + q) * sb, rebuilt + s * rebuilt_stride + (mt[1] + i) * sb, lo, hi);
  }
}

// 2: 16-byte accesses, 1: dwords, 0: bytes
int copy_mode(std::initializer_list<uint64_t> vals) {
  uint64_t al = 0;
  for (uint64_t v : vals) al |= v;
  return al % 16 == 0 ? 2 : al % 4 == 0 ? 1 : 0;
}

}  // namespace

hipError_t launch_rebuild_prepare(const uint8_t *present, uint64_t present_stride, uint32_t k, uint32_t m,
                                  uint32_t max_e, uint64_t n, uint32_t *meta, int32_t *status, hipStream_t s) {
  if (n == 0) return hipSuccess;
  trace_launch("k_rebuild_prepare");
  hipLaunchKernelGGL(k_rebuild_prepare, dim3(static_cast<uint32_t>((n + 63) / 64)), dim3(64), 0, s, present,
                     present_stride, k, m, max_e, n, meta, status);
  return hipGetLastError();
}

hipError_t launch_rebuild_gather(const uint8_t *orig, uint64_t orig_stride, const uint8_t *rebuilt,
                                 uint64_t rebuilt_stride, uint64_t sb, uint64_t n, uint32_t k, uint32_t m,
                                 const uint32_t *meta, uint8_t *data, hipStream_t s) {
  if (n == 0) return hipSuccess;
  const int mode = copy_mode({reinterpret_cast<uint64_t>(orig), orig_stride, reinterpret_cast<uint64_t>(rebuilt),
                              rebuilt_stride, reinterpret_cast<uint64_t>(data), sb});
  static const char *const kNames[3] = {"k_rebuild_gather_x1", "k_rebuild_gather_x4", "k_rebuild_gather_x16"};
  trace_launch(kNames[mode]);
  const uint64_t segs = (sb + kRebuildSeg - 1) / kRebuildSeg, mw = rebuild_meta_words(k, m);
  const dim3 grid(static_cast<uint32_t>(std::min<uint64_t>(n * segs * k, 1u << 20)));
#define RS_GATHER(MODE_)                                                                                             \
  hipLaunchKernelGGL(k_rebuild_gather<MODE_>, grid, dim3(256), 0, s, orig, orig_stride, rebuilt, rebuilt_stride, sb, n, \
                     k, mw, segs, meta, data)
  if (mode == 2) RS_GATHER(2);
  else if (mode == 1) RS_GATHER(1);
  else RS_GATHER(0);
#undef RS_GATHER
  return hipGetLastError();
}

hipError_t launch_rebuild_pick(const uint8_t *par, uint64_t sb, uint64_t n, uint32_t k, uint32_t m, uint32_t max_e,
                               const uint32_t *meta, uint8_t *rebuilt, uint64_t rebuilt_stride, hipStream_t s) {
  if (n == 0 || max_e == 0) return hipSuccess;
  const int mode =
      copy_mode({reinterpret_cast<uint64_t>(par), reinterpret_cast<uint64_t>(rebuilt), rebuilt_stride, sb});
  static const char *const kNames[3] = {"k_rebuild_pick_x1", "k_rebuild_pick_x4", "k_rebuild_pick_x16"};
  trace_launch(kNames[mode]);
  const uint64_t segs = (sb + kRebuildSeg - 1) / kRebuildSeg, mw = rebuild_meta_words(k, m);
  const dim3 grid(static_cast<uint32_t>(std::min<uint64_t>(n * segs * max_e, 1u << 20)));
#define RS_PICK(MODE_)                                                                                               \
  hipLaunchKernelGGL(k_rebuild_pick<MODE_>, grid, dim3(256), 0, s, par, sb, n, k, m, max_e, mw, segs, meta, rebuilt, \
                     rebuilt_stride)
  if (mode == 2) RS_PICK(2);
  else if (mode == 1) RS_PICK(1);
  else RS_PICK(0);
#undef RS_PICK
  return hipGetLastError();
}

}  // namespace rs
