// rs_locate_kernels.hip — the kernels of rs_locate_batch_dev (rs_locate.cpp):
// which single shard explains a stripe whose stored recovery shards disagree with its originals.
//
// Inputs per slice of stripes: enc = the encode of the originals ([n][m][sb], rs_encode_batch_dev
// into a scratch), rec = the stored recovery shards, bad = k_verify_compare's flags [n][m]. The
// syndrome of recovery row r is S_r = enc[r] ^ rec[r], symbol by symbol. Under the corrected
// arithmetic the encode is linear over GF(2^16) with nonzero coefficients c[r][j], so one corrupt
// original j with error err gives S_r = c[r][j] * err for every r, and the ratio c[1][j] / c[0][j]
// names j (the ratios are distinct: every 2 x 2 minor of an MDS code's c is nonzero).
//  * k_locate_classify: one workgroup per stripe counts the flags. Fewer than m set: the class is
//    final and no shard data is read. All m set: scan S_0 for a nonzero byte, take the symbol it
//    belongs to, look log S_1 - log S_0 up among the code's k ratio logs (one j per lane), and
//    build the candidate's m - 1 multiply tables c[r][j] / c[0][j] from their logs.
//  * k_locate_confirm: flattened over (stripe, row group, 16 KiB segment), grid-stride; checks
//    S_r == mul(S_0, c[r][j] / c[0][j]) with dev::span_check (rs_device_span.hpp: one pivot row,
//    row 0, rows from 1, no position wanted); a wave that sees a difference stores 1 to the
//    stripe's reject byte. A stripe that is no candidate costs one load of its class per work item.
//  * k_locate_finish: d_located, the d_present rows, d_counts.
// A kernel boundary separates every producer from its consumers (no hand-off inside a kernel).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rs_device.hpp"
#include "rs_device_lanes.hpp"
#include "rs_device_span.hpp"
#include "rs_internal.hpp"

namespace rs {
namespace {

using dev::build_tab;
using dev::kRows;
using dev::kSeg;

constexpr uint32_t kNoLog = 0xFFFFFFFFu;

// ============================================================ classify + candidate
// cls[s]: kLocClean / kLocRecoverySet / kLocUnlocated, k + r (one recovery shard disagrees), or a
// candidate original j in [0, k) that k_locate_confirm still has to check; its tables go to
// tabs[s][0, m - 1). rlog[k] = log(c[1][j] / c[0][j]); dl[k][m - 1] = log(c[r][j] / c[0][j]), r >= 1.
template <int MODE>
__global__ __launch_bounds__(256) void k_locate_classify(
    const uint8_t *__restrict__ enc, uint64_t enc_stride, const uint8_t *__restrict__ rec, uint64_t rec_stride,
    uint64_t sb, uint64_t n, uint32_t k, uint32_t m, const uint8_t *__restrict__ bad,
    const uint16_t *__restrict__ rlog, const uint16_t *__restrict__ dl, const uint16_t *__restrict__ d_exp,
    const uint16_t *__restrict__ d_log, RsTab *__restrict__ tabs, int32_t *__restrict__ cls) {
  __shared__ uint32_t sh_cnt, sh_first, sh_dlog;
  __shared__ int32_t sh_cand;
  __shared__ unsigned long long sh_pos;
  const uint32_t tid = threadIdx.x;
  for (uint64_t s = blockIdx.x; s < n; s += gridDim.x) {
    __syncthreads();  // the previous stripe's shared words are no longer read
    if (tid == 0) {
      sh_cnt = 0;
      sh_first = 0xFFFFFFFFu;
      sh_dlog = kNoLog;
      sh_cand = -1;
      sh_pos = ~0ull;
    }
    __syncthreads();
    uint32_t c = 0, first = 0xFFFFFFFFu;
    for (uint32_t r = tid; r < m; r += 256u)
      if (bad[s * m + r]) {
        c++;
        first = first < r ? first : r;
      }
    if (c) {
      atomicAdd(&sh_cnt, c);
      atomicMin(&sh_first, first);
    }
    __syncthreads();
    const uint32_t cnt = sh_cnt;  // workgroup-uniform from here
    if (cnt < m || m < 2) {
      if (tid == 0)
        cls[s] = cnt == 0               ? kLocClean
                 : m < 2                ? kLocUnlocated
                 : cnt == 1             ? static_cast<int32_t>(k + sh_first)
                                        : kLocRecoverySet;
      continue;
    }
    // every row disagrees: a byte where S_0 is nonzero (the lowest offset of the first segment
    // that has one)
    const uint8_t *pa = enc + s * enc_stride, *pb = rec + s * rec_stride;
    for (uint64_t base = 0; base < sb; base += kSeg) {
      const uint32_t len = static_cast<uint32_t>(sb - base < kSeg ? sb - base : kSeg);
      const uint8_t *qa = pa + base, *qb = pb + base;
      uint32_t at = 0xFFFFFFFFu;
      if (MODE == 2) {
        typedef uint32_t v4u __attribute__((ext_vector_type(4)));
        // a segment is 4 passes of the workgroup: all 8 loads of a lane are issued before any is
        // looked at (a pass past the end re-reads offset 0 and drops the result; len >= 16 here)
        v4u x[4], y[4];
        bool in[4];
#pragma unroll
        for (uint32_t u = 0; u < 4; u++) {
          const uint32_t i = tid * 16u + u * 4096u;
          in[u] = i + 16u <= len;
          x[u] = __builtin_nontemporal_load(reinterpret_cast<const v4u *>(qa + (in[u] ? i : 0u)));
          y[u] = __builtin_nontemporal_load(reinterpret_cast<const v4u *>(qb + (in[u] ? i : 0u)));
        }
#pragma unroll
        for (int u = 3; u >= 0; u--)
#pragma unroll
          for (int v = 3; v >= 0; v--) {
            const uint32_t d = x[u][v] ^ y[u][v];
            if (d && in[u]) at = min(at, tid * 16u + u * 4096u + 4u * v + (static_cast<uint32_t>(__builtin_ctz(d)) >> 3));
          }
      } else if (MODE == 1) {
        for (uint32_t i = tid * 4u; i + 4u <= len; i += 256u * 4u) {
          const uint32_t d = *reinterpret_cast<const uint32_t *>(qa + i) ^ *reinterpret_cast<const uint32_t *>(qb + i);
          if (d) at = min(at, i + (static_cast<uint32_t>(__builtin_ctz(d)) >> 3));
        }
      } else {
        for (uint32_t i = tid; i < len; i += 256u)
          if (qa[i] != qb[i]) at = min(at, i);
      }
      if (at != 0xFFFFFFFFu) atomicMin(&sh_pos, static_cast<unsigned long long>(base + at));
      if (__syncthreads_or(at != 0xFFFFFFFFu)) break;
    }
    __syncthreads();
    if (tid == 0 && sh_pos != ~0ull) {
      uint64_t lo, hi;  // the byte offsets of the symbol that byte sh_pos belongs to
      dev::symbol_bytes(sb, dev::symbol_of(sb, sh_pos), lo, hi);
      const uint32_t s0 = static_cast<uint32_t>(pa[lo] ^ pb[lo]) | static_cast<uint32_t>(pa[hi] ^ pb[hi]) << 8;
      const uint32_t s1 = static_cast<uint32_t>(pa[sb + lo] ^ pb[sb + lo]) |
                          static_cast<uint32_t>(pa[sb + hi] ^ pb[sb + hi]) << 8;
      if (s0 != 0 && s1 != 0) sh_dlog = (static_cast<uint32_t>(d_log[s1]) + kModulus - d_log[s0]) % kModulus;
    }
    __syncthreads();
    const uint32_t want = sh_dlog;
    if (want != kNoLog)
      for (uint32_t j = tid; j < k; j += 256u)
        if (rlog[j] == want) sh_cand = static_cast<int32_t>(j);  // the ratios are distinct: one writer
    __syncthreads();
    const int32_t cand = sh_cand;
    if (tid == 0) cls[s] = cand < 0 ? kLocUnlocated : cand;
    if (cand >= 0)
      for (uint32_t r1 = tid; r1 < m - 1; r1 += 256u)
        build_tab(tabs + s * (m - 1) + r1, dl[static_cast<uint64_t>(cand) * (m - 1) + r1], d_exp, d_log);
  }
}

// ======================================================================= confirm
// Work item = (stripe, group of up to kRows rows r >= 1, segment): dev::span_check with the one
// pivot row 0, whose S_0 stays in registers while the group's rows pass; the table of (stripe, r)
// is tabs[s][r - 1].
template <int MODE>
__global__ __launch_bounds__(256) void k_locate_confirm(const uint8_t *__restrict__ enc, uint64_t enc_stride,
                                                        const uint8_t *__restrict__ rec, uint64_t rec_stride,
                                                        uint64_t sb, uint64_t n, uint32_t k, uint32_t m, uint64_t segs,
                                                        uint32_t groups, const int32_t *__restrict__ cls,
                                                        const RsTab *__restrict__ tabs, uint8_t *reject) {
  const uint64_t per_stripe = segs * groups, total = n * per_stripe;
  const uint32_t piv[1] = {0};
  for (uint64_t w = blockIdx.x; w < total; w += gridDim.x) {
    const uint64_t s = w / per_stripe, rem = w % per_stripe;
    const int32_t cand = cls[s];
    if (cand < 0 || static_cast<uint32_t>(cand) >= k) continue;  // no candidate: nothing to read
    if (*static_cast<volatile uint8_t *>(reject + s)) continue;  // already rejected (a stale 0 only costs time)
    const uint32_t g = static_cast<uint32_t>(rem / segs);
    const uint32_t r_lo = 1 + g * kRows, r_hi = min(m, r_lo + kRows);
    const RsTab *tb = tabs + s * (m - 1);
    const uint32_t at = dev::span_check<MODE, 1, false>(enc + s * enc_stride, rec + s * rec_stride, sb, rem % segs, segs,
                                                        r_lo, r_hi, piv, nullptr,
                                                        [&](int, uint32_t r) { return tb + (r - 1); });
    if (__builtin_amdgcn_ballot_w64(at != dev::kNoSym) != 0ull && (threadIdx.x & 63u) == 0u) reject[s] = 1;
  }
}

// ======================================================================== finish
// One thread per (stripe, byte of its present row) — or per stripe without d_present. A candidate
// whose confirm was rejected becomes kLocUnlocated. counts[4] (zeroed by the host): clean,
// single shard, recovery set, unlocated.
__global__ __launch_bounds__(256) void k_locate_finish(const int32_t *__restrict__ cls,
                                                       const uint8_t *__restrict__ bad,
                                                       const uint8_t *__restrict__ reject, uint32_t k, uint32_t m,
                                                       uint64_t n, int32_t *__restrict__ located,
                                                       uint8_t *__restrict__ present, uint64_t present_stride,
                                                       unsigned long long *counts) {
  __shared__ uint32_t part[4];
  if (threadIdx.x < 4) part[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t row = present ? static_cast<uint64_t>(k) + m : 1, total = n * row;
  for (uint64_t g = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; g < total;
       g += static_cast<uint64_t>(gridDim.x) * 256u) {
    const uint64_t s = g / row, i = g % row;
    int32_t loc = cls[s];
    if (loc >= 0 && static_cast<uint32_t>(loc) < k && reject[s]) loc = kLocUnlocated;
    if (i == 0) {
      located[s] = loc;
      if (counts) atomicAdd(&part[loc >= 0 ? 1 : loc == kLocClean ? 0 : loc == kLocRecoverySet ? 2 : 3], 1u);
    }
    if (present) {
      uint8_t v = 1;
      if (loc >= 0) v = i != static_cast<uint64_t>(loc);
      else if (loc == kLocRecoverySet && i >= k) v = bad[s * m + (i - k)] == 0;
      present[s * present_stride + i] = v;
    }
  }
  __syncthreads();
  if (counts && threadIdx.x < 4 && part[threadIdx.x])
    atomicAdd(counts + threadIdx.x, static_cast<unsigned long long>(part[threadIdx.x]));
}

}  // namespace

hipError_t launch_locate_classify(const uint8_t *enc, uint64_t enc_stride, const uint8_t *rec, uint64_t rec_stride,
                                  uint64_t sb, uint64_t n, uint32_t k, uint32_t m, const uint8_t *bad,
                                  const uint16_t *rlog, const uint16_t *dl, const uint16_t *d_exp,
                                  const uint16_t *d_log, RsTab *tabs, int32_t *cls, hipStream_t s) {
  if (n == 0) return hipSuccess;
  trace_launch("k_locate_classify");
  const dim3 grid(static_cast<uint32_t>(std::min<uint64_t>(n, 1u << 20)));
  with_int(load_mode(enc, enc_stride, rec, rec_stride, sb), kModes, [&](auto mode) {
    hipLaunchKernelGGL(k_locate_classify<decltype(mode)::value>, grid, dim3(256), 0, s, enc, enc_stride, rec,
                       rec_stride, sb, n, k, m, bad, rlog, dl, d_exp, d_log, tabs, cls);
  });
  return hipGetLastError();
}

hipError_t launch_locate_confirm(const uint8_t *enc, uint64_t enc_stride, const uint8_t *rec, uint64_t rec_stride,
                                 uint64_t sb, uint64_t n, uint32_t k, uint32_t m, const int32_t *cls,
                                 const RsTab *tabs, uint8_t *reject, hipStream_t s) {
  if (n == 0 || m < 2) return hipSuccess;
  trace_launch("k_locate_confirm");
  const uint64_t segs = (sb + kSeg - 1) / kSeg;
  const uint32_t groups = (m - 1 + kRows - 1) / kRows;
  const dim3 grid(static_cast<uint32_t>(std::min<uint64_t>(n * segs * groups, 1u << 20)));
  with_int(load_mode(enc, enc_stride, rec, rec_stride, sb), kModes, [&](auto mode) {
    hipLaunchKernelGGL(k_locate_confirm<decltype(mode)::value>, grid, dim3(256), 0, s, enc, enc_stride, rec,
                       rec_stride, sb, n, k, m, segs, groups, cls, tabs, reject);
  });
  return hipGetLastError();
}

hipError_t launch_locate_finish(const int32_t *cls, const uint8_t *bad, const uint8_t *reject, uint32_t k, uint32_t m,
                                uint64_t n, int32_t *located, uint8_t *present, uint64_t present_stride,
                                uint64_t *counts, hipStream_t s) {
  if (n == 0) return hipSuccess;
  trace_launch("k_locate_finish");
  const uint64_t total = n * (present ? static_cast<uint64_t>(k) + m : 1);
  const uint64_t blocks = std::min<uint64_t>((total + 255) / 256, 1u << 16);
  hipLaunchKernelGGL(k_locate_finish, dim3(static_cast<uint32_t>(blocks)), dim3(256), 0, s, cls, bad, reject, k, m, n,
                     located, present, present_stride, reinterpret_cast<unsigned long long *>(counts));
  return hipGetLastError();
}

}  // namespace rs
