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
//    S_r == mul(S_0, c[r][j] / c[0][j]) on Sym<NV> registers with the v_perm multiply; a wave that
//    sees a difference stores 1 to the stripe's reject byte. A stripe that is no candidate costs
//    one load of its class per work item.
//  * k_locate_finish: d_located, the d_present rows, d_counts.
// A kernel boundary separates every producer from its consumers (no hand-off inside a kernel).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rs_device.hpp"
#include "rs_device_lanes.hpp"
#include "rs_internal.hpp"

namespace rs {
namespace {

using dev::build_tab;
using dev::Lanes;
using dev::ld_xor;
using dev::ld_xor_tail;
using dev::Sym;
using dev::Tab;

constexpr uint32_t kLocateSeg = 16384;  // as k_verify_compare: a multiple of 16 and of 64
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
    for (uint64_t base = 0; base < sb; base += kLocateSeg) {
      const uint32_t len = static_cast<uint32_t>(sb - base < kLocateSeg ? sb - base : kLocateSeg);
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
      const uint64_t o = sh_pos, t = sb % 64, whole = sb - t, h = t / 2;
      uint64_t lo, hi;  // the byte offsets of the symbol that byte o belongs to
      if (o < whole) {
        lo = o / 64 * 64 + o % 32;
        hi = lo + 32;
      } else {
        lo = whole + (o - whole) % h;
        hi = lo + h;
      }
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
// Work item = (stripe, group of up to kLocateRows rows r >= 1, segment). S_0 of the lane's unit
// stays in registers while the group's rows pass; the table of (stripe, r) is wave-uniform.
constexpr uint32_t kLocateRows = 16;

template <int MODE>
__global__ __launch_bounds__(256) void k_locate_confirm(const uint8_t *__restrict__ enc, uint64_t enc_stride,
                                                        const uint8_t *__restrict__ rec, uint64_t rec_stride,
                                                        uint64_t sb, uint64_t n, uint32_t k, uint32_t m, uint64_t segs,
                                                        uint32_t groups, const int32_t *__restrict__ cls,
                                                        const RsTab *__restrict__ tabs, uint8_t *reject) {
  constexpr int NV = Lanes<MODE>::NV;
  constexpr uint32_t kUnitsPerChunk = 8 / NV, kLo = 4 * NV;  // a unit: kLo low + kLo high bytes of one chunk
  const uint64_t per_stripe = segs * groups, total = n * per_stripe;
  const uint32_t t = static_cast<uint32_t>(sb % 64);
  const uint64_t whole = sb - t;
  const uint32_t tid = threadIdx.x;
  for (uint64_t w = blockIdx.x; w < total; w += gridDim.x) {
    const uint64_t s = w / per_stripe, rem = w % per_stripe;
    const int32_t cand = cls[s];
    if (cand < 0 || static_cast<uint32_t>(cand) >= k) continue;  // no candidate: nothing to read
    if (*static_cast<volatile uint8_t *>(reject + s)) continue;  // already rejected (a stale 0 only costs time)
    const uint32_t g = static_cast<uint32_t>(rem / segs);
    const uint64_t seg = rem % segs, base = seg * kLocateSeg;
    const uint32_t r_lo = 1 + g * kLocateRows, r_hi = min(m, r_lo + kLocateRows);
    const uint8_t *pa = enc + s * enc_stride + base, *pb = rec + s * rec_stride + base;
    const RsTab *tb = tabs + s * (m - 1);
    const uint32_t wb = base < whole ? static_cast<uint32_t>(whole - base < kLocateSeg ? whole - base : kLocateSeg) : 0;
    const uint32_t units = wb / 64 * kUnitsPerChunk;
    uint32_t d = 0;
    // the loop bounds are workgroup-uniform (a lane past the end re-reads unit 0 and drops the
    // result), so the table loads stay scalar
    for (uint32_t u0 = 0; u0 < units; u0 += 256u) {
      const bool live = u0 + tid < units;
      const uint32_t u = live ? u0 + tid : 0;
      const uint32_t off = u / kUnitsPerChunk * 64 + u % kUnitsPerChunk * kLo;
      Sym<NV> s0, sr;
      ld_xor<MODE>(s0, pa + off, pb + off);
      ld_xor<MODE>(sr, pa + r_lo * sb + off, pb + r_lo * sb + off);
      uint32_t dd = 0;
      for (uint32_t r = r_lo; r < r_hi; r++) {
        Sym<NV> next = sr, pr;
        // the next row's loads are in flight while this row is multiplied
        if (r + 1 < r_hi) ld_xor<MODE>(next, pa + (r + 1) * sb + off, pb + (r + 1) * sb + off);
        const Tab tab = dev::load_tab(tb + (r - 1));
        dev::zero(pr);
        dev::mul_add(pr, s0, tab);
#pragma unroll
        for (int v = 0; v < NV; v++) dd |= (pr.l[v] ^ sr.l[v]) | (pr.h[v] ^ sr.h[v]);
        sr = next;
      }
      d |= live ? dd : 0u;
    }
    if (t != 0 && seg == segs - 1) {  // the tail chunk, bytes (wave 0: lanes 0-7 hold its symbols)
      const uint8_t *ta = enc + s * enc_stride + whole, *tbp = rec + s * rec_stride + whole;
      if (tid < 64) {
        const uint32_t lane = tid < 8 ? tid : 0, h = t / 2;
        Sym<1> s0;
        ld_xor_tail(s0, ta, tbp, h, lane);
        uint32_t dd = 0;
        for (uint32_t r = r_lo; r < r_hi; r++) {
          Sym<1> sr, pr;
          ld_xor_tail(sr, ta + r * sb, tbp + r * sb, h, lane);
          const Tab tab = dev::load_tab(tb + (r - 1));
          dev::zero(pr);
          dev::mul_add(pr, s0, tab);
          dd |= (pr.l[0] ^ sr.l[0]) | (pr.h[0] ^ sr.h[0]);
        }
        d |= tid < 8 ? dd : 0u;
      }
    }
    if (__builtin_amdgcn_ballot_w64(d != 0u) != 0ull && (tid & 63u) == 0u) reject[s] = 1;
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

// 2: 16-byte loads, 1: dwords, 0: bytes — what both buffers, both strides and sb allow
int load_mode(const uint8_t *a, uint64_t a_stride, const uint8_t *b, uint64_t b_stride, uint64_t sb) {
  const uint64_t al = reinterpret_cast<uint64_t>(a) | reinterpret_cast<uint64_t>(b) | a_stride | b_stride | sb;
  return al % 16 == 0 ? 2 : al % 4 == 0 ? 1 : 0;
}

}  // namespace

hipError_t launch_locate_classify(const uint8_t *enc, uint64_t enc_stride, const uint8_t *rec, uint64_t rec_stride,
                                  uint64_t sb, uint64_t n, uint32_t k, uint32_t m, const uint8_t *bad,
                                  const uint16_t *rlog, const uint16_t *dl, const uint16_t *d_exp,
                                  const uint16_t *d_log, RsTab *tabs, int32_t *cls, hipStream_t s) {
  if (n == 0) return hipSuccess;
  trace_launch("k_locate_classify");
  const dim3 grid(static_cast<uint32_t>(std::min<uint64_t>(n, 1u << 20)));
  switch (load_mode(enc, enc_stride, rec, rec_stride, sb)) {
    case 2:
      hipLaunchKernelGGL(k_locate_classify<2>, grid, dim3(256), 0, s, enc, enc_stride, rec, rec_stride, sb, n, k, m,
                         bad, rlog, dl, d_exp, d_log, tabs, cls);
      break;
    case 1:
      hipLaunchKernelGGL(k_locate_classify<1>, grid, dim3(256), 0, s, enc, enc_stride, rec, rec_stride, sb, n, k, m,
                         bad, rlog, dl, d_exp, d_log, tabs, cls);
      break;
    default:
      hipLaunchKernelGGL(k_locate_classify<0>, grid, dim3(256), 0, s, enc, enc_stride, rec, rec_stride, sb, n, k, m,
                         bad, rlog, dl, d_exp, d_log, tabs, cls);
  }
  return hipGetLastError();
}

hipError_t launch_locate_confirm(const uint8_t *enc, uint64_t enc_stride, const uint8_t *rec, uint64_t rec_stride,
                                 uint64_t sb, uint64_t n, uint32_t k, uint32_t m, const int32_t *cls,
                                 const RsTab *tabs, uint8_t *reject, hipStream_t s) {
  if (n == 0 || m < 2) return hipSuccess;
  trace_launch("k_locate_confirm");
  const uint64_t segs = (sb + kLocateSeg - 1) / kLocateSeg;
  const uint32_t groups = (m - 1 + kLocateRows - 1) / kLocateRows;
  const dim3 grid(static_cast<uint32_t>(std::min<uint64_t>(n * segs * groups, 1u << 20)));
  switch (load_mode(enc, enc_stride, rec, rec_stride, sb)) {
    case 2:
      hipLaunchKernelGGL(k_locate_confirm<2>, grid, dim3(256), 0, s, enc, enc_stride, rec, rec_stride, sb, n, k, m,
                         segs, groups, cls, tabs, reject);
      break;
    case 1:
      hipLaunchKernelGGL(k_locate_confirm<1>, grid, dim3(256), 0, s, enc, enc_stride, rec, rec_stride, sb, n, k, m,
                         segs, groups, cls, tabs, reject);
      break;
    default:
      hipLaunchKernelGGL(k_locate_confirm<0>, grid, dim3(256), 0, s, enc, enc_stride, rec, rec_stride, sb, n, k, m,
                         segs, groups, cls, tabs, reject);
  }
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
