// rs_locate_multi_kernels.hip — the kernels of rs_locate_multi_batch_dev (rs_locate_multi.cpp,
// DESIGN.md §3.13): which set of up to max_t shards explains a stripe whose stored recovery shards
// disagree with its originals.
//
// Inputs per slice of stripes, as for locate (rs_locate_kernels.hip): enc = the encode of the
// originals ([n][m][sb]), rec = the stored recovery shards, bad = k_verify_compare's flags [n][m].
// The syndrome vector of symbol p is S(p) = (enc[r] ^ rec[r])(p), r < m. With corrupt shards T it is
// sum_{i in T} G_i * err_i(p), G = [C | I_m]: column j < k holds the encode's coefficients
// c[r][j], column k + r is the unit vector e_r. All symbols of a stripe share T, so the S(p) span a
// subspace V of dimension rho <= |T|, and the columns of G that lie in V are the corrupt shards.
//
// Per stripe: a basis B_0 .. B_{i-1} of the span found so far in reduced echelon form
// (B_j[piv_l] = delta_jl), as 16-bit symbols basis[max_t][m], pivot rows piv[max_t], and the
// multiply tables tabs[max_t][m] of its entries (an all-zero table for a zero entry); state
// (kMlocActive, the final rank rho >= 0, or kLocUnlocated) and pos, the smallest symbol index that
// the last check found outside the span (kMlocNoPos: none).
//  * k_mloc_check<MODE, NT>, round i = NT: flattened over (stripe, group of 16 rows, 16 KiB
//    segment), grid-stride. Symbol p lies in the span iff S_r(p) == sum_j B_j[r] * S_{piv_j}(p) for
//    every r: dev::span_check (rs_device_span.hpp, the pass k_locate_confirm runs with one pivot)
//    with the NT pivot rows piv[0, NT), rows from 0 and the position wanted. A lane that sees a
//    difference contributes its symbol index; one atomicMin per wave. Round 0 (an empty basis)
//    looks for a nonzero syndrome and reads only rows whose compare flag is set, so a clean stripe
//    costs its flags.
//  * k_mloc_extend, one workgroup per stripe: no failing symbol settles the stripe with rho = i;
//    one at i == max_t makes it unlocated; otherwise S(pos) is reduced by the basis, normalised at
//    its first nonzero row (the new pivot), the earlier vectors are reduced by it and all tables
//    are rebuilt.
//  * k_mloc_match: which of the k + m columns of G lie in the span, one column per lane.
//  * k_mloc_finish: d_count, the d_located and d_present rows, d_counts.
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
using dev::kNoSym;
using dev::kRows;
using dev::kSeg;
using dev::kSegSyms;

// a * b for symbols a, b (log[0] is no logarithm: zero is tested)
__device__ __forceinline__ uint32_t gf_mul_log(uint32_t a, uint32_t log_b, const uint16_t *__restrict__ d_exp,
                                               const uint16_t *__restrict__ d_log) {
  if (a == 0) return 0;
  const uint32_t sum = static_cast<uint32_t>(d_log[a]) + log_b;
  return d_exp[(sum + (sum >> 16)) & 0xFFFFu];  // rs_gf.hpp add_mod
}
__device__ __forceinline__ uint32_t gf_mul(uint32_t a, uint32_t b, const uint16_t *__restrict__ d_exp,
                                           const uint16_t *__restrict__ d_log) {
  return b == 0 ? 0 : gf_mul_log(a, d_log[b], d_exp, d_log);
}

// ========================================================================= check
template <int MODE, int NT>
__global__ __launch_bounds__(256) void k_mloc_check(const uint8_t *__restrict__ enc, uint64_t enc_stride,
                                                    const uint8_t *__restrict__ rec, uint64_t rec_stride, uint64_t sb,
                                                    uint64_t n, uint32_t m, uint32_t max_t, uint64_t segs,
                                                    uint32_t groups, const int32_t *__restrict__ state,
                                                    const uint8_t *__restrict__ bad,
                                                    const uint32_t *__restrict__ piv, const RsTab *__restrict__ tabs,
                                                    unsigned long long *pos) {
  const uint64_t per_stripe = segs * groups, total = n * per_stripe;
  const uint32_t tid = threadIdx.x;
  for (uint64_t w = blockIdx.x; w < total; w += gridDim.x) {
    const uint64_t s = w / per_stripe, rem = w % per_stripe;
    if (state[s] != kMlocActive) continue;  // settled: nothing to read
    const uint32_t g = static_cast<uint32_t>(rem / segs);
    const uint64_t seg = rem % segs;
    // an earlier segment already has a failing symbol (a stale value only costs time)
    if (*static_cast<volatile unsigned long long *>(pos + s) < seg * kSegSyms) continue;
    const uint32_t r_lo = g * kRows, r_hi = min(m, r_lo + kRows);
    const uint8_t *flag = bad + s * m;
    if (NT == 0) {  // rows that agree hold no nonzero syndrome
      uint32_t any = 0;
      for (uint32_t r = r_lo; r < r_hi; r++) any |= flag[r];
      if (!any) continue;
    }
    const RsTab *tb = tabs + s * max_t * m;
    uint32_t pr[NT > 0 ? NT : 1];
#pragma unroll
    for (int j = 0; j < NT; j++) pr[j] = piv[s * max_t + j];
    // the lane's smallest failing symbol, counted from the segment's first
    const uint32_t at = dev::span_check<MODE, NT, true>(enc + s * enc_stride, rec + s * rec_stride, sb, seg, segs, r_lo,
                                                        r_hi, pr, flag, [&](int j, uint32_t r) { return tb + j * m + r; });
    if (__builtin_amdgcn_ballot_w64(at != kNoSym) != 0ull) {  // wave-uniform: one atomic per wave
      uint32_t lowest = at;
      for (int o = 32; o > 0; o >>= 1) lowest = min(lowest, static_cast<uint32_t>(__shfl_xor(static_cast<int>(lowest), o)));
      if ((tid & 63u) == 0u) atomicMin(pos + s, static_cast<unsigned long long>(seg * kSegSyms + lowest));
    }
  }
}

// ======================================================================== extend
__device__ __forceinline__ void zero_tab(RsTab *out) {
#pragma unroll
  for (int i = 0; i < 10; i++) out->lo[i] = out->hi[i] = 0;
  out->flags = 0;
  out->log_m = kModulus;
  out->pad[0] = out->pad[1] = 0;
}

__global__ __launch_bounds__(256) void k_mloc_extend(const uint8_t *__restrict__ enc, uint64_t enc_stride,
                                                     const uint8_t *__restrict__ rec, uint64_t rec_stride, uint64_t sb,
                                                     uint64_t n, uint32_t m, uint32_t round, uint32_t max_t,
                                                     const uint16_t *__restrict__ d_exp,
                                                     const uint16_t *__restrict__ d_log, int32_t *state,
                                                     unsigned long long *pos, uint32_t *piv, uint16_t *basis,
                                                     RsTab *tabs) {
  __shared__ uint32_t sh_coef[kMlocMaxT], sh_piv, sh_lead;
  __shared__ int32_t sh_state;
  __shared__ unsigned long long sh_pos;
  const uint32_t tid = threadIdx.x;
  for (uint64_t s = blockIdx.x; s < n; s += gridDim.x) {
    __syncthreads();  // the previous stripe's shared words are no longer read
    if (tid == 0) {
      sh_state = state[s];
      sh_pos = pos[s];
      sh_piv = 0xFFFFFFFFu;
    }
    __syncthreads();
    if (sh_state != kMlocActive) continue;  // workgroup-uniform
    const unsigned long long p = sh_pos;
    if (p == kMlocNoPos || round == max_t) {
      // every symbol lies in the span: rank `round`; or the rank is above max_t
      if (tid == 0) state[s] = p == kMlocNoPos ? static_cast<int32_t>(round) : kLocUnlocated;
      continue;
    }
    uint64_t lo, hi;  // the byte offsets of symbol p
    dev::symbol_bytes(sb, p, lo, hi);
    const uint8_t *pa = enc + s * enc_stride, *pb = rec + s * rec_stride;
    auto syndrome = [&](uint32_t r) {
      return static_cast<uint32_t>(pa[r * sb + lo] ^ pb[r * sb + lo]) |
             static_cast<uint32_t>(pa[r * sb + hi] ^ pb[r * sb + hi]) << 8;
    };
    uint16_t *B = basis + s * max_t * m;
    uint32_t *pv = piv + s * max_t;
    if (tid < round) sh_coef[tid] = syndrome(pv[tid]);
    __syncthreads();
    // v = S(p) reduced by the basis; its first nonzero row is the new pivot
    for (uint32_t r = tid; r < m; r += 256u) {
      uint32_t v = syndrome(r);
      for (uint32_t j = 0; j < round; j++) v ^= gf_mul(B[j * m + r], sh_coef[j], d_exp, d_log);
      B[round * m + r] = static_cast<uint16_t>(v);
      if (v) atomicMin(&sh_piv, r);
    }
    __syncthreads();
    const uint32_t rho = sh_piv;
    if (rho == 0xFFFFFFFFu) {  // not reached: the symbol failed the check, so v != 0
      if (tid == 0) state[s] = kLocUnlocated;
      continue;
    }
    if (tid < round) sh_coef[tid] = B[tid * m + rho];  // before the earlier vectors change
    if (tid == 0) sh_lead = B[round * m + rho];
    __syncthreads();
    const uint32_t inv_log = (kModulus - d_log[sh_lead]) % kModulus;
    for (uint32_t r = tid; r < m; r += 256u) {
      const uint32_t b = gf_mul_log(B[round * m + r], inv_log, d_exp, d_log);
      B[round * m + r] = static_cast<uint16_t>(b);
      for (uint32_t j = 0; j < round; j++) B[j * m + r] ^= static_cast<uint16_t>(gf_mul(b, sh_coef[j], d_exp, d_log));
    }
    __syncthreads();
    // a zero entry is an all-zero table: it has no logarithm to build from
    RsTab *tb = tabs + s * max_t * m;
    for (uint32_t i = tid; i < (round + 1) * m; i += 256u) {
      const uint32_t e = B[i];
      if (e == 0) zero_tab(tb + i);
      else build_tab(tb + i, d_log[e], d_exp, d_log);
    }
    if (tid == 0) {
      pv[round] = rho;
      pos[s] = kMlocNoPos;
    }
  }
}

// ========================================================================= match
// found[s][0, nfound[s]): the columns of G in the span of stripe s, ascending. At most rho of them:
// any m columns of G are independent and rho < m.
__global__ __launch_bounds__(256) void k_mloc_match(uint64_t n, uint32_t k, uint32_t m, uint32_t max_t,
                                                    const uint16_t *__restrict__ cl,
                                                    const uint16_t *__restrict__ d_exp,
                                                    const uint16_t *__restrict__ d_log,
                                                    const int32_t *__restrict__ state,
                                                    const uint32_t *__restrict__ piv,
                                                    const uint16_t *__restrict__ basis, int32_t *__restrict__ found,
                                                    uint32_t *__restrict__ nfound) {
  __shared__ uint32_t sh_n, sh_piv[kMlocMaxT];
  __shared__ int32_t sh_list[kMlocMaxT];
  const uint32_t tid = threadIdx.x;
  for (uint64_t s = blockIdx.x; s < n; s += gridDim.x) {
    __syncthreads();  // the previous stripe's shared words are no longer read
    const int32_t st = state[s];
    if (st <= 0) {  // clean or unlocated: no column to name
      if (tid == 0) nfound[s] = 0;
      continue;
    }
    const uint32_t rho = static_cast<uint32_t>(st);
    if (tid == 0) sh_n = 0;
    if (tid < rho) sh_piv[tid] = piv[s * max_t + tid];
    __syncthreads();
    const uint16_t *B = basis + s * max_t * m;
    for (uint32_t c = tid; c < k + m; c += 256u) {
      bool in;
      if (c < k) {  // G_c[r] == sum_l B_l[r] * G_c[piv_l] for every r
        const uint16_t *col = cl + static_cast<uint64_t>(c) * m;
        in = true;
        for (uint32_t r = 0; r < m && in; r++) {
          uint32_t sum = 0;
          for (uint32_t l = 0; l < rho; l++) sum ^= gf_mul_log(B[l * m + r], col[sh_piv[l]], d_exp, d_log);
          in = sum == d_exp[col[r]];
        }
      } else {  // e_r lies in the span iff a basis vector is e_r: its pivot is r and it is zero elsewhere
        const uint32_t r = c - k;
        in = false;
        for (uint32_t l = 0; l < rho; l++)
          if (sh_piv[l] == r) {
            in = true;
            for (uint32_t q = 0; q < m; q++)
              if (q != r && B[l * m + q]) in = false;
          }
      }
      if (in) {
        const uint32_t slot = atomicAdd(&sh_n, 1u);
        if (slot < kMlocMaxT) sh_list[slot] = static_cast<int32_t>(c);
      }
    }
    __syncthreads();
    if (tid == 0) {
      const uint32_t cnt = min(sh_n, rho);
      for (uint32_t i = 1; i < cnt; i++)  // ascending: at most 8 entries
        for (uint32_t j = i; j > 0 && sh_list[j - 1] > sh_list[j]; j--) {
          const int32_t x = sh_list[j];
          sh_list[j] = sh_list[j - 1];
          sh_list[j - 1] = x;
        }
      for (uint32_t i = 0; i < cnt; i++) found[s * max_t + i] = sh_list[i];
      nfound[s] = sh_n;
    }
  }
}

// ======================================================================== finish
// One thread per (stripe, byte of its present row) — or per stripe without d_present. A stripe of
// rank rho is located iff exactly rho columns lie in its span. counts[max_t + 2] (zeroed by the
// host): the stripes with 0 .. max_t located shards, then the unlocated ones.
__global__ __launch_bounds__(256) void k_mloc_finish(const int32_t *__restrict__ state,
                                                     const int32_t *__restrict__ found,
                                                     const uint32_t *__restrict__ nfound, uint32_t k, uint32_t m,
                                                     uint32_t max_t, uint64_t n, int32_t *__restrict__ count,
                                                     int32_t *__restrict__ located, uint64_t located_stride,
                                                     uint8_t *__restrict__ present, uint64_t present_stride,
                                                     unsigned long long *counts) {
  __shared__ uint32_t part[kMlocMaxT + 2];
  if (threadIdx.x < kMlocMaxT + 2) part[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t row = present ? static_cast<uint64_t>(k) + m : 1, total = n * row;
  for (uint64_t g = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; g < total;
       g += static_cast<uint64_t>(gridDim.x) * 256u) {
    const uint64_t s = g / row, i = g % row;
    const int32_t rho = state[s];
    const int32_t cnt = rho == 0 ? 0 : rho > 0 && nfound[s] == static_cast<uint32_t>(rho) ? rho : kLocUnlocated;
    const int32_t *list = found + s * max_t;
    if (i == 0) {
      count[s] = cnt;
      if (located)
        for (uint32_t q = 0; q < max_t; q++)
          located[s * located_stride + q] = static_cast<int32_t>(q) < cnt ? list[q] : -1;
      if (counts) atomicAdd(&part[cnt >= 0 ? static_cast<uint32_t>(cnt) : max_t + 1], 1u);
    }
    if (present) {
      uint8_t v = 1;
      for (int32_t q = 0; q < cnt; q++)
        if (static_cast<uint64_t>(list[q]) == i) v = 0;
      present[s * present_stride + i] = v;
    }
  }
  __syncthreads();
  if (counts && threadIdx.x < max_t + 2 && part[threadIdx.x])
    atomicAdd(counts + threadIdx.x, static_cast<unsigned long long>(part[threadIdx.x]));
}

}  // namespace

hipError_t launch_mloc_check(const uint8_t *enc, uint64_t enc_stride, const uint8_t *rec, uint64_t rec_stride,
                             uint64_t sb, uint64_t n, uint32_t m, uint32_t round, uint32_t max_t, const int32_t *state,
                             const uint8_t *bad, const uint32_t *piv, const RsTab *tabs, uint64_t *pos,
                             hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (round > max_t || max_t > kMlocMaxT) return hipErrorInvalidValue;
  const uint64_t segs = (sb + kSeg - 1) / kSeg;
  const uint32_t groups = (m + kRows - 1) / kRows;
  const dim3 grid(static_cast<uint32_t>(std::min<uint64_t>(n * segs * groups, 1u << 20)));
  unsigned long long *p = reinterpret_cast<unsigned long long *>(pos);
  static const char *const kNames[3] = {"k_mloc_check_x1", "k_mloc_check_x4", "k_mloc_check_x16"};
  with_int(load_mode(enc, enc_stride, rec, rec_stride, sb), kModes, [&](auto mode) {
    trace_launch(kNames[decltype(mode)::value]);
    with_int(static_cast<int>(round), std::make_integer_sequence<int, kMlocMaxT + 1>(), [&](auto nt) {
      hipLaunchKernelGGL((k_mloc_check<decltype(mode)::value, decltype(nt)::value>), grid, dim3(256), 0, s, enc,
                         enc_stride, rec, rec_stride, sb, n, m, max_t, segs, groups, state, bad, piv, tabs, p);
    });
  });
  return hipGetLastError();
}

hipError_t launch_mloc_extend(const uint8_t *enc, uint64_t enc_stride, const uint8_t *rec, uint64_t rec_stride,
                              uint64_t sb, uint64_t n, uint32_t m, uint32_t round, uint32_t max_t,
                              const uint16_t *d_exp, const uint16_t *d_log, int32_t *state, uint64_t *pos,
                              uint32_t *piv, uint16_t *basis, RsTab *tabs, hipStream_t s) {
  if (n == 0) return hipSuccess;
  trace_launch("k_mloc_extend");
  const dim3 grid(static_cast<uint32_t>(std::min<uint64_t>(n, 1u << 20)));
  hipLaunchKernelGGL(k_mloc_extend, grid, dim3(256), 0, s, enc, enc_stride, rec, rec_stride, sb, n, m, round, max_t,
                     d_exp, d_log, state, reinterpret_cast<unsigned long long *>(pos), piv, basis, tabs);
  return hipGetLastError();
}

hipError_t launch_mloc_match(uint64_t n, uint32_t k, uint32_t m, uint32_t max_t, const uint16_t *cl,
                             const uint16_t *d_exp, const uint16_t *d_log, const int32_t *state, const uint32_t *piv,
                             const uint16_t *basis, int32_t *found, uint32_t *nfound, hipStream_t s) {
  if (n == 0) return hipSuccess;
  trace_launch("k_mloc_match");
  const dim3 grid(static_cast<uint32_t>(std::min<uint64_t>(n, 1u << 20)));
  hipLaunchKernelGGL(k_mloc_match, grid, dim3(256), 0, s, n, k, m, max_t, cl, d_exp, d_log, state, piv, basis, found,
                     nfound);
  return hipGetLastError();
}

hipError_t launch_mloc_finish(const int32_t *state, const int32_t *found, const uint32_t *nfound, uint32_t k,
                              uint32_t m, uint32_t max_t, uint64_t n, int32_t *count, int32_t *located,
                              uint64_t located_stride, uint8_t *present, uint64_t present_stride, uint64_t *counts,
                              hipStream_t s) {
  if (n == 0) return hipSuccess;
  trace_launch("k_mloc_finish");
  const uint64_t total = n * (present ? static_cast<uint64_t>(k) + m : 1);
  const uint64_t blocks = std::min<uint64_t>((total + 255) / 256, 1u << 16);
  hipLaunchKernelGGL(k_mloc_finish, dim3(static_cast<uint32_t>(blocks)), dim3(256), 0, s, state, found, nfound, k, m,
                     max_t, n, count, located, located_stride, present, present_stride,
                     reinterpret_cast<unsigned long long *>(counts));
  return hipGetLastError();
}

}  // namespace rs
