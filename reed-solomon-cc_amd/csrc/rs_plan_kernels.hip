// rs_plan_kernels.hip — the per-stripe plan kernels for gfx950 (MI355X): what a batch with its
// own erasure pattern per stripe needs before the codec kernels run, computed on the device
// from the present rows. Scalar GF(2^16) code (log / exp tables, one symbol per thread): the
// erasure locator (k_erasure_logs), the multiplier tables and maps of each path
// (k_pattern_tables, k_pattern_images / k_pattern_mtabs, k_psyn_plan, k_psyn_rebuild_plan, k_wps_plan,
// k_wps_plan_wave, k_fdec_block) and the present rows trimmed to k shards (k_trim_present).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rs_internal.hpp"

namespace rs {
namespace {

// ================================== per-stripe erasure patterns: plans on device
// (§8f rank 2) One workgroup per stripe evaluates the erasure locator exactly as
// Generic.zig:200-215 does — FWHT truncated to chunk+k, pointwise product with
// log_walsh mod 65535, full 65536-point FWHT (walsh_hadamard.zig:16-62) — on a
// 128 KiB u16 array in LDS, then the stripe's W multiplier tables are built.
__device__ __forceinline__ uint32_t add_mod_d(uint32_t x, uint32_t y) {
  const uint32_t s = x + y;
  return (s + (s >> 16)) & 0xFFFF;
}
__device__ __forceinline__ uint32_t sub_mod_d(uint32_t x, uint32_t y) {
  const uint32_t d = x + 65535u - y;
  return (d + (d >> 16)) & 0xFFFF;
}

// walsh_hadamard.zig:16-31 over LDS, groups r < m; all threads call
__device__ void fwht_lds(uint16_t *e, uint32_t m) {
  uint32_t dist = 1;
  for (uint32_t stride = 4; stride <= 65536; dist = stride, stride *= 4) {
    const uint32_t groups = (m + stride - 1) / stride;
    const uint32_t total = groups * dist;
    for (uint32_t t = threadIdx.x; t < total; t += blockDim.x) {
      const uint32_t x0 = t / dist * stride + t % dist;
      const uint32_t x1 = x0 + dist, x2 = x1 + dist, x3 = x2 + dist;
      const uint32_t a0 = e[x0], a1 = e[x1], a2 = e[x2], a3 = e[x3];
      const uint32_t s0 = add_mod_d(a0, a1), d0 = sub_mod_d(a0, a1);
      const uint32_t s1 = add_mod_d(a2, a3), d1 = sub_mod_d(a2, a3);
      e[x0] = static_cast<uint16_t>(add_mod_d(s0, s1));
      e[x1] = static_cast<uint16_t>(add_mod_d(d0, d1));
      e[x2] = static_cast<uint16_t>(sub_mod_d(s0, s1));
      e[x3] = static_cast<uint16_t>(sub_mod_d(d0, d1));
    }
    __syncthreads();
  }
}

// per stripe: present[k+m] -> logs[W] (root.zig:277-289 + Generic.zig:200-215). low: the
// low-rate layout of rs_gf.cpp erasure_logs_low (C = ceilPow2(k): originals [0, k), known
// zeros [k, C), recovery [C, C + m), unknown [C + m, W), transform over W). A small erased set
// (W x |set| <= 2^20) is summed point by point, logs[p] = sum over erased j of log[p ^ j] mod
// 65535 (the dyadic convolution the two transforms evaluate, rs_gf.cpp erasure_logs_of: equal
// mod 65535); larger sets take the transforms in LDS.
__device__ __forceinline__ uint32_t erased_flag(const uint8_t *pr, uint32_t i, uint32_t k, uint32_t m, uint32_t C,
                                                uint32_t W, uint32_t end, uint32_t low) {
  if (low) {
    if (i < k) return pr[i] ? 0u : 1u;
    if (i >= C && i < end) return pr[k + i - C] ? 0u : 1u;
    return i >= end && i < W ? 1u : 0u;
  }
  if (i < m) return pr[k + i] ? 0u : 1u;
  if (i < C) return 1u;
  return i < end ? (pr[i - C] ? 0u : 1u) : 0u;
}

__global__ __launch_bounds__(1024) void k_erasure_logs(const uint8_t *__restrict__ present, uint64_t present_stride,
                                                       uint32_t k, uint32_t m, uint32_t C, uint32_t W, uint32_t low,
                                                       const uint16_t *__restrict__ log_walsh,
                                                       const uint16_t *__restrict__ log_t,
                                                       uint16_t *__restrict__ logs) {
  __shared__ uint16_t e[65536];
  __shared__ uint32_t n_er;
  const uint8_t *pr = present + static_cast<uint64_t>(blockIdx.x) * present_stride;
  const uint32_t end = low ? C + m : C + k, trunc = low ? W : end;
  uint16_t *out = logs + static_cast<uint64_t>(blockIdx.x) * W;
  if (threadIdx.x == 0) n_er = 0;
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < trunc; i += blockDim.x)
    if (erased_flag(pr, i, k, m, C, W, end, low)) e[atomicAdd(&n_er, 1u)] = static_cast<uint16_t>(i);
  __syncthreads();
  const uint32_t n = n_er;
  if (static_cast<uint64_t>(W) * n <= (1u << 20)) {  // integer sums: the list's order does not matter
    for (uint32_t p = threadIdx.x; p < W; p += blockDim.x) {
      uint32_t sum = 0;  // n <= 2^20 / W <= 1024 terms: no overflow
      for (uint32_t j = 0; j < n; j++) sum += log_t[p ^ e[j]];
      out[p] = static_cast<uint16_t>(sum % 65535u);
    }
    return;
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < 65536; i += blockDim.x)
    e[i] = static_cast<uint16_t>(i < trunc ? erased_flag(pr, i, k, m, C, W, end, low) : 0u);
  __syncthreads();
  fwht_lds(e, trunc);
  for (uint32_t i = threadIdx.x; i < 65536; i += blockDim.x) {
    const uint32_t prod = static_cast<uint32_t>(e[i]) * log_walsh[i];
    e[i] = static_cast<uint16_t>(add_mod_d(prod & 0xFFFF, prod >> 16));
  }
  __syncthreads();
  fwht_lds(e, 65536);
  for (uint32_t p = threadIdx.x; p < W; p += blockDim.x) out[p] = e[p];
}

__device__ __forceinline__ uint32_t mul16_d(uint32_t x, uint32_t lm, const uint16_t *exp, const uint16_t *log) {
  return x == 0 ? 0 : exp[add_mod_d(log[x], lm)];
}
__device__ uint32_t mul_engine_d(uint32_t x, uint32_t lm, bool d1, const uint16_t *exp, const uint16_t *log) {
  if (!d1) return mul16_d(x, lm, exp, log);
  const uint32_t xh = ((x & 0xF) << 4) ^ (x & 0xFFF0);
  return (mul16_d(x, lm, exp, log) & 0xFF) | (mul16_d(xh, lm, exp, log) & 0xFF00);
}
// rs_gf.cpp make_tab on device
__device__ void make_tab_d(RsTab &t, uint32_t lm, bool d1, const uint16_t *exp, const uint16_t *log) {
  constexpr int kOff[6] = {0, 3, 6, 8, 11, 14};
  constexpr int kBits[6] = {3, 3, 2, 3, 3, 2};
  constexpr int kSlot[6] = {0, 2, 4, 5, 7, 9};
#pragma unroll
  for (int i = 0; i < 10; i++) t.lo[i] = t.hi[i] = 0;
#pragma unroll
  for (int f = 0; f < 6; f++)
    for (uint32_t v = 0; v < (1u << kBits[f]); v++) {
      const uint32_t p = mul_engine_d(v << kOff[f], lm, d1, exp, log);
      const int w = kSlot[f] + (v >> 2), sh = 8 * (v & 3);
      t.lo[w] |= (p & 0xFF) << sh;
      t.hi[w] |= (p >> 8) << sh;
    }
  t.flags = 0;
  t.log_m = lm;
  t.pad[0] = t.pad[1] = 0;
}

// per (stripe, position): masks, sources, restored slots (root.zig:291-326)
__global__ __launch_bounds__(256) void k_pattern_tables(const uint8_t *__restrict__ present, uint64_t present_stride,
                                                        uint32_t k, uint32_t m, uint32_t C, uint32_t W, uint32_t n,
                                                        uint32_t max_e, bool d1, uint32_t low,
                                                        const uint16_t *__restrict__ logs,
                                                        const uint16_t *__restrict__ exp, const uint16_t *__restrict__ log,
                                                        RsTab *pre, RsTab *post, int32_t *src, int32_t *dst,
                                                        int32_t *status) {
  const uint64_t g = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (g >= static_cast<uint64_t>(n) * W) return;
  const uint64_t s = g / W;
  const uint32_t p = static_cast<uint32_t>(g % W);
  const uint8_t *pr = present + s * present_stride;
  if (p == 0 && status) {  // root.zig:271 NotEnoughShards; restored slots beyond max_e: InvalidArgument
    uint32_t have = 0, e = 0;
    for (uint32_t i = 0; i < k + m; i++) have += pr[i] ? 1 : 0;
    for (uint32_t i = 0; i < k; i++) e += pr[i] ? 0 : 1;
    status[s] = have < k ? 2 : (e > max_e ? 14 : 0);
  }
  const uint32_t lm = logs[g];
  int32_t sv = -1, dv = -1;
  RsTab tp{}, tq{};
  // positions: originals at o0 + i, recovery at r0 + r (low rate: o0 = 0, r0 = C)
  const uint32_t o0 = low ? 0 : C, r0 = low ? C : 0;
  if (p >= r0 && p < r0 + m && pr[k + p - r0]) {
    sv = kSrcRecovery | static_cast<int32_t>(p - r0);
    make_tab_d(tp, lm, d1, exp, log);
  } else if (p >= o0 && p < o0 + k && pr[p - o0]) {
    sv = static_cast<int32_t>(p - o0);
    make_tab_d(tp, lm, d1, exp, log);
  }
  if (p >= o0 && p < o0 + k && !pr[p - o0]) {
    int32_t slot = 0;
    for (uint32_t i = 0; i < p - o0; i++) slot += pr[i] ? 0 : 1;
    uint32_t have = 0;  // a NotEnoughShards stripe restores nothing: no slot of its row is written
    for (uint32_t i = 0; i < k + m; i++) have += pr[i] ? 1 : 0;
    dv = have >= k && slot < static_cast<int32_t>(max_e) ? slot : -1;
    make_tab_d(tq, 65535u - lm, d1, exp, log);
  }
  pre[g] = tp;
  post[g] = tq;
  src[g] = sv;
  dst[g] = dv;
}

// ---- per-stripe patterns as per-stripe e x k matrices (corrected multiply)
// One thread per (stripe, input t, basis bit b): the reconstruct of root.zig:268-335
// on one symbol per position (W <= 32 in registers), input t = basis symbol 1 << b,
// every other position zero; the restored originals are column (t, b) of the
// stripe's map. Inputs: the present originals, then the first e present recovery
// shards (k in all); outputs: the missing originals, ascending, up to max_e.
__device__ __forceinline__ void ifft_bf_s(uint32_t &x, uint32_t &y, const RsTab &t, const uint16_t *exp,
                                          const uint16_t *log) {
  y ^= x;
  if (!(t.flags & kTabXorOnly)) x ^= mul16_d(y, t.log_m, exp, log);
}
__device__ __forceinline__ void fft_bf_s(uint32_t &x, uint32_t &y, const RsTab &t, const uint16_t *exp,
                                         const uint16_t *log) {
  if (!(t.flags & kTabXorOnly)) x ^= mul16_d(y, t.log_m, exp, log);
  y ^= x;
}

template <int W>
__global__ __launch_bounds__(256) void k_pattern_images(const uint8_t *__restrict__ present, uint64_t present_stride,
                                                        uint32_t k, uint32_t m, uint32_t C, uint64_t n, uint32_t max_e,
                                                        const uint16_t *__restrict__ logs, const RsTab *__restrict__ ti,
                                                        const RsTab *__restrict__ tf, const uint16_t *__restrict__ exp,
                                                        const uint16_t *__restrict__ log, uint16_t *__restrict__ images,
                                                        int32_t *__restrict__ srcs, int32_t *__restrict__ nout) {
  const uint64_t g = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (g >= n * k * 16) return;
  const uint64_t s = g / (k * 16);
  const uint32_t t = static_cast<uint32_t>(g / 16 % k), b = static_cast<uint32_t>(g % 16);
  const uint8_t *pr = present + s * present_stride;
  const uint16_t *lg = logs + s * W;
  uint32_t have = 0, e = 0;
  for (uint32_t i = 0; i < k + m; i++) have += pr[i] ? 1 : 0;
  for (uint32_t i = 0; i < k; i++) e += pr[i] ? 0 : 1;
  int32_t in_pos = -1, src = 0;
  uint32_t cnt = 0;
  for (uint32_t i = 0; i < k && in_pos < 0; i++)
    if (pr[i]) {
      if (cnt == t) in_pos = static_cast<int32_t>(C + i), src = static_cast<int32_t>(i);
      cnt++;
    }
  for (uint32_t r = 0; r < m && in_pos < 0; r++)
    if (pr[k + r]) {
      if (cnt == t) in_pos = static_cast<int32_t>(r), src = kSrcRecovery | static_cast<int32_t>(r);
      cnt++;
    }
  if (b == 0) srcs[s * k + t] = src;  // a valid shard even for NotEnoughShards stripes (nothing is stored)
  if (t == 0 && b == 0) nout[s] = have >= k ? static_cast<int32_t>(min(e, max_e)) : 0;
  const uint32_t trunc = C + k;
  uint32_t v[W];
  const uint32_t x0 = in_pos >= 0 ? mul16_d(1u << b, lg[in_pos], exp, log) : 0u;  // erasure mask, root.zig:291-302
#pragma unroll
  for (int p = 0; p < W; p++) v[p] = p == in_pos ? x0 : 0u;
  {  // IFFT, Generic.zig:80-147 (schedule of push_ifft_tabs)
    int q = 0, d = 1;
#pragma unroll
    for (int d4 = 4; d4 <= W; d4 <<= 2) {
#pragma unroll
      for (int r = 0; r < W; r += d4) {
        if (static_cast<uint32_t>(r) < trunc) {
          const RsTab m01 = ti[q], m02 = ti[q + 1], m23 = ti[q + 2];
#pragma unroll
          for (int i = r; i < r + d; i++) {
            ifft_bf_s(v[i], v[i + d], m01, exp, log);
            ifft_bf_s(v[i + 2 * d], v[i + 3 * d], m23, exp, log);
            ifft_bf_s(v[i], v[i + 2 * d], m02, exp, log);
            ifft_bf_s(v[i + d], v[i + 3 * d], m02, exp, log);
          }
        }
        q += 3;
      }
      d = d4;
    }
    if (d < W) {
#pragma unroll
      for (int i = 0; i < d; i++) ifft_bf_s(v[i], v[d + i], ti[q], exp, log);
    }
  }
#pragma unroll
  for (int i = 1; i < W; i++) {  // formal derivative, root.zig:309-315
    const int w = i & -i;
#pragma unroll
    for (int j = 0; j < w; j++)
      if (i + j < W) v[i - w + j] ^= v[i + j];
  }
  {  // FFT, Generic.zig:15-78 (schedule of push_fft_tabs)
    int q = 0, d4 = W;
#pragma unroll
    for (int d = W >> 2; d != 0; d >>= 2) {
#pragma unroll
      for (int r = 0; r < W; r += d4) {
        if (static_cast<uint32_t>(r) < trunc) {
          const RsTab m01 = tf[q], m02 = tf[q + 1], m23 = tf[q + 2];
#pragma unroll
          for (int i = r; i < r + d; i++) {
            fft_bf_s(v[i], v[i + 2 * d], m02, exp, log);
            fft_bf_s(v[i + d], v[i + 3 * d], m02, exp, log);
            fft_bf_s(v[i], v[i + d], m01, exp, log);
            fft_bf_s(v[i + 2 * d], v[i + 3 * d], m23, exp, log);
          }
        }
        q += 3;
      }
      d4 = d;
    }
    if (d4 == 2) {
#pragma unroll
      for (int r = 0; r < W; r += 2)
        if (static_cast<uint32_t>(r) < trunc) fft_bf_s(v[r], v[r + 1], tf[q + r / 2], exp, log);
    }
  }
  uint16_t *img = images + (s * k + t) * max_e * 16 + b;
  uint32_t j = 0;
#pragma unroll
  for (int p = 0; p < W; p++) {  // reveal the missing originals, root.zig:320-326
    if (static_cast<uint32_t>(p) >= C && static_cast<uint32_t>(p) < C + k && !pr[p - C]) {
      if (j < max_e) img[j * 16] = static_cast<uint16_t>(mul16_d(v[p], 65535u - lg[p], exp, log));
      j++;
    }
  }
  for (; j < max_e; j++) img[j * 16] = 0;
}

// Per-stripe plan of the syndrome-network path (rs_psyn.hpp), one thread per stripe:
// E = the erased originals, R = the first e present recovery rows, A = G[R][E] (e x e
// block of the code's encode coefficients, G[r][t] = parity r of data t = 1), and
// x_E = A^-1 s_R with s_r = p_r ^ Enc_r(data, erased read as 0). Block per stripe
// (u32, nw = ceil(k / 32)): [0, nw) erased mask, [nw] R mask, [nw + 1] outputs stored =
// min(e, max_e) (0: none), then [nw + 2 + r * max_out + j] = A^-1[j][i(r)] in polynomial
// coordinates (bit i: the coefficient of alpha^i; 0 for rows outside R), the form the
// kernel multiplies in.
// G: [m][k] coefficients followed by the 16 Cantor basis elements (polynomial form).
__device__ __forceinline__ uint32_t gf_mul_d(uint32_t a, uint32_t b, const uint16_t *exp, const uint16_t *log) {
  return (a == 0 || b == 0) ? 0u : exp[add_mod_d(log[a], log[b])];
}

__global__ __launch_bounds__(64) void k_psyn_plan(const uint8_t *__restrict__ present, uint64_t present_stride,
                                                  uint32_t k, uint32_t m, uint32_t max_out, uint32_t max_e, uint64_t n,
                                                  const uint16_t *__restrict__ G, const uint16_t *__restrict__ exp,
                                                  const uint16_t *__restrict__ log, uint32_t *__restrict__ plan,
                                                  uint32_t plan_dw, int32_t *__restrict__ status) {
  const uint64_t s = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const uint8_t *pr = present + s * present_stride;
  uint32_t *pl = plan + s * plan_dw;
  const uint32_t nw = (k + 31) / 32;  // erased-original mask words (rs_psyn.hpp plan_dwords)
  uint32_t have = 0, e = 0;
  for (uint32_t i = 0; i < k + m; i++) have += pr[i] ? 1 : 0;
  for (uint32_t i = 0; i < k; i++) e += pr[i] ? 0 : 1;
  if (status) status[s] = have < k ? 2 : (e > max_e ? 14 : 0);  // as k_pattern_tables
  for (uint32_t w = 0; w < nw + 2; w++) pl[w] = 0;
  if (have < k || e == 0) return;  // nothing restored (e <= present recovery <= m from here)
  uint32_t E[kPsynMaxM], R[kPsynMaxM], rm = 0;
  for (uint32_t i = 0, c = 0; i < k && c < e; i++)
    if (!pr[i]) E[c++] = i;
  for (uint32_t r = 0, c = 0; r < m && c < e; r++)
    if (pr[k + r]) R[c++] = r, rm |= 1u << r;
  // Gauss-Jordan on [A | I] over GF(2^16)
  uint32_t A[kPsynMaxM][2 * kPsynMaxM];
  for (uint32_t i = 0; i < e; i++)
    for (uint32_t j = 0; j < 2 * e; j++) A[i][j] = j < e ? G[R[i] * k + E[j]] : (j - e == i ? 1u : 0u);
  for (uint32_t c = 0; c < e; c++) {
    uint32_t piv = c;
    while (piv < e && A[piv][c] == 0) piv++;
    if (piv == e) {  // singular: not an MDS code (the host keeps such codes off this path)
      if (status) status[s] = 15;  // RS_ERR_DEVICE: nothing restored
      return;
    }
    for (uint32_t j = 0; j < 2 * e; j++) {
      const uint32_t t = A[c][j];
      A[c][j] = A[piv][j];
      A[piv][j] = t;
    }
    const uint32_t inv = exp[(65535u - log[A[c][c]]) % 65535u];
    for (uint32_t j = 0; j < 2 * e; j++) A[c][j] = gf_mul_d(A[c][j], inv, exp, log);
    for (uint32_t i = 0; i < e; i++)
      if (i != c && A[i][c]) {
        const uint32_t f = A[i][c];
        for (uint32_t j = 0; j < 2 * e; j++) A[i][j] ^= gf_mul_d(f, A[c][j], exp, log);
      }
  }
  const uint16_t *cantor = G + m * k;
  for (uint32_t r = 0; r < m; r++) {
    int32_t ir = -1;
    for (uint32_t i = 0; i < e; i++) ir = R[i] == r ? static_cast<int32_t>(i) : ir;
    for (uint32_t j = 0; j < max_out; j++) {
      const uint32_t c = (ir >= 0 && j < e) ? A[j][e + ir] : 0u;  // x_j += A^-1[j][i] s_{R_i}
      uint32_t poly = 0;
      for (int b = 0; b < 16; b++) poly ^= (c >> b & 1u) ? cantor[b] : 0u;
      pl[nw + 2 + r * max_out + j] = poly;
    }
  }
  for (uint32_t i = 0; i < e; i++) pl[E[i] / 32] |= 1u << (E[i] % 32);
  pl[nw] = rm;
  pl[nw + 1] = e < max_e ? e : max_e;
}

// The plan of the rebuild variant (psyn::Spec::rebuild): the lost recovery
// shards Q are outputs as well. Absent recovery rows are read as zero, so for q in Q the network
// leaves s_q = Enc_q(data, erased read as 0), and p_q = s_q ^ sum_t G[q][E_t] x_t
// = s_q ^ sum_{r in R} (G[q][E] A^-1)[i(r)] s_r. Block per stripe (u32): [0, nw) erased mask,
// [nw] R (the rows whose p_r is loaded), [nw + 1] outputs stored = min(e_s, max_e), [nw + 2] the
// rows used in the solve, R | Q, then [nw + 3 + r * m + j] the coefficient of s_r in output j:
// j < e_o row j of A^-1 as above; j = e_o + q the products at R, the field's one at row Q_q.
__global__ __launch_bounds__(64) void k_psyn_rebuild_plan(const uint8_t *__restrict__ present, uint64_t present_stride,
                                                          uint32_t k, uint32_t m, uint32_t max_e, uint64_t n,
                                                          const uint16_t *__restrict__ G,
                                                          const uint16_t *__restrict__ exp,
                                                          const uint16_t *__restrict__ log, uint32_t *__restrict__ plan,
                                                          uint32_t plan_dw, int32_t *__restrict__ status) {
  const uint64_t s = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const uint8_t *pr = present + s * present_stride;
  uint32_t *pl = plan + s * plan_dw;
  const uint32_t nw = (k + 31) / 32;
  uint32_t e = 0, er = 0;
  for (uint32_t i = 0; i < k; i++) e += pr[i] ? 0 : 1;
  for (uint32_t r = 0; r < m; r++) er += pr[k + r] ? 0 : 1;
  const uint32_t es = e + er;
  if (status) status[s] = es > m ? 2 : (es > max_e ? 14 : 0);
  for (uint32_t w = 0; w < nw + 3; w++) pl[w] = 0;
  if (es > m || es == 0) return;  // fewer than k present, or nothing missing (e <= present recovery from here)
  uint32_t E[kPsynMaxM], R[kPsynMaxM], Q[kPsynMaxM], rm = 0, qm = 0;
  for (uint32_t i = 0, c = 0; i < k && c < e; i++)
    if (!pr[i]) E[c++] = i;
  for (uint32_t r = 0, c = 0, q = 0; r < m; r++) {
    if (pr[k + r]) {
      if (c < e) R[c++] = r, rm |= 1u << r;
    } else {
      Q[q++] = r, qm |= 1u << r;
    }
  }
  // Gauss-Jordan on [A | I] over GF(2^16) (no step when no original is missing)
  uint32_t A[kPsynMaxM][2 * kPsynMaxM];
  for (uint32_t i = 0; i < e; i++)
    for (uint32_t j = 0; j < 2 * e; j++) A[i][j] = j < e ? G[R[i] * k + E[j]] : (j - e == i ? 1u : 0u);
  for (uint32_t c = 0; c < e; c++) {
    uint32_t piv = c;
    while (piv < e && A[piv][c] == 0) piv++;
    if (piv == e) {  // singular: not an MDS code (the host keeps such codes off this path)
      if (status) status[s] = 15;  // RS_ERR_DEVICE: nothing rebuilt
      return;
    }
    for (uint32_t j = 0; j < 2 * e; j++) {
      const uint32_t t = A[c][j];
      A[c][j] = A[piv][j];
      A[piv][j] = t;
    }
    const uint32_t inv = exp[(65535u - log[A[c][c]]) % 65535u];
    for (uint32_t j = 0; j < 2 * e; j++) A[c][j] = gf_mul_d(A[c][j], inv, exp, log);
    for (uint32_t i = 0; i < e; i++)
      if (i != c && A[i][c]) {
        const uint32_t f = A[i][c];
        for (uint32_t j = 0; j < 2 * e; j++) A[i][j] ^= gf_mul_d(f, A[c][j], exp, log);
      }
  }
  const uint16_t *cantor = G + m * k;
  for (uint32_t r = 0; r < m; r++) {
    int32_t ir = -1;
    for (uint32_t i = 0; i < e; i++) ir = R[i] == r ? static_cast<int32_t>(i) : ir;
    for (uint32_t j = 0; j < m; j++) {
      uint32_t c = 0;
      if (j < e) {
        c = ir >= 0 ? A[j][e + ir] : 0u;  // x_j += A^-1[j][i] s_{R_i}
      } else if (j < es) {
        const uint32_t q = Q[j - e];
        if (ir >= 0)
          for (uint32_t t = 0; t < e; t++) c ^= gf_mul_d(G[q * k + E[t]], A[t][e + ir], exp, log);
        else if (r == q)
          c = 1u;  // s_q itself
      }
      uint32_t poly = 0;
      for (int b = 0; b < 16; b++) poly ^= (c >> b & 1u) ? cantor[b] : 0u;
      pl[nw + 3 + r * m + j] = poly;
    }
  }
  for (uint32_t i = 0; i < e; i++) pl[E[i] / 32] |= 1u << (E[i] % 32);
  pl[nw] = rm;
  pl[nw + 1] = es < max_e ? es : max_e;
  pl[nw + 2] = rm | qm;
}

// Per-stripe plan of the wide-code path (rs_psyn.hpp solve kernel after the FFT
// syndrome kernel, chunk 32 / 64): as k_psyn_plan for any e <= m <= 64, one thread per
// stripe (the e x 2e Gauss-Jordan lives in private memory). Block per stripe (u32):
// [0, dmw) the FFT kernel's masks (fftnet::dyn_mask_words: erased data bits, then the
// R rows stored), then at hdr = dmw: [0] outputs stored = min(e, max_e), [1] e,
// [2, 2 + 64) R, [66 + i * cs + j] = A^-1[j][i] in polynomial form for j < cs
// (cs = wps_coef_stride(max_e): 8, or max_e rounded up to 8 for the wave kernel below).
constexpr uint32_t kWpsMaxM = 64, kWpsMaxOut = 8;
__global__ __launch_bounds__(64) void k_wps_plan(const uint8_t *__restrict__ present, uint64_t present_stride,
                                                 uint32_t k, uint32_t m, uint32_t max_e, uint64_t n,
                                                 const uint16_t *__restrict__ G, const uint16_t *__restrict__ exp,
                                                 const uint16_t *__restrict__ log, uint32_t *__restrict__ plan,
                                                 uint32_t plan_dw, uint32_t dmw, int32_t *__restrict__ status) {
  const uint64_t s = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const uint8_t *pr = present + s * present_stride;
  uint32_t *pl = plan + s * plan_dw, *hd = pl + dmw;
  uint32_t have = 0, e = 0;
  for (uint32_t i = 0; i < k + m; i++) have += pr[i] ? 1 : 0;
  for (uint32_t i = 0; i < k; i++) e += pr[i] ? 0 : 1;
  if (status) status[s] = have < k ? 2 : (e > max_e ? 14 : 0);  // as k_pattern_tables
  for (uint32_t i = 0; i < dmw; i++) pl[i] = 0;
  hd[0] = hd[1] = 0;
  if (have < k || e == 0) return;
  uint16_t E[kWpsMaxM], R[kWpsMaxM];
  for (uint32_t i = 0, c = 0; i < k && c < e; i++)
    if (!pr[i]) E[c++] = static_cast<uint16_t>(i);
  for (uint32_t r = 0, c = 0; r < m && c < e; r++)
    if (pr[k + r]) R[c++] = static_cast<uint16_t>(r);
  uint16_t A[kWpsMaxM][2 * kWpsMaxM];
  for (uint32_t i = 0; i < e; i++)
    for (uint32_t j = 0; j < 2 * e; j++)
      A[i][j] = static_cast<uint16_t>(j < e ? G[R[i] * k + E[j]] : (j - e == i ? 1u : 0u));
  for (uint32_t c = 0; c < e; c++) {
    uint32_t piv = c;
    while (piv < e && A[piv][c] == 0) piv++;
    if (piv == e) {  // singular: not an MDS code (the host keeps such codes off this path)
      if (status) status[s] = 15;  // RS_ERR_DEVICE: nothing restored
      hd[0] = 0;
      return;
    }
    for (uint32_t j = 0; j < 2 * e; j++) {
      const uint16_t t = A[c][j];
      A[c][j] = A[piv][j];
      A[piv][j] = t;
    }
    const uint32_t inv = exp[(65535u - log[A[c][c]]) % 65535u];
    for (uint32_t j = c; j < 2 * e; j++) A[c][j] = static_cast<uint16_t>(gf_mul_d(A[c][j], inv, exp, log));
    for (uint32_t i = 0; i < e; i++)
      if (i != c && A[i][c]) {
        const uint32_t f = A[i][c];
        for (uint32_t j = c; j < 2 * e; j++) A[i][j] ^= static_cast<uint16_t>(gf_mul_d(f, A[c][j], exp, log));
      }
  }
  const uint16_t *cantor = G + m * k;
  const uint32_t kw = dmw - 2;  // skip words, then 2 store words
  for (uint32_t i = 0; i < e; i++) {
    pl[E[i] / 32] |= 1u << (E[i] % 32);
    pl[kw + R[i] / 32] |= 1u << (R[i] % 32);
    hd[2 + i] = R[i];
    for (uint32_t j = 0; j < kWpsMaxOut; j++) {
      const uint32_t c = j < e ? A[j][e + i] : 0u;
      uint32_t poly = 0;
      for (int b = 0; b < 16; b++) poly ^= (c >> b & 1u) ? cantor[b] : 0u;
      hd[2 + kWpsMaxM + i * kWpsMaxOut + j] = poly;
    }
  }
  hd[1] = e;
  hd[0] = e < max_e ? e : max_e;
}

// The same plan for max_e > 8 (every output of up to 64 erased originals): one wave per
// stripe, the e x 2e Gauss-Jordan in LDS with the columns spread over the lanes (a
// thread per stripe would run e^3 / 3 table multiplies on its own: ~55,000 for e = 55).
// Coefficients at [66 + i * cs + j] for j < cs (cs = max_e rounded up to 8, <= 64).
__global__ __launch_bounds__(64) void k_wps_plan_wave(const uint8_t *__restrict__ present, uint64_t present_stride,
                                                      uint32_t k, uint32_t m, uint32_t max_e,
                                                      const uint16_t *__restrict__ G, const uint16_t *__restrict__ exp,
                                                      const uint16_t *__restrict__ log, uint32_t *__restrict__ plan,
                                                      uint32_t plan_dw, uint32_t dmw, uint32_t cs,
                                                      int32_t *__restrict__ status) {
  __shared__ uint16_t A[kWpsMaxM][2 * kWpsMaxM];
  __shared__ uint16_t E[kWpsMaxM], R[kWpsMaxM];
  const uint64_t s = blockIdx.x;
  const uint32_t t = threadIdx.x;
  const uint8_t *pr = present + s * present_stride;
  uint32_t *pl = plan + s * plan_dw, *hd = pl + dmw;
  uint32_t have = 0, e = 0;
  for (uint32_t i = t; i < k + m; i += 64) {
    have += pr[i] ? 1u : 0u;
    e += (i < k && !pr[i]) ? 1u : 0u;
  }
  for (int o = 32; o > 0; o >>= 1) {
    have += __shfl_xor(have, o);
    e += __shfl_xor(e, o);
  }
  if (t == 0 && status) status[s] = have < k ? 2 : (e > max_e ? 14 : 0);  // as k_pattern_tables
  for (uint32_t i = t; i < dmw; i += 64) pl[i] = 0;
  if (t == 0) hd[0] = hd[1] = 0;
  if (have < k || e == 0 || e > kWpsMaxM) return;  // wave-uniform
  if (t == 0) {
    for (uint32_t i = 0, c = 0; i < k && c < e; i++)
      if (!pr[i]) E[c++] = static_cast<uint16_t>(i);
    for (uint32_t r = 0, c = 0; r < m && c < e; r++)
      if (pr[k + r]) R[c++] = static_cast<uint16_t>(r);
  }
  __syncthreads();
  for (uint32_t i = 0; i < e; i++)
    for (uint32_t j = t; j < 2 * e; j += 64)
      A[i][j] = static_cast<uint16_t>(j < e ? G[R[i] * k + E[j]] : (j - e == i ? 1u : 0u));
  __syncthreads();
  for (uint32_t c = 0; c < e; c++) {
    const uint64_t nz = __ballot(t >= c && t < e && A[t][c] != 0);
    if (nz == 0) {  // singular: not an MDS code (the host keeps such codes off this path)
      if (t == 0 && status) status[s] = 15;  // RS_ERR_DEVICE: nothing restored
      if (t == 0) hd[0] = 0;
      return;
    }
    const uint32_t piv = static_cast<uint32_t>(__ffsll(static_cast<unsigned long long>(nz)) - 1);
    if (piv != c)
      for (uint32_t j = t; j < 2 * e; j += 64) {
        const uint16_t x = A[c][j];
        A[c][j] = A[piv][j];
        A[piv][j] = x;
      }
    __syncthreads();
    const uint32_t inv = exp[(65535u - log[A[c][c]]) % 65535u];
    __syncthreads();  // every lane has read the pivot before its column is scaled
    for (uint32_t j = t; j < 2 * e; j += 64) A[c][j] = static_cast<uint16_t>(gf_mul_d(A[c][j], inv, exp, log));
    __syncthreads();
    // elimination: lane t owns columns t and t + 64 and holds row t's factor; the logs of
    // the pivot row's entries are looked up once per pivot, so each update is one
    // independent exp lookup (no dependent table chain, no barrier per row)
    const uint32_t fr = t < e ? A[t][c] : 0u, lfr = fr ? log[fr] : 0u;
    const uint32_t p0 = t < 2 * e ? A[c][t] : 0u, p1 = t + 64 < 2 * e ? A[c][t + 64] : 0u;
    const uint32_t lp0 = p0 ? log[p0] : 0u, lp1 = p1 ? log[p1] : 0u;
    __syncthreads();  // column c read by every lane before its owner rewrites it
#pragma unroll 4
    for (uint32_t i = 0; i < e; i++) {
      const uint32_t f = __shfl(fr, static_cast<int>(i)), lf = __shfl(lfr, static_cast<int>(i));
      if (i == c || f == 0) continue;  // wave-uniform
      if (p0) A[i][t] ^= exp[add_mod_d(lf, lp0)];
      if (p1) A[i][t + 64] ^= exp[add_mod_d(lf, lp1)];
    }
    __syncthreads();
  }
  const uint16_t *cantor = G + m * k;
  const uint32_t kw = dmw - 2;  // skip words, then 2 store words
  if (t == 0)
    for (uint32_t i = 0; i < e; i++) {
      pl[E[i] / 32] |= 1u << (E[i] % 32);
      pl[kw + R[i] / 32] |= 1u << (R[i] % 32);
    }
  for (uint32_t i = t; i < e; i += 64) hd[2 + i] = R[i];
  for (uint32_t x = t; x < e * cs; x += 64) {
    const uint32_t i = x / cs, j = x % cs;
    const uint32_t c = j < e ? A[j][e + i] : 0u;
    uint32_t poly = 0;
    for (int b = 0; b < 16; b++) poly ^= (c >> b & 1u) ? cantor[b] : 0u;
    hd[2 + kWpsMaxM + i * cs + j] = poly;
  }
  if (t == 0) {
    hd[1] = e;
    hd[0] = e < max_e ? e : max_e;
  }
}

// The matrix path decodes from exactly k received shards (the present originals and
// the first e present recovery shards), so the erasure locator must be evaluated for
// that set: present rows with the other recovery shards marked absent.
__global__ __launch_bounds__(256) void k_trim_present(const uint8_t *__restrict__ present, uint64_t present_stride,
                                                      uint32_t k, uint32_t m, uint64_t n, uint8_t *__restrict__ out) {
  const uint64_t s = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const uint8_t *pr = present + s * present_stride;
  uint8_t *o = out + s * (k + m);
  uint32_t e = 0;
  for (uint32_t i = 0; i < k; i++) {
    o[i] = pr[i] ? 1 : 0;
    e += pr[i] ? 0 : 1;
  }
  uint32_t used = 0;
  for (uint32_t r = 0; r < m; r++) {
    const bool keep = pr[k + r] && used < e;
    used += keep ? 1 : 0;
    o[k + r] = keep ? 1 : 0;
  }
  // fewer than k present in total: keep the row as it is (the plan reports NotEnoughShards)
  if (used < e)
    for (uint32_t r = 0; r < m; r++) o[k + r] = pr[k + r] ? 1 : 0;
}

// rs_gf.cpp make_tab_from_images on device: one thread per (stripe, input, output)
__global__ __launch_bounds__(256) void k_pattern_mtabs(const uint16_t *__restrict__ images, uint64_t count,
                                                       RsTab *__restrict__ tabs) {
  const uint64_t g = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (g >= count) return;
  const uint16_t *img = images + g * 16;
  constexpr int kOff[6] = {0, 3, 6, 8, 11, 14};
  constexpr int kBits[6] = {3, 3, 2, 3, 3, 2};
  constexpr int kSlot[6] = {0, 2, 4, 5, 7, 9};
  RsTab t;
#pragma unroll
  for (int i = 0; i < 10; i++) t.lo[i] = t.hi[i] = 0;
#pragma unroll
  for (int f = 0; f < 6; f++)
    for (uint32_t v = 0; v < (1u << kBits[f]); v++) {
      uint32_t p = 0;
      for (int bit = 0; bit < kBits[f]; bit++)
        if (v >> bit & 1) p ^= img[kOff[f] + bit];
      const int w = kSlot[f] + (v >> 2), sh = 8 * (v & 3);
      t.lo[w] |= (p & 0xFF) << sh;
      t.hi[w] |= (p >> 8) << sh;
    }
  t.flags = 0;
  t.log_m = 0;
  t.pad[0] = t.pad[1] = 0;
  tabs[g] = t;
}

}  // namespace

hipError_t launch_pattern_matrix(const uint8_t *d_present, uint64_t present_stride, uint32_t k, uint32_t m, uint32_t C,
                                 uint32_t W, uint64_t n, uint32_t max_e, const uint16_t *logs, const RsTab *tab_ifft,
                                 const RsTab *tab_fft, const uint16_t *d_exp, const uint16_t *d_log, uint16_t *images,
                                 RsTab *tabs, int32_t *srcs, int32_t *nout, hipStream_t s) {
  const uint64_t threads = n * k * 16;
  const dim3 grid(static_cast<uint32_t>((threads + 255) / 256));
  trace_launch("k_pattern_images");
  trace_launch("k_pattern_mtabs");
  switch (W) {
#define RS_PIMG(W_)                                                                                                   \
  case W_:                                                                                                            \
    hipLaunchKernelGGL(k_pattern_images<W_>, grid, dim3(256), 0, s, d_present, present_stride, k, m, C, n, max_e, logs, \
                       tab_ifft, tab_fft, d_exp, d_log, images, srcs, nout);                                          \
    break;
    RS_PIMG(2) RS_PIMG(4) RS_PIMG(8) RS_PIMG(16) RS_PIMG(32)
#undef RS_PIMG
    default: return hipErrorInvalidValue;
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const uint64_t count = n * k * max_e;
  hipLaunchKernelGGL(k_pattern_mtabs, dim3(static_cast<uint32_t>((count + 255) / 256)), dim3(256), 0, s, images, count,
                     tabs);
  return hipGetLastError();
}

hipError_t launch_pattern_plan(const uint8_t *d_present, uint64_t present_stride, uint32_t k, uint32_t m, uint32_t C,
                               uint32_t W, uint64_t n, uint32_t max_e, bool d1, bool low, const uint16_t *d_exp,
                               const uint16_t *d_log, const uint16_t *d_log_walsh, uint16_t *logs, RsTab *pre,
                               RsTab *post, int32_t *src, int32_t *dst, int32_t *status, hipStream_t s) {
  trace_launch("k_erasure_logs");
  trace_launch("k_pattern_tables");
  for (uint64_t s0 = 0; s0 < n; s0 += 65535) {
    const uint32_t cnt = static_cast<uint32_t>(std::min<uint64_t>(65535, n - s0));
    hipLaunchKernelGGL(k_erasure_logs, dim3(cnt), dim3(1024), 0, s, d_present + s0 * present_stride,
                       present_stride, k, m, C, W, low ? 1u : 0u, d_log_walsh, d_log, logs + s0 * W);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  const uint64_t total = n * W;
  const uint64_t blocks = (total + 255) / 256;
  hipLaunchKernelGGL(k_pattern_tables, dim3(static_cast<uint32_t>(blocks)), dim3(256), 0, s, d_present,
                     present_stride, k, m, C, W, static_cast<uint32_t>(n), max_e, d1, low ? 1u : 0u, logs, d_exp, d_log,
                     pre, post, src, dst, status);
  return hipGetLastError();
}

hipError_t launch_psyn_plan(const uint8_t *present, uint64_t present_stride, uint32_t k, uint32_t m, uint32_t max_out,
                            uint32_t max_e, uint64_t n, const uint16_t *G, const uint16_t *d_exp, const uint16_t *d_log,
                            uint32_t *plan, uint32_t plan_dw, int32_t *status, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (k > 256 || m > kPsynMaxM || max_out > m || plan_dw < (k + 31) / 32 + 2 + m * max_out) return hipErrorInvalidValue;
  trace_launch("k_psyn_plan");
  hipLaunchKernelGGL(k_psyn_plan, dim3(static_cast<uint32_t>((n + 63) / 64)), dim3(64), 0, s, present, present_stride,
                     k, m, max_out, max_e, n, G, d_exp, d_log, plan, plan_dw, status);
  return hipGetLastError();
}

hipError_t launch_psyn_rebuild_plan(const uint8_t *present, uint64_t present_stride, uint32_t k, uint32_t m,
                                    uint32_t max_e, uint64_t n, const uint16_t *G, const uint16_t *d_exp,
                                    const uint16_t *d_log, uint32_t *plan, uint32_t plan_dw, int32_t *status,
                                    hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (k > 256 || m > kPsynMaxM || plan_dw < (k + 31) / 32 + 3 + m * m) return hipErrorInvalidValue;
  trace_launch("k_psyn_rebuild_plan");
  hipLaunchKernelGGL(k_psyn_rebuild_plan, dim3(static_cast<uint32_t>((n + 63) / 64)), dim3(64), 0, s, present,
                     present_stride, k, m, max_e, n, G, d_exp, d_log, plan, plan_dw, status);
  return hipGetLastError();
}

uint32_t wps_coef_stride(uint32_t max_e) {
  return max_e <= kWpsMaxOut ? kWpsMaxOut : std::min(kWpsMaxM, (max_e + 7u) / 8u * 8u);
}

hipError_t launch_wps_plan(const uint8_t *present, uint64_t present_stride, uint32_t k, uint32_t m, uint32_t max_e,
                           uint64_t n, const uint16_t *G, const uint16_t *d_exp, const uint16_t *d_log, uint32_t *plan,
                           uint32_t plan_dw, uint32_t dmw, int32_t *status, hipStream_t s) {
  if (n == 0) return hipSuccess;
  const uint32_t cs = wps_coef_stride(max_e);
  if (m > kWpsMaxM || dmw < 2 || plan_dw < dmw + 2 + kWpsMaxM + kWpsMaxM * cs || (dmw - 2) * 32 < k)
    return hipErrorInvalidValue;
  trace_launch(cs == kWpsMaxOut ? "k_wps_plan" : "k_wps_plan_wave");
  if (cs == kWpsMaxOut) {
    hipLaunchKernelGGL(k_wps_plan, dim3(static_cast<uint32_t>((n + 63) / 64)), dim3(64), 0, s, present,
                       present_stride, k, m, max_e, n, G, d_exp, d_log, plan, plan_dw, dmw, status);
  } else {
    if (n > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_wps_plan_wave, dim3(static_cast<uint32_t>(n)), dim3(64), 0, s, present, present_stride, k, m,
                       max_e, G, d_exp, d_log, plan, plan_dw, dmw, cs, status);
  }
  return hipGetLastError();
}

// Per-stripe decode blocks of the fused FFT reconstruct (rs_fftnet.hpp decode_block, on
// the device): one thread per (stripe, slot). Slot 0 writes the mask words, the block
// mask, the rows R (the trimmed present rows), the output rows and the status; slot
// 1 + p the masks of L_p (recovery row p in R); slot 1 + m + g those of
// L'_g * beta_K (erased data shard g); unused slots write zero masks.
__device__ uint32_t to_uv_d(uint32_t x, const FdecConsts &c) {
  uint32_t lo = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) lo ^= (x >> (8 + i) & 1) ? c.p[i] : 0u;
  return x ^ lo;
}
__global__ __launch_bounds__(256) void k_fdec_block(const uint8_t *__restrict__ trimmed, uint32_t k, uint32_t m,
                                                    uint32_t C, uint32_t W, uint64_t n, uint32_t max_e,
                                                    const uint16_t *__restrict__ logs, const uint16_t *__restrict__ exp,
                                                    const uint16_t *__restrict__ log, uint32_t dwm, uint32_t mko,
                                                    uint32_t words, uint32_t *__restrict__ blk, int32_t *status,
                                                    FdecConsts cst) {
  const uint64_t slots = 1ull + m + k, gi = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (gi >= n * slots) return;
  const uint64_t s = gi / slots;
  const uint32_t slot = static_cast<uint32_t>(gi % slots);
  const uint8_t *pr = trimmed + s * (k + m);
  uint32_t *b = blk + s * words;
  const uint16_t *lg = logs + s * W;
  if (slot == 0) {
    uint32_t e = 0, used = 0;
    for (uint32_t g = 0; g < k; g++) e += pr[g] ? 0u : 1u;
    for (uint32_t p = 0; p < m; p++) used += pr[k + p] ? 1u : 0u;
    if (status) status[s] = used < e ? 2 : (e > max_e ? 14 : 0);  // NotEnoughShards / InvalidArgument
    for (uint32_t i = 0; i < mko; i++) b[i] = 0;
    for (uint32_t g = 0; g < k; g++) b[dwm + 3 + g] = 0xFFFFFFFFu;
    if (used < e) return;  // nothing restored
    uint32_t row = 0;  // more than max_e erased: the first max_e are restored (status 14)
    for (uint32_t g = 0; g < k; g++)
      if (!pr[g]) {
        b[g / 32] |= 1u << (g % 32);
        if (row < max_e) {
          b[dwm + 3 + g] = row++;
          b[dwm] |= 1u << ((C + g) / C);
        }
      }
    for (uint32_t p = 0; p < m; p++)
      if (pr[k + p]) b[dwm + 1 + p / 32] |= 1u << (p % 32);
    return;
  }
  uint32_t c = 0;
  if (slot <= m) {
    const uint32_t p = slot - 1;
    if (pr[k + p]) c = exp[lg[p]];  // root.zig:292-295
  } else {
    const uint32_t g = slot - 1 - m;
    if (!pr[g]) c = mul16_d(cst.beta[(C + g) / C], 65535u - lg[C + g], exp, log);  // root.zig:321-326
  }
  uint32_t *M = b + mko + 128u * (slot - 1);
  uint32_t cu[8], cv[8];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    cu[j] = c ? to_uv_d(mul16_d(to_uv_d(1u << j, cst), log[c], exp, log), cst) : 0u;
    cv[j] = c ? to_uv_d(mul16_d(to_uv_d(1u << (8 + j), cst), log[c], exp, log), cst) : 0u;
  }
  for (int i = 0; i < 8; i++)
    for (int j = 0; j < 8; j++) {
      M[16 * i + j] = ((cu[j] >> i & 1) ? 0x0F0F0F0Fu : 0u) | ((cv[j] >> (8 + i) & 1) ? 0xF0F0F0F0u : 0u);
      M[16 * i + 8 + j] = ((cv[j] >> i & 1) ? 0x0F0F0F0Fu : 0u) | ((cu[j] >> (8 + i) & 1) ? 0xF0F0F0F0u : 0u);
    }
}

hipError_t launch_fdec_plan(const uint8_t *present, uint64_t present_stride, uint32_t k, uint32_t m, uint32_t C,
                            uint32_t W, uint64_t n, uint32_t max_e, const uint16_t *d_exp, const uint16_t *d_log,
                            const uint16_t *d_log_walsh, uint8_t *trimmed, uint16_t *logs, uint32_t *blk,
                            uint32_t dwm, uint32_t mko, uint32_t words, const FdecConsts &cst, int32_t *status,
                            hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (W / C > 32 || mko < dwm + 3 + k || words < mko + 128 * (m + k)) return hipErrorInvalidValue;
  trace_launch("k_trim_present");
  trace_launch("k_erasure_logs");
  trace_launch("k_fdec_block");
  hipLaunchKernelGGL(k_trim_present, dim3(static_cast<uint32_t>((n + 255) / 256)), dim3(256), 0, s, present,
                     present_stride, k, m, n, trimmed);
  hipError_t e = hipGetLastError();
  for (uint64_t s0 = 0; e == hipSuccess && s0 < n; s0 += 65535) {
    const uint32_t cnt = static_cast<uint32_t>(std::min<uint64_t>(65535, n - s0));
    hipLaunchKernelGGL(k_erasure_logs, dim3(cnt), dim3(1024), 0, s, trimmed + s0 * (k + m), static_cast<uint64_t>(k + m),
                       k, m, C, W, 0u, d_log_walsh, d_log, logs + s0 * W);
    e = hipGetLastError();
  }
  if (e != hipSuccess) return e;
  const uint64_t threads = n * (1ull + m + k);
  hipLaunchKernelGGL(k_fdec_block, dim3(static_cast<uint32_t>((threads + 255) / 256)), dim3(256), 0, s, trimmed, k, m, C,
                     W, n, max_e, logs, d_exp, d_log, dwm, mko, words, blk, status, cst);
  return hipGetLastError();
}

hipError_t launch_trim_present(const uint8_t *present, uint64_t present_stride, uint32_t k, uint32_t m, uint64_t n,
                               uint8_t *out, hipStream_t s) {
  trace_launch("k_trim_present");
  hipLaunchKernelGGL(k_trim_present, dim3(static_cast<uint32_t>((n + 255) / 256)), dim3(256), 0, s, present,
                     present_stride, k, m, n, out);
  return hipGetLastError();
}

}  // namespace rs
