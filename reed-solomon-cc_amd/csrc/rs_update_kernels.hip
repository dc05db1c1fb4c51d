// rs_update_kernels.hip — the kernels of rs_update_batch_dev (rs_update.cpp):
// the small write. Under the corrected arithmetic parity[r] = sum_j c[r][j] * original[j] over
// GF(2^16), so changing original j from old to new changes recovery shard r by c[r][j] * (old ^ new).
//
// Inputs per slice of stripes: index rows [n][max_u] (the changed originals, kUpdateNone = an
// empty slot), the change buffers d_old / d_new [n][max_u][sb] (d_old == nullptr: d_new already
// holds old ^ new) and the recovery shards [n][m][sb], which are updated in place.
//  * k_update_prepare: one workgroup per stripe validates the row (an LDS bitmap of k bits finds a
//    repeated index), writes the status, compacts the live slots into list[s][0, e_s) as
//    slot << 16 | j with the count live[s] = e_s (0 for a rejected stripe), and builds the e_s * m
//    multiply tables tabs[s][e][r] of c[r][j_e] from the plan's coefficient logs.
//  * k_update_apply: flattened over (stripe, group of up to 16 recovery rows, 16 KiB segment),
//    grid-stride. A work item of a stripe with e_s == 0 reads that word and leaves. Otherwise it
//    holds the deltas of a tile of up to T live slots of the lane's unit in Sym<NV> registers and
//    walks the group's rows, B at a time: load the parity units, mul_add every delta of the tile
//    with the wave-uniform table of (stripe, slot, row), store; the next B rows' loads are issued
//    before the current rows are multiplied (B = 4 rows beside 1 or 2 deltas, 2 beside 3 or 4:
//    with one row in flight per lane the kernel was latency-bound, 6 to 10 % slower at u = 1).
//    Every parity byte belongs to one lane of one work item: no atomics and no hand-off. A stripe
//    with e_s > T takes its further tiles in the same work item, one after the other: each extra
//    tile costs 2 more passes (a load and a store) over the group's parity rows, so T = 4 covers up
//    to 4 changed originals in one pass and 5..8 in two.
// Measured crossover with the encode of the whole stripe (tools/update_bench.py):
// on RS(200,55) the update is ahead at every u measured (1, 2, 4: 0.50 to 0.61 of the encode's
// time); on RS(10,4) at u = 1 (0.84, delta form 0.76) and, barely, u = 2 (0.97), and behind at
// u = 4 (1.4), where traffic alone already says 1.14: re-encode such stripes.
// A kernel boundary separates prepare from apply.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "rs_device.hpp"
#include "rs_device_lanes.hpp"
#include "rs_device_span.hpp"
#include "rs_internal.hpp"

namespace rs {
namespace {

using dev::Lanes;
using dev::Sym;
using dev::Tab;

constexpr uint32_t kUpdateSeg = dev::kSeg, kUpdateRows = dev::kRows;  // the scrub family's work item

// ======================================================================= prepare
// cl [k][m] = log c[r][j]. status may be nullptr.
__global__ __launch_bounds__(256) void k_update_prepare(const uint32_t *__restrict__ index, uint64_t index_stride,
                                                        uint32_t max_u, uint64_t n, uint32_t k, uint32_t m,
                                                        const uint16_t *__restrict__ cl,
                                                        const uint16_t *__restrict__ d_exp,
                                                        const uint16_t *__restrict__ d_log, RsTab *__restrict__ tabs,
                                                        uint32_t *list, uint32_t *__restrict__ live,
                                                        int32_t *__restrict__ status) {
  __shared__ uint32_t sh_seen[kOrder / 32];  // one bit per original (k <= 65536)
  __shared__ uint32_t sh_fault, sh_wave[4];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  for (uint64_t s = blockIdx.x; s < n; s += gridDim.x) {
    __syncthreads();  // the previous stripe's shared words are no longer read
    for (uint32_t w = tid; w < (k + 31u) / 32u; w += 256u) sh_seen[w] = 0;
    if (tid == 0) sh_fault = 0;
    __syncthreads();
    const uint32_t *row = index + s * index_stride;
    uint32_t fault = 0;  // bit 0: an index >= k, bit 1: an index named twice
    for (uint32_t i = tid; i < max_u; i += 256u) {
      const uint32_t j = row[i];
      if (j == kUpdateNone) continue;
      if (j >= k) {
        fault |= 1u;
      } else {
        const uint32_t bit = 1u << (j & 31u);
        if (atomicOr(&sh_seen[j >> 5], bit) & bit) fault |= 2u;
      }
    }
    if (fault) atomicOr(&sh_fault, fault);
    __syncthreads();
    const uint32_t f = sh_fault;  // workgroup-uniform from here
    if (tid == 0 && status)
      status[s] = (f & 1u) ? kUpdateInvalidIndex : (f & 2u) ? kUpdateDuplicateIndex : 0;
    if (f) {
      if (tid == 0) live[s] = 0;
      continue;
    }
    // the live slots in slot order
    uint32_t *ls = list + s * max_u;
    uint32_t e = 0;
    for (uint32_t i0 = 0; i0 < max_u; i0 += 256u) {
      const uint32_t i = i0 + tid;
      const uint32_t j = i < max_u ? row[i] : kUpdateNone;
      const unsigned long long mask = __builtin_amdgcn_ballot_w64(j != kUpdateNone);
      if (lane == 0) sh_wave[wave] = static_cast<uint32_t>(__builtin_popcountll(mask));
      __syncthreads();
      uint32_t at = e, all = 0;
#pragma unroll
      for (uint32_t w = 0; w < 4; w++) {
        at += w < wave ? sh_wave[w] : 0u;
        all += sh_wave[w];
      }
      if (j != kUpdateNone) ls[at + static_cast<uint32_t>(__builtin_popcountll(mask & ((1ull << lane) - 1ull)))] = i << 16 | j;
      e += all;
      __syncthreads();
    }
    if (tid == 0) live[s] = e;
    __threadfence_block();  // the list is read back below by other lanes of this workgroup
    __syncthreads();
    RsTab *ts = tabs + s * max_u * m;
    for (uint32_t q = tid; q < e * m; q += 256u) {
      const uint32_t le = q / m, r = q % m, j = ls[le] & 0xFFFFu;
      dev::build_tab(ts + q, cl[static_cast<uint64_t>(j) * m + r], d_exp, d_log);
    }
  }
}

// ========================================================================= apply
// One tile of NT live slots (list entries ls[0, NT)) applied to rows [r_lo, r_hi) of one segment.
// pn / po: the stripe's change buffers (po may be nullptr); pr: its recovery shards; tb: the tables
// of the tile's first slot, [NT][m].
template <int MODE, int NT>
__device__ __forceinline__ void update_tile(const uint8_t *__restrict__ po, const uint8_t *__restrict__ pn, uint8_t *pr,
                                            uint64_t sb, uint64_t base, uint32_t units, uint32_t tail_h, uint64_t whole,
                                            uint32_t m, uint32_t r_lo, uint32_t r_hi, const uint32_t *__restrict__ ls,
                                            const RsTab *__restrict__ tb) {
  constexpr int NV = Lanes<MODE>::NV;
  constexpr uint32_t kUnitsPerChunk = 8 / NV, kLo = 4 * NV;  // a unit: kLo low + kLo high bytes of one chunk
  constexpr int B = NT <= 2 ? 4 : 2;  // parity rows of a lane in flight (the registers left beside the deltas)
  const uint32_t tid = threadIdx.x;
  uint64_t doff[NT];  // the tile's shards in the change buffers
#pragma unroll
  for (int i = 0; i < NT; i++) doff[i] = static_cast<uint64_t>(ls[i] >> 16) * sb;
  // the loop bounds are workgroup-uniform (a lane past the end re-reads unit 0 and stores
  // nothing), so the table loads stay scalar
  for (uint32_t u0 = 0; u0 < units; u0 += 256u) {
    const bool on = u0 + tid < units;
    const uint32_t u = on ? u0 + tid : 0;
    const uint64_t off = base + u / kUnitsPerChunk * 64 + u % kUnitsPerChunk * kLo;
    Sym<NV> d[NT], p[B];
#pragma unroll
    for (int i = 0; i < NT; i++) {
      if (po) dev::ld_xor<MODE>(d[i], po + doff[i] + off, pn + doff[i] + off);
      else dev::ld<MODE>(d[i], pn + doff[i] + off);
    }
    // B rows at a time; a row past the group re-reads the group's last row and is dropped
#pragma unroll
    for (int b = 0; b < B; b++) dev::ld<MODE>(p[b], pr + min(r_lo + b, r_hi - 1) * sb + off);
    for (uint32_t rb = r_lo; rb < r_hi; rb += B) {
      Sym<NV> next[B];
#pragma unroll
      for (int b = 0; b < B; b++) next[b] = p[b];
      // the next rows' loads are in flight while these rows are multiplied
      if (rb + B < r_hi) {
#pragma unroll
        for (int b = 0; b < B; b++) dev::ld<MODE>(next[b], pr + min(rb + B + b, r_hi - 1) * sb + off);
      }
#pragma unroll
      for (int b = 0; b < B; b++) {
        const uint32_t r = rb + b;
        if (r < r_hi) {
#pragma unroll
          for (int i = 0; i < NT; i++) dev::mul_add(p[b], d[i], dev::load_tab(tb + static_cast<uint64_t>(i) * m + r));
          if (on) dev::st<MODE>(pr + r * sb + off, p[b]);
        }
        p[b] = next[b];
      }
    }
  }
  if (tail_h != 0 && tid < 64) {  // the tail chunk, bytes (wave 0: lanes 0-7 hold its symbols)
    const uint32_t lane = tid < 8 ? tid : 0;
    Sym<1> d[NT];
#pragma unroll
    for (int i = 0; i < NT; i++) {
      if (po) dev::ld_xor_tail(d[i], po + doff[i] + whole, pn + doff[i] + whole, tail_h, lane);
      else dev::ld_tail(d[i], pn + doff[i] + whole, tail_h, lane);
    }
    for (uint32_t r = r_lo; r < r_hi; r++) {
      Sym<1> p;
      dev::ld_tail(p, pr + r * sb + whole, tail_h, lane);
#pragma unroll
      for (int i = 0; i < NT; i++) dev::mul_add(p, d[i], dev::load_tab(tb + static_cast<uint64_t>(i) * m + r));
      if (tid < 8) dev::st_tail(pr + r * sb + whole, p, tail_h, lane);
    }
  }
}

// Work item = (stripe, group of up to kUpdateRows rows, segment). T: the slots of a tile (1, 2, 4).
template <int MODE, int T>
__global__ __launch_bounds__(256) void k_update_apply(const uint8_t *__restrict__ d_old,
                                                      const uint8_t *__restrict__ d_new, uint64_t change_stride,
                                                      uint8_t *rec, uint64_t rec_stride, uint64_t sb, uint64_t n,
                                                      uint32_t m, uint32_t max_u, uint64_t segs, uint32_t groups,
                                                      const uint32_t *__restrict__ list,
                                                      const uint32_t *__restrict__ live,
                                                      const RsTab *__restrict__ tabs) {
  constexpr uint32_t kUnitsPerChunk = 8 / Lanes<MODE>::NV;
  const uint64_t per_stripe = segs * groups, total = n * per_stripe;
  const uint32_t t = static_cast<uint32_t>(sb % 64);
  const uint64_t whole = sb - t;
  for (uint64_t w = blockIdx.x; w < total; w += gridDim.x) {
    const uint64_t s = w / per_stripe, rem = w % per_stripe;
    const uint32_t e = live[s];
    if (e == 0) continue;  // an all-NONE or a rejected row: nothing of the stripe is read or written
    const uint32_t g = static_cast<uint32_t>(rem / segs);
    const uint64_t seg = rem % segs, base = seg * kUpdateSeg;
    const uint32_t r_lo = g * kUpdateRows, r_hi = min(m, r_lo + kUpdateRows);
    const uint8_t *po = d_old ? d_old + s * change_stride : nullptr, *pn = d_new + s * change_stride;
    uint8_t *pr = rec + s * rec_stride;
    const uint32_t wb = base < whole ? static_cast<uint32_t>(whole - base < kUpdateSeg ? whole - base : kUpdateSeg) : 0;
    const uint32_t units = wb / 64 * kUnitsPerChunk;
    const uint32_t tail_h = seg == segs - 1 ? t / 2 : 0;
    const uint32_t *ls = list + s * max_u;
    const RsTab *tb = tabs + s * max_u * m;
    for (uint32_t e0 = 0; e0 < e; e0 += T) {
      const uint32_t nt = min(static_cast<uint32_t>(T), e - e0);
      const RsTab *tt = tb + static_cast<uint64_t>(e0) * m;
      auto tile = [&](auto nt_c) {
        update_tile<MODE, decltype(nt_c)::value>(po, pn, pr, sb, base, units, tail_h, whole, m, r_lo, r_hi, ls + e0, tt);
      };
      if constexpr (T >= 4) {
        if (nt == 4) {
          tile(std::integral_constant<int, 4>());
          continue;
        }
        if (nt == 3) {
          tile(std::integral_constant<int, 3>());
          continue;
        }
      }
      if constexpr (T >= 2) {
        if (nt == 2) {
          tile(std::integral_constant<int, 2>());
          continue;
        }
      }
      tile(std::integral_constant<int, 1>());
    }
  }
}

}  // namespace

hipError_t launch_update_prepare(const uint32_t *index, uint64_t index_stride, uint32_t max_u, uint64_t n, uint32_t k,
                                 uint32_t m, const uint16_t *cl, const uint16_t *d_exp, const uint16_t *d_log,
                                 RsTab *tabs, uint32_t *list, uint32_t *live, int32_t *status, hipStream_t s) {
  if (n == 0) return hipSuccess;
  trace_launch("k_update_prepare");
  const dim3 grid(static_cast<uint32_t>(std::min<uint64_t>(n, 1u << 20)));
  hipLaunchKernelGGL(k_update_prepare, grid, dim3(256), 0, s, index, index_stride, max_u, n, k, m, cl, d_exp, d_log,
                     tabs, list, live, status);
  return hipGetLastError();
}

hipError_t launch_update_apply(const uint8_t *d_old, const uint8_t *d_new, uint64_t change_stride, uint8_t *rec,
                               uint64_t rec_stride, uint64_t sb, uint64_t n, uint32_t m, uint32_t max_u,
                               const uint32_t *list, const uint32_t *live, const RsTab *tabs, hipStream_t s) {
  if (n == 0) return hipSuccess;
  const int mode = load_mode(d_old, d_new, rec, change_stride, rec_stride, sb);
  const int tile = max_u >= 3 ? 4 : static_cast<int>(max_u);
  static const char *const kNames[3][3] = {
      {"k_update_apply_x1_t1", "k_update_apply_x1_t2", "k_update_apply_x1_t4"},
      {"k_update_apply_x4_t1", "k_update_apply_x4_t2", "k_update_apply_x4_t4"},
      {"k_update_apply_x16_t1", "k_update_apply_x16_t2", "k_update_apply_x16_t4"}};
  trace_launch(kNames[mode][tile == 4 ? 2 : tile - 1]);
  const uint64_t segs = (sb + kUpdateSeg - 1) / kUpdateSeg;
  const uint32_t groups = (m + kUpdateRows - 1) / kUpdateRows;
  const dim3 grid(static_cast<uint32_t>(std::min<uint64_t>(n * segs * groups, 1u << 20)));
  with_int(mode, kModes, [&](auto mc) {
    with_int(tile, std::integer_sequence<int, 1, 2, 4>(), [&](auto tc) {
      hipLaunchKernelGGL((k_update_apply<decltype(mc)::value, decltype(tc)::value>), grid, dim3(256), 0, s, d_old, d_new,
                         change_stride, rec, rec_stride, sb, n, m, max_u, segs, groups, list, live, tabs);
    });
  });
  return hipGetLastError();
}

}  // namespace rs
