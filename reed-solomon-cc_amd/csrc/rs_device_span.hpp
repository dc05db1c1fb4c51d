// rs_device_span.hpp — what the two locates (rs_locate_kernels.hip, rs_locate_multi_kernels.hip)
// share on the device beyond the lane loads of rs_device_lanes.hpp: the work item of the scrub
// family, the byte offsets of a symbol, and the one pass both run over a stripe's syndromes:
// does S_r(p) == sum_j B_j[r] * S_{piv_j}(p) hold for every row r of a group and every symbol p of
// a segment.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "rs_device.hpp"
#include "rs_device_lanes.hpp"

namespace rs {
namespace dev {

// A work item of the scrub family is (stripe, group of up to kRows rows, segment of kSeg bytes of
// every shard). kSeg is a multiple of 16 (segment starts keep the shard's alignment) and of 64
// (whole chunks); tests/scrub_sweep.py's SEG is this value.
constexpr uint32_t kSeg = 16384;
constexpr uint32_t kSegSyms = kSeg / 2;  // symbols of a whole segment
constexpr uint32_t kRows = 16;
constexpr uint32_t kNoSym = 0xFFFFFFFFu;

// Symbols of a shard of sb bytes, in the order of the whole chunks' low bytes, then the tail
// chunk's (tests/locate_model.py symbol_of / symbol_bytes). A whole 64-byte chunk holds 32 symbols,
// low bytes at [0, 32), high bytes at [32, 64); the tail chunk of t = sb % 64 bytes holds h = t / 2,
// low bytes at [0, h), high bytes at [h, t).
__device__ __forceinline__ uint64_t symbol_of(uint64_t sb, uint64_t o) {  // the symbol byte o belongs to
  const uint32_t t = static_cast<uint32_t>(sb % 64);
  const uint64_t whole = sb - t;
  return o < whole ? o / 64 * 32 + o % 32 : whole / 2 + static_cast<uint32_t>(o - whole) % (t / 2);
}
__device__ __forceinline__ void symbol_bytes(uint64_t sb, uint64_t p, uint64_t &lo, uint64_t &hi) {
  const uint64_t t = sb % 64, half = (sb - t) / 2;  // half: the symbols of the whole chunks
  lo = p < half ? p / 32 * 64 + p % 32 : p + half;
  hi = lo + (p < half ? 32 : t / 2);
}

// One work item's part of the span check: rows [r_lo, r_hi) of segment `seg` (of `segs`) of the
// stripe whose syndromes are a ^ b (both [rows][sb]), against the NT pivot rows piv[0, NT) with
// the multiply table of (pivot j, row r) at tab_of(j, r), a wave-uniform address. Returns the
// lane's smallest failing symbol, counted from the segment's first, or kNoSym. POS false: only
// whether one failed is wanted (0 or kNoSym), and no position is computed. NT == 0 is the scan for
// a nonzero syndrome; it reads only the rows whose flag[r] is set.
// 256 lanes; the tail chunk goes by bytes on lanes 0-7 of wave 0. The loop bounds are
// workgroup-uniform (a lane past the end re-reads unit 0 and drops the result), so the table loads
// stay scalar.
template <int MODE, int NT, bool POS, class TabOf>
__device__ __forceinline__ uint32_t span_check(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b,
                                               uint64_t sb, uint64_t seg, uint64_t segs, uint32_t r_lo, uint32_t r_hi,
                                               const uint32_t *piv, const uint8_t *flag, TabOf tab_of) {
  constexpr int NV = Lanes<MODE>::NV, ND = POS ? NV : 1;     // ND: the words a lane's differences are kept in
  constexpr uint32_t kUnitsPerChunk = 8 / NV, kLo = 4 * NV;  // a unit: kLo low + kLo high bytes of one chunk
  constexpr int NP = NT > 0 ? NT : 1;
  const uint32_t t = static_cast<uint32_t>(sb % 64), tid = threadIdx.x;
  const uint64_t whole = sb - t, base = seg * kSeg;
  const uint8_t *pa = a + base, *pb = b + base;
  const uint32_t wb = base < whole ? static_cast<uint32_t>(whole - base < kSeg ? whole - base : kSeg) : 0;
  const uint32_t units = wb / 64 * kUnitsPerChunk;
  uint32_t at = kNoSym, any = 0;
  for (uint32_t u0 = 0; u0 < units; u0 += 256u) {
    const bool live = u0 + tid < units;
    const uint32_t u = live ? u0 + tid : 0;
    const uint32_t off = u / kUnitsPerChunk * 64 + u % kUnitsPerChunk * kLo;
    uint32_t dd[ND];
#pragma unroll
    for (int v = 0; v < ND; v++) dd[v] = 0;
    if constexpr (NT == 0) {
      for (uint32_t r = r_lo; r < r_hi; r++) {
        if (!flag[r]) continue;
        Sym<NV> sr;
        ld_xor<MODE>(sr, pa + r * sb + off, pb + r * sb + off);
#pragma unroll
        for (int v = 0; v < NV; v++) dd[POS ? v : 0] |= sr.l[v] | sr.h[v];
      }
    } else {
      Sym<NV> sp[NP], sr;
#pragma unroll
      for (int j = 0; j < NT; j++) ld_xor<MODE>(sp[j], pa + piv[j] * sb + off, pb + piv[j] * sb + off);
      ld_xor<MODE>(sr, pa + r_lo * sb + off, pb + r_lo * sb + off);
      for (uint32_t r = r_lo; r < r_hi; r++) {
        Sym<NV> next = sr, acc;
        // the next row's loads are in flight while this row is multiplied
        if (r + 1 < r_hi) ld_xor<MODE>(next, pa + (r + 1) * sb + off, pb + (r + 1) * sb + off);
        zero(acc);
#pragma unroll
        for (int j = 0; j < NT; j++) {
          const Tab tab = load_tab(tab_of(j, r));
          mul_add(acc, sp[j], tab);
        }
#pragma unroll
        for (int v = 0; v < NV; v++) dd[POS ? v : 0] |= (acc.l[v] ^ sr.l[v]) | (acc.h[v] ^ sr.h[v]);
        sr = next;
      }
    }
    if constexpr (POS) {
      if (live) {
        const uint32_t first = u / kUnitsPerChunk * 32 + u % kUnitsPerChunk * kLo;  // the unit's first symbol
#pragma unroll
        for (int v = NV - 1; v >= 0; v--)
          if (dd[v]) at = min(at, first + 4u * v + (static_cast<uint32_t>(__builtin_ctz(dd[v])) >> 3));
      }
    } else {
      any |= live ? dd[0] : 0u;
    }
  }
  if (t != 0 && seg == segs - 1 && tid < 64) {  // the tail chunk: lanes 0-7 hold its symbols
    const uint8_t *ta = a + whole, *tb = b + whole;
    const uint32_t lane = tid < 8 ? tid : 0, h = t / 2;
    uint32_t dd = 0;
    if constexpr (NT == 0) {
      for (uint32_t r = r_lo; r < r_hi; r++) {
        Sym<1> sr;
        ld_xor_tail(sr, ta + r * sb, tb + r * sb, h, lane);
        dd |= sr.l[0] | sr.h[0];
      }
    } else {
      Sym<1> sp[NP];
#pragma unroll
      for (int j = 0; j < NT; j++) ld_xor_tail(sp[j], ta + piv[j] * sb, tb + piv[j] * sb, h, lane);
      for (uint32_t r = r_lo; r < r_hi; r++) {
        Sym<1> sr, acc;
        ld_xor_tail(sr, ta + r * sb, tb + r * sb, h, lane);
        zero(acc);
#pragma unroll
        for (int j = 0; j < NT; j++) {
          const Tab tab = load_tab(tab_of(j, r));
          mul_add(acc, sp[j], tab);
        }
        dd |= (acc.l[0] ^ sr.l[0]) | (acc.h[0] ^ sr.h[0]);
      }
    }
    // symbols past the tail's h read as zero on both sides: they never differ
    if constexpr (POS) {
      if (tid < 8 && dd) at = min(at, wb / 2 + 4u * lane + (static_cast<uint32_t>(__builtin_ctz(dd)) >> 3));
    } else {
      any |= tid < 8 ? dd : 0u;
    }
  }
  if constexpr (!POS) at = any ? 0u : kNoSym;
  return at;
}

}  // namespace dev
}  // namespace rs
