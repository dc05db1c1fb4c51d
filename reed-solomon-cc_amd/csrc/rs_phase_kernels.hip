// rs_phase_kernels.hip — the phase kernels for gfx950 (MI355X), one launch per transform phase:
// the generic reconstruct for any W (launch_decode_generic, k_dphase), the low-rate encode for
// C >= 64 (launch_encode_low_phases, k_ephase) and the low-rate reconstruct in block form
// (launch_low_blocks: k_ephase, k_lbfin1, k_lbfinal, k_dphase).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "rs_device.hpp"
#include "rs_internal.hpp"
#include "rs_xform.hpp"

namespace rs {
namespace {

using dev::Sym;
using dev::Tab;
using dev::fft_sub;
using dev::group_fence;
using dev::ifft_sub;
using dev::opq;
using dev::opqu;
using dev::row_rsrc;
using dev::zero_rsrc;

// ---- the generic reconstruct as a launch sequence (launch_decode_generic): one launch per
// phase of xform_ph, the phase's sub-problems across the grid (y), so a small batch still
// fills the chip. Grid: x = column units, y = sub-problem, z = stripes (strided).
// Per stripe the scratch holds X (W positions: the IFFT, in place; then A, written over X by
// the first FFT phase) and B (the positions the truncated FFT still needs after its first
// phase; decode_generic_rows). The steps ride
// on the phases:
//  * GATHER (first IFFT phase): positions come from the received shards * pre, zero where
//    nothing was received (root.zig:291-303), instead of a staging pass;
//  * the IFFT writes only positions < round_up(trunc, span): a sub-problem past the
//    truncation is all zero and so is what it would write (the next phase reads zeros);
//  * the formal derivative (root.zig:306-312) is out[p] = in[p] ^ XOR over clear bits b of
//    p of in[p + 2^b] (every read an original value): D = I + H + L, H the bits the first
//    FFT phase F1 holds (it spans every position), L the bits below its stride. L acts on
//    the low bits only and F1 on the high bits only (its twiddles depend on the group, not
//    on the low bits), so F1 D = F1 (I + H) + L F1. DERIV (first FFT phase): H in VGPRs
//    (ascending, reads above writes), A = F1((I + H) X); SPLITB: the same sub-problem
//    again without H, B = F1(X); LSUM (second FFT phase): A + L B, L's bits the
//    sub-problem holds in VGPRs, the ones below its stride as loads of B (none for
//    W = 2048). No partner loads of X (tests/test_decode_phases_model.py checks this
//    against the layer-by-layer decode);
//  * the FFT writes only positions < round_up(trunc_fft, span) and skips sub-problems past
//    the truncation (their outputs feed nothing: root.zig:318 reads [0, trunc));
//  * SCATTER (last FFT phase): only the erased positions, * post, into the restored rows
//    (root.zig:320-326).
enum : int { kPhGather = 1, kPhDeriv = 2, kPhScatter = 4, kPhSplitB = 8, kPhLsum = 16 };

struct PhaseArgs {
  const uint8_t *src = nullptr;  // stripe s's input: src + s * src_stride, position p at + p * sb
  uint8_t *dst = nullptr;        // output (in place: dst == src)
  uint64_t src_stride = 0, dst_stride = 0, n_src = 0, n_dst = 0;  // >= n_src read as zero, >= n_dst not stored
  uint64_t sb = 0, size = 0, rmax = 0, ti = 0;
  const RsTab *tabs = nullptr;
  uint32_t dlo_log = 0;
  const uint8_t *src2 = nullptr;  // LSUM: B (stride src_stride)
  uint8_t *dst2 = nullptr;        // SPLITB: B (stride dst_stride)
  bool contig = false;            // shard rows in the contiguous lane layout (shard_bytes % 512 == 0)
  // NI > 0 (the first FFT phase): the IFFT's last phase runs on the loaded rows first
  const RsTab *tabs_i = nullptr;
  uint64_t ti_i = 0, rmax_i = 0;
  uint32_t dlo_i = 0;
  // k_ephase SYN (low-rate block form): the recovery rows and the syndrome multipliers
  const uint8_t *rec = nullptr;
  uint64_t rec_stride = 0;
  const int32_t *syn_idx = nullptr;
  const RsTab *syn_tab = nullptr;
};

// Table pointers made opaque inside the stripe / pass loops: a group's table loads are then
// issued where the group runs. Hoisted out of the loops (the tables do not depend on the
// stripe), every group's tables stayed live across them, 21 SGPRs each: 1,200-2,300 SGPRs
// spilled into VGPR lanes per 64-point phase kernel and 250+ VGPRs, one wave per SIMD (round 5).
__device__ __forceinline__ PhaseArgs opq(const PhaseArgs &q) {
  PhaseArgs r = q;
  r.tabs = opq(r.tabs);
  r.tabs_i = opq(r.tabs_i);
  r.syn_tab = opq(r.syn_tab);
  r.dlo_log = opqu(r.dlo_log);  // the row offsets (blk + lo + (j << dlo_log)) * sb likewise
  return r;
}

// The IFFT's last phase inside the first FFT phase's sub-problem: that sub-problem (fixed
// position bits below dlo_f, registers j over the bits above) is the union of G = N / NI of
// the IFFT phase's sub-problems (bits below dlo_i = dlo_f + log2 G fixed): group g holds
// registers g + t G, t < NI (tests/test_decode_phases_model.py)
template <int N, int NI>
__device__ __forceinline__ void ifft_last_in(Sym<1> *v, const PhaseArgs &q) {
  if constexpr (NI > 0) {
    constexpr int G = N / NI;
#pragma unroll
    for (int g = 0; g < G; g++) {
      Sym<1> w[NI];
#pragma unroll
      for (int t = 0; t < NI; t++) w[t] = v[g + t * G];
      ifft_sub<NI, 1>(w, opq(q.tabs_i), q.ti_i, q.size, q.rmax_i, 0, q.dlo_i);  // the groups share tables
#pragma unroll
      for (int t = 0; t < NI; t++) v[g + t * G] = w[t];
    }
  }
}

// scratch rows (X, A, B): lane u's 4 symbols as one 8-byte (lo, hi) pair at u * 8, so a
// wave's access is 512 contiguous bytes (one dwordx2 per lane); only the shard rows keep the
// reference's chunk layout (Generic.zig:152-156)
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void ldp(Sym<1> &s, __amdgpu_buffer_rsrc_t r, uint32_t o) {
  const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(r, o, 0, 0);
  s.l[0] = v.x;
  s.h[0] = v.y;
}
__device__ __forceinline__ void stp(__amdgpu_buffer_rsrc_t r, uint32_t o, const Sym<1> &s) {
  u32x2 v;
  v.x = s.l[0];
  v.y = s.h[0];
  __builtin_amdgcn_raw_buffer_store_b64(v, r, o, 0, 0);
}

// a shard row's lo / hi halves (raw: dev::pair_halves) through r; no records: zeros, no store
__device__ __forceinline__ void ld_shard(Sym<1> &s, __amdgpu_buffer_rsrc_t r, uint32_t io, uint32_t io_h) {
  s.l[0] = __builtin_amdgcn_raw_buffer_load_b32(r, io, 0, 0);
  s.h[0] = __builtin_amdgcn_raw_buffer_load_b32(r, io_h, 0, 0);
}
__device__ __forceinline__ void st_shard(__amdgpu_buffer_rsrc_t r, uint32_t io, uint32_t io_h, const Sym<1> &s) {
  __builtin_amdgcn_raw_buffer_store_b32(s.l[0], r, io, 0, 0);
  __builtin_amdgcn_raw_buffer_store_b32(s.h[0], r, io_h, 0, 0);
}

// The formal derivative's terms of register j over the register bits from B0 up: acc ^= XOR over
// clear bits bb >= B0 of j of v[j + bb] (ascending j may write v[j]: reads lie above writes)
template <int N, int B0>
__device__ __forceinline__ void deriv_terms(Sym<1> &acc, const Sym<1> *v, int j) {
#pragma unroll
  for (int bb = B0; bb < N; bb <<= 1)
    if (!(j & bb)) dev::xor_into(acc, v[j + bb]);
}

template <int N, bool INV, int MODE, int NI = 0>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(3))) void k_dphase(DecodeArgs a, PhaseArgs q0) {
  const PhaseArgs &q = q0;
  // lane unit u (4 symbols of one shard column); lanes past the shard's last unit stay (the
  // lane reads below need every lane): they load at offset 0 and store nothing
  const uint64_t sb = q.sb, u = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const bool act = u < sb / 8;
  const uint32_t so = act ? static_cast<uint32_t>(u * 8) : 0u;  // scratch offset
  // shard-row offset: the contiguous lane layout (512-B waves, lo / hi halves paired by a
  // lane swap) where the shard is whole 512-B waves, else 4 + 4 bytes of one 64-B chunk
  const uint32_t io = act ? dev::lane_byte_offset<1>(u / 64, static_cast<uint32_t>(u % 64), q.contig) : 0u;
  const uint32_t io_h = io + (q.contig ? 256u : 32u);
  const uint64_t sub = blockIdx.y, dlo = 1ull << q.dlo_log;
  const uint64_t blk = (sub >> q.dlo_log) * (static_cast<uint64_t>(N) << q.dlo_log), lo = sub & (dlo - 1);
  for (uint64_t s = blockIdx.z; s < a.n_stripes; s += gridDim.z) {
    const PhaseArgs q = opq(q0);
    Sym<1> v[N];
    if constexpr ((MODE & kPhSplitB) != 0) {  // B = F1(X), the sub-problem without H: first,
      // since A is then written over X (in place: the lane reads its positions before it
      // writes them, and no other lane or workgroup touches them; decode_generic_rows)
      const uint8_t *x = q.src + s * q.src_stride;
      uint8_t *y = q.dst2 + s * q.dst_stride;
#pragma unroll
      for (int j = 0; j < N; j++) {
        const uint64_t p = blk + lo + (static_cast<uint64_t>(j) << q.dlo_log);
        if (p < q.n_src) ldp(v[j], row_rsrc(x + p * sb), so);
        else dev::zero(v[j]);
      }
      ifft_last_in<N, NI>(v, q);
      fft_sub<N, 1>(v, q.tabs, q.ti, q.size, q.rmax, blk, q.dlo_log);
      const uint32_t dls = opqu(q.dlo_log);  // store offsets recomputed, not held across the transform
#pragma unroll
      for (int j = 0; j < N; j++) {
        const uint64_t p = blk + lo + (static_cast<uint64_t>(j) << dls);
        if (act && p < q.n_dst) stp(row_rsrc(y + p * sb), so, v[j]);
      }
    }
    if constexpr ((MODE & kPhGather) != 0) {
      // the sub-problem's sources in one vector load (lane j: position j), then per position
      // a lane read and a load through a buffer resource with no records when nothing was
      // received (reads zero): no scalar load, wait and branch in front of every load
      const uint8_t *orig = a.orig + s * a.orig_stripe_stride;
      const uint8_t *rec = a.rec + s * a.rec_stripe_stride;
      const RsTab *tab_pre = a.tab_pre + s * a.pattern_stride;
      const int32_t *pos_src = a.pos_src + s * a.pattern_stride;
      const uint32_t ln = __lane_id();
      const uint64_t lp = blk + lo + (static_cast<uint64_t>(ln) << q.dlo_log);
      const int32_t my = ln < static_cast<uint32_t>(N) && lp < q.n_src ? pos_src[lp] : -1;
      int32_t srcs[N];
#pragma unroll
      for (int j = 0; j < N; j++) {
        srcs[j] = __builtin_amdgcn_readlane(my, j);
        const uint8_t *row = ((srcs[j] & kSrcRecovery) ? rec : orig) + static_cast<uint64_t>(srcs[j] & kSrcIndexMask) * sb;
        const __amdgpu_buffer_rsrc_t r = srcs[j] >= 0 ? row_rsrc(row) : zero_rsrc();
        ld_shard(v[j], r, io, io_h);
      }
      if (q.contig)  // pair after every load is issued (a swap behind its own load waits for it)
#pragma unroll
        for (int j = 0; j < N; j++) dev::pair_halves(v[j], true);
#pragma unroll
      for (int j = 0; j < N; j++) {
        if (srcs[j] >= 0) dev::mul_inplace(v[j], dev::load_tab(tab_pre + blk + lo + (static_cast<uint64_t>(j) << q.dlo_log)));
        group_fence();
      }
    } else if constexpr ((MODE & kPhLsum) != 0) {
      const uint8_t *A = q.src + s * q.src_stride, *B = q.src2 + s * q.src_stride;
#pragma unroll
      for (int j = 0; j < N; j++) {
        const uint64_t p = blk + lo + (static_cast<uint64_t>(j) << q.dlo_log);
        if (p < q.n_src) ldp(v[j], row_rsrc(B + p * sb), so);
        else dev::zero(v[j]);
      }
#pragma unroll
      for (int j = 0; j < N; j++) {  // L's bits in VGPRs: v[j] = XOR over clear bits of B[j + bb]
        Sym<1> t;
        dev::zero(t);
        deriv_terms<N, 1>(t, v, j);
        v[j] = t;
      }
      for (uint32_t b = 0; b < q.dlo_log; b++) {  // L's bits below the stride: loads of B
        if ((lo >> b) & 1) continue;                // wave-uniform
#pragma unroll
        for (int j = 0; j < N; j++) {
          const uint64_t p = blk + lo + (1ull << b) + (static_cast<uint64_t>(j) << q.dlo_log);
          if (p < q.n_src) {
            Sym<1> t;
            ldp(t, row_rsrc(B + p * sb), so);
            dev::xor_into(v[j], t);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < N; j++) {
        const uint64_t p = blk + lo + (static_cast<uint64_t>(j) << q.dlo_log);
        if (p < q.n_src) {
          Sym<1> t;
          ldp(t, row_rsrc(A + p * sb), so);
          dev::xor_into(v[j], t);
        }
      }
    } else {
      const uint8_t *x = q.src + s * q.src_stride;
      const uint32_t dll = opqu(q.dlo_log);  // not the SPLITB loads' offsets, held across its FFT
#pragma unroll
      for (int j = 0; j < N; j++) {
        const uint64_t p = blk + lo + (static_cast<uint64_t>(j) << dll);
        if (p < q.n_src) ldp(v[j], row_rsrc(x + p * sb), so);
        else dev::zero(v[j]);
      }
      ifft_last_in<N, NI>(v, q);
      if constexpr ((MODE & kPhDeriv) != 0) {  // H: the bits this sub-problem holds
#pragma unroll
        for (int j = 0; j < N; j++)  // in place, not through deriv_terms: that reorders these kernels' code
#pragma unroll
          for (int bb = 1; bb < N; bb <<= 1)
            if (!(j & bb)) dev::xor_into(v[j], v[j + bb]);
      }
    }
    if constexpr (INV) ifft_sub<N, 1>(v, q.tabs, q.ti, q.size, q.rmax, blk, q.dlo_log);
    else fft_sub<N, 1>(v, q.tabs, q.ti, q.size, q.rmax, blk, q.dlo_log);
    if constexpr ((MODE & kPhScatter) != 0) {
      uint8_t *out = a.out + s * a.out_stripe_stride;
      const RsTab *tab_post = a.tab_post + s * a.pattern_stride;
      const int32_t *pos_dst = a.pos_dst + s * a.pattern_stride;
      const uint32_t ln = __lane_id();
      const uint64_t lp = blk + lo + (static_cast<uint64_t>(ln) << q.dlo_log);
      const int32_t my = ln < static_cast<uint32_t>(N) && lp < q.rmax ? pos_dst[lp] : -1;
#pragma unroll
      for (int j = 0; j < N; j++) {
        const int32_t dst = __builtin_amdgcn_readlane(my, j);
        if (dst >= 0) {  // wave-uniform
          dev::mul_inplace(v[j], dev::load_tab(tab_post + blk + lo + (static_cast<uint64_t>(j) << q.dlo_log)));
          if (q.contig) dev::pair_halves(v[j], true);  // back to the lo / hi halves (an involution)
          const __amdgpu_buffer_rsrc_t r = act ? row_rsrc(out + static_cast<uint64_t>(dst) * sb) : zero_rsrc();
          st_shard(r, io, io_h, v[j]);
        }
        group_fence();
      }
    } else {
      uint8_t *y = q.dst + s * q.dst_stride;
      const uint32_t dls = opqu(q.dlo_log);  // store offsets recomputed, not held across the transform
#pragma unroll
      for (int j = 0; j < N; j++) {
        const uint64_t p = blk + lo + (static_cast<uint64_t>(j) << dls);
        if (act && p < q.n_dst) stp(row_rsrc(y + p * sb), so, v[j]);
      }
    }
  }
}

// ---- the low-rate generic encode as one launch per transform phase (launch_encode_low_phases):
// coefficients = IFFT_C(originals at [0, k), trunc k) in region 0 of the stripe's scratch
// (the first phase gathers the original rows); recovery chunk j = FFT_C(coefficients, skew
// (j+1)C, trunc t_j = min(C, m - jC)) in region 1 + (j - chunk0), its last phase storing
// the recovery rows jC + p directly. The IFFT's last phase runs inside the first FFT
// phase's loads (as launch_decode_generic does), so region 0 is read, never rewritten, by
// every chunk. Grid y = (chunk of the launch, sub-problem) for the FFT phases.
// SYN (the low-rate reconstruct in block form, launch_low_blocks): the last FFT phase of block
// K = j + 1 forms the residual's syndromes instead of storing recovery rows, and the gather
// reads the originals flagged in a.skip (the erased ones) as zero.
// DLO (an IFFT phase of 64 contiguous positions, launch_low_blocks): besides its output U, the
// phase stores W = ((1 + gamma) I + D_lo) U to dst2 (1 + gamma: the block's table at syn_tab),
// D_lo the formal derivative's terms over the bits the phase holds (bits 0-5): the later IFFT
// phases act on higher bits with twiddles that do not depend on these, so they commute with D_lo
// and k_lbfin1 gets (1 + gamma) U + D_lo U of the final IFFT output by running the last IFFT
// phase on W.
enum : int { kEpGather = 1, kEpOut = 2, kEpFft = 4, kEpSyn = 8, kEpDlo = 16 };

template <int N, int MODE, int NI>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(3))) void k_ephase(EncodeArgs a, PhaseArgs q0, uint32_t subs, uint32_t from_chunk) {
  const PhaseArgs &q = q0;
  const uint64_t sb = q.sb, u = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const bool act = u < sb / 8;
  const uint32_t so = act ? static_cast<uint32_t>(u * 8) : 0u;
  const uint32_t io = act ? dev::lane_byte_offset<1>(u / 64, static_cast<uint32_t>(u % 64), q.contig) : 0u;
  const uint32_t io_h = io + (q.contig ? 256u : 32u);
  constexpr bool kFft = (MODE & kEpFft) != 0;
  const uint64_t C = q.size, dlo = 1ull << q.dlo_log;
  const uint32_t sl = static_cast<uint32_t>(__builtin_ctz(subs | (1u << 31)));  // subs: a power of two
  const uint32_t ch = kFft ? blockIdx.y >> sl : 0u;  // chunk of this launch (scalar shifts, not a VALU divide)
  const uint64_t sub = kFft ? blockIdx.y & (subs - 1) : blockIdx.y;
  const uint64_t blk = (sub >> q.dlo_log) * (static_cast<uint64_t>(N) << q.dlo_log), lo = sub & (dlo - 1);
  const uint64_t j = a.chunk0 + ch;  // recovery chunk
  const uint64_t rmax = kFft ? (a.m - j * C < C ? a.m - j * C : C) : q.rmax;
  if (kFft && blk >= rmax) return;  // wave-uniform: outputs past the chunk's truncation feed nothing
  const uint64_t n_dst = kFft ? (rmax + dlo - 1) / dlo * dlo : q.n_dst;  // what later phases read
  for (uint64_t s = blockIdx.z; s < a.n_stripes; s += gridDim.z) {
    const PhaseArgs q = opq(q0);
    const RsTab *tabs = kFft ? q.tabs + j * a.tabs_per_chunk : q.tabs;
    Sym<1> v[N];
    const uint8_t *x = q.src + s * q.src_stride + (from_chunk ? (1 + ch) * C * sb : 0);
    if constexpr ((MODE & kEpGather) != 0) {
      const uint8_t *d = a.data + s * a.data_stripe_stride;
#pragma unroll
      for (int jj = 0; jj < N; jj++) {
        const uint64_t p = blk + lo + (static_cast<uint64_t>(jj) << q.dlo_log);
        const bool rd = p < q.n_src && !skipped(a, static_cast<uint32_t>(p));
        const __amdgpu_buffer_rsrc_t r = rd ? row_rsrc(d + p * sb) : zero_rsrc();
        ld_shard(v[jj], r, io, io_h);
      }
      if (q.contig)
#pragma unroll
        for (int jj = 0; jj < N; jj++) dev::pair_halves(v[jj], true);
    } else {
#pragma unroll
      for (int jj = 0; jj < N; jj++) {
        const uint64_t p = blk + lo + (static_cast<uint64_t>(jj) << q.dlo_log);
        if (p < q.n_src) ldp(v[jj], row_rsrc(x + p * sb), so);
        else dev::zero(v[jj]);
      }
      ifft_last_in<N, NI>(v, q);
    }
    if constexpr (kFft) fft_sub<N, 1>(v, tabs, q.ti, C, rmax, blk, q.dlo_log);
    else ifft_sub<N, 1>(v, tabs, q.ti, C, rmax, blk, q.dlo_log);
    if constexpr ((MODE & kEpSyn) != 0) {
      // recovery row r = jC + p: (rec_r ^ Enc(d')_r) L_r sigma_K where r is a row used, else
      // zero; the rows in groups of 8 loads (lane jj holds position jj's row flag)
      const uint8_t *rc = q.rec + s * q.rec_stride + j * C * sb;
      const int32_t *si = q.syn_idx + j * C;
      const RsTab *st = q.syn_tab + j * C;
      uint8_t *y = q.dst + s * q.dst_stride + (1 + ch) * C * sb;
      const uint32_t ln = __lane_id();
      const uint64_t lp = blk + lo + (static_cast<uint64_t>(ln) << q.dlo_log);
      const int32_t my = ln < static_cast<uint32_t>(N) && lp < rmax ? si[lp] : -1;
      constexpr int G8 = N < 8 ? N : 8;
#pragma unroll
      for (int g0 = 0; g0 < N; g0 += G8) {
        Sym<1> t[G8];
#pragma unroll
        for (int jj = 0; jj < G8; jj++) {
          const uint64_t p = blk + lo + (static_cast<uint64_t>(g0 + jj) << q.dlo_log);
          const bool used = __builtin_amdgcn_readlane(my, g0 + jj) >= 0;
          const __amdgpu_buffer_rsrc_t r = used ? row_rsrc(rc + p * sb) : zero_rsrc();  // wave-uniform
          ld_shard(t[jj], r, io, io_h);
        }
        if (q.contig)
#pragma unroll
          for (int jj = 0; jj < G8; jj++) dev::pair_halves(t[jj], true);
#pragma unroll
        for (int jj = 0; jj < G8; jj++) {
          const uint64_t p = blk + lo + (static_cast<uint64_t>(g0 + jj) << q.dlo_log);
          if (__builtin_amdgcn_readlane(my, g0 + jj) >= 0) {  // wave-uniform
            dev::xor_into(v[g0 + jj], t[jj]);
            dev::mul_inplace(v[g0 + jj], dev::load_tab(st + p));
          } else {
            dev::zero(v[g0 + jj]);
          }
          if (act && p < rmax) stp(row_rsrc(y + p * sb), so, v[g0 + jj]);
          group_fence();
        }
      }
    } else if constexpr ((MODE & kEpOut) != 0) {
      uint8_t *par = a.parity + s * a.parity_stripe_stride + j * C * sb;
#pragma unroll
      for (int jj = 0; jj < N; jj++) {
        const uint64_t p = blk + lo + (static_cast<uint64_t>(jj) << q.dlo_log);
        if (p < rmax) {  // wave-uniform
          if (q.contig) dev::pair_halves(v[jj], true);
          const __amdgpu_buffer_rsrc_t r = act ? row_rsrc(par + p * sb) : zero_rsrc();
          st_shard(r, io, io_h, v[jj]);
        }
      }
    } else {
      uint8_t *y = q.dst + s * q.dst_stride + (kFft ? (1 + ch) * C * sb : 0);
      const uint32_t dls = opqu(q.dlo_log);  // store offsets recomputed, not held across the transform
#pragma unroll
      for (int jj = 0; jj < N; jj++) {
        const uint64_t p = blk + lo + (static_cast<uint64_t>(jj) << dls);
        if (act && p < n_dst) stp(row_rsrc(y + p * sb), so, v[jj]);
      }
      if constexpr ((MODE & kEpDlo) != 0) {  // W = ((1 + gamma) I + D_lo) U, ascending (reads above writes)
        const Tab g1 = dev::load_tab(q.syn_tab);
#pragma unroll
        for (int jj = 0; jj < N; jj++) {
          Sym<1> t = v[jj];
          dev::mul_inplace(t, g1);
          deriv_terms<N, 1>(t, v, jj);
          v[jj] = t;
          group_fence();
        }
        uint8_t *w = q.dst2 + s * q.dst_stride;
        const uint32_t dlw = opqu(q.dlo_log);
#pragma unroll
        for (int jj = 0; jj < N; jj++) {
          const uint64_t p = blk + lo + (static_cast<uint64_t>(jj) << dlw);
          if (act && p < n_dst) stp(row_rsrc(w + p * sb), so, v[jj]);
        }
      }
    }
  }
}

// The final FFT's first phase for the block form with the derivative applied whole before it
// (IFFTs of two phases, C <= 4096): block K's U = IFFT_last(U_pre) and
// IFFT_last(W) = (1 + gamma) U + D_lo U (W from k_ephase DLO) are formed in VGPRs, then
// Z = D_hi U + IFFT_last(W) = D_C U + gamma U (D_hi: the derivative's terms over the bits the
// last IFFT phase holds, register bits >= G = N / NI of this sub-problem) for u = 1, Z = U for
// u = 0, and A' += F1(Z) (acc: add to what an earlier block stored). The next phase is then a
// plain FFT phase with the scatter: no B' and no LSUM.
template <int NI>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(3))) void k_lbfin1(uint64_t n_stripes,
                                                                                         PhaseArgs q0, uint32_t u,
                                                                                         uint32_t acc) {
  const PhaseArgs &q = q0;
  constexpr int N = 64, G = N / NI;
  const uint64_t sb = q.sb, uu = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const bool act = uu < sb / 8;
  const uint32_t so = act ? static_cast<uint32_t>(uu * 8) : 0u;
  const uint64_t sub = blockIdx.y, dlo = 1ull << q.dlo_log;
  const uint64_t blk = (sub >> q.dlo_log) * (static_cast<uint64_t>(N) << q.dlo_log), lo = sub & (dlo - 1);
  for (uint64_t s = blockIdx.z; s < n_stripes; s += gridDim.z) {
    const PhaseArgs q = opq(q0);
    const uint8_t *x = q.src + s * q.src_stride;
    Sym<1> v[N];
#pragma unroll
    for (int j = 0; j < N; j++) {
      const uint64_t p = blk + lo + (static_cast<uint64_t>(j) << q.dlo_log);
      if (p < q.n_src) ldp(v[j], row_rsrc(x + p * sb), so);
      else dev::zero(v[j]);
    }
    ifft_last_in<N, NI>(v, q);
    if (u) {
#pragma unroll
      for (int j = 0; j < N; j++) {  // D_hi U, ascending (reads above writes)
        Sym<1> t;
        dev::zero(t);
        deriv_terms<N, G>(t, v, j);
        v[j] = t;
      }
      const uint8_t *wq = q.src2 + s * q.src_stride;
      const uint32_t dlw = opqu(q.dlo_log);
#pragma unroll
      for (int gg = 0; gg < G; gg++) {  // + IFFT_last(W), one group of the last IFFT phase at a time
        Sym<1> w[NI];
#pragma unroll
        for (int t = 0; t < NI; t++) {
          const uint64_t p = blk + lo + (static_cast<uint64_t>(gg + t * G) << dlw);
          if (p < q.n_src) ldp(w[t], row_rsrc(wq + p * sb), so);
          else dev::zero(w[t]);
        }
        ifft_sub<NI, 1>(w, opq(q.tabs_i), q.ti_i, q.size, q.rmax_i, 0, q.dlo_i);
#pragma unroll
        for (int t = 0; t < NI; t++) dev::xor_into(v[gg + t * G], w[t]);
        group_fence();  // one group's W rows live at a time
      }
    }
    fft_sub<N, 1>(v, q.tabs, q.ti, q.size, q.rmax, blk, q.dlo_log);
    uint8_t *y = q.dst + s * q.dst_stride;
    const uint32_t dls = opqu(q.dlo_log);
    if (acc) {
#pragma unroll
      for (int j = 0; j < N; j++) {
        const uint64_t p = blk + lo + (static_cast<uint64_t>(j) << dls);
        if (p < q.n_dst) {
          Sym<1> o;
          ldp(o, row_rsrc(y + p * sb), so);
          dev::xor_into(v[j], o);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < N; j++) {
      const uint64_t p = blk + lo + (static_cast<uint64_t>(j) << dls);
      if (act && p < q.n_dst) stp(row_rsrc(y + p * sb), so, v[j]);
    }
  }
}

// The low-rate reconstruct in block form (launch_low_blocks): the final FFT's (skew 0) first
// phase with block K's IFFT_{C, skew KC} last phase fused in (ifft_last_in), adding block K's
// share of A' = F1(U' + V) and B' = F1(U) (U = D_C's argument, U' = (I + H) U as k_dphase's
// DERIV, V the blocks' plain terms) to what the earlier blocks stored (acc): the block's
// syndromes were scaled by sigma_K, so its U term is b (u = 1) or none (u = 0) and its V term
// gamma b (the first block stores B' = 0 when it has no U term). k_dphase's LSUM then forms
// A' + L B' = F1 (D_C U + V).
template <int NI, int PASS>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(3))) void k_lbfinal(uint64_t n_stripes, PhaseArgs q0, const RsTab *gamma, uint32_t u,
                                                    uint32_t acc) {
  // PASS 0: B' (u = 0: zeros, stored by the first block only); PASS 1: A' (one launch each:
  // a pass loop kept both passes' addresses live, 250+ VGPRs)
  const PhaseArgs &q = q0;
  constexpr int N = 64;
  const uint64_t sb = q.sb, uu = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const bool act = uu < sb / 8;
  const uint32_t so = act ? static_cast<uint32_t>(uu * 8) : 0u;
  const uint64_t sub = blockIdx.y, dlo = 1ull << q.dlo_log;
  const uint64_t blk = (sub >> q.dlo_log) * (static_cast<uint64_t>(N) << q.dlo_log), lo = sub & (dlo - 1);
  for (uint64_t s = blockIdx.z; s < n_stripes; s += gridDim.z) {
    const PhaseArgs q = opq(q0);
    const uint8_t *x = q.src + s * q.src_stride;
    Sym<1> v[N];
#pragma unroll
    for (int j = 0; j < N; j++) {
      const uint64_t p = blk + lo + (static_cast<uint64_t>(j) << q.dlo_log);
      if (p < q.n_src && (PASS == 1 || u)) ldp(v[j], row_rsrc(x + p * sb), so);
      else dev::zero(v[j]);
    }
    ifft_last_in<N, NI>(v, q);
    if (PASS == 1 && u) {  // v = (I + H) v + gamma v, ascending (reads above writes)
      const Tab g = dev::load_tab(opq(gamma));
#pragma unroll
      for (int j = 0; j < N; j++) {
        Sym<1> t = v[j];
        dev::mul_inplace(t, g);
#pragma unroll
        for (int bb = 1; bb < N; bb <<= 1)  // in place, as in k_dphase's DERIV
          if (!(j & bb)) dev::xor_into(v[j], v[j + bb]);
        dev::xor_into(v[j], t);
        group_fence();  // one product live at a time (all 64 scheduled first: 247 VGPRs)
      }
    }
    fft_sub<N, 1>(v, q.tabs, q.ti, q.size, q.rmax, blk, q.dlo_log);
    uint8_t *y = (PASS == 0 ? q.dst2 : q.dst) + s * q.dst_stride;
    const uint32_t dls = opqu(q.dlo_log);  // output offsets recomputed, not held across the transform
    if (acc) {
#pragma unroll
      for (int j = 0; j < N; j++) {
        const uint64_t p = blk + lo + (static_cast<uint64_t>(j) << dls);
        if (p < q.n_dst) {
          Sym<1> o;
          ldp(o, row_rsrc(y + p * sb), so);
          dev::xor_into(v[j], o);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < N; j++) {
      const uint64_t p = blk + lo + (static_cast<uint64_t>(j) << dls);
      if (act && p < q.n_dst) stp(row_rsrc(y + p * sb), so, v[j]);
    }
  }
}

}  // namespace

// the phases of xform_ph (same grouping): size N, lowest distance 2^dlo_log, first table
void xform_phases(uint64_t size, bool inv, std::vector<XPhase> &out) {
  uint32_t lg = 0;
  while ((1ull << lg) < size) lg++;
  const uint32_t n4 = lg / 2;
  uint32_t layer = 0;
  bool r2_done = !(lg & 1);
  uint64_t ti = 0;
  out.clear();
  do {
    const uint32_t c = std::min<uint32_t>(3, n4 - layer);
    const bool with_r2 = !r2_done && layer + c == n4 && c < 3;
    const uint32_t nn = (1u << (2 * c)) << (with_r2 ? 1 : 0);
    out.push_back({nn, inv ? 2 * layer : (with_r2 || c == 0 ? 0 : lg - 2 * (layer + c)), ti});
    for (uint32_t l = layer; l < layer + c; l++) ti += inv ? 3 * (size >> (2 * l + 2)) : 3ull << (2 * l);
    layer += c;
    r2_done = r2_done || with_r2 || c == 0;
  } while (layer < n4 || !r2_done);
}

// positions of the FFT's A and B buffers: those the phases after the first read (0 for one phase)
static uint64_t decode_y_rows(uint64_t W, uint64_t rmax_fft) {
  std::vector<XPhase> ph;
  xform_phases(W, false, ph);
  return ph.size() > 1 ? std::min(W, round_up(rmax_fft, 1ull << ph[0].dlo_log)) : 0;
}

// X (A written over it in place) | B. The first FFT phase reads every position of its
// sub-problem from X before it writes that sub-problem's A rows, and sub-problems are disjoint,
// so A needs no buffer of its own (X | A | B took ~3W rows per stripe at W = 65536)
uint64_t decode_generic_rows(uint64_t W, uint64_t trunc, uint64_t trunc_fft) {
  return W + decode_y_rows(W, trunc_fft ? trunc_fft : trunc);
}

// ---- launches. The kernel templates' sizes come from run-time phase shapes: for_size calls
// f(std::integral_constant<int, N>) for the power of two n == N in [2, 64] that MASK holds and
// returns the launch's error, hipErrorInvalidValue for any other n. MASK: the sub-problem sizes a
// mode runs with for W = 64 .. 65536 (xform_phases): the first phases and the middle ones are 64
// points, only the last phases vary (instantiating just those keeps the build time down).
template <int MASK, int N = 2, class F>
static hipError_t for_size(uint32_t n, F &&f) {
  if constexpr (N <= 64) {
    if constexpr ((MASK & N) != 0) {
      if (n == N) {
        f(std::integral_constant<int, N>{});
        return hipGetLastError();
      }
    }
    return for_size<MASK, 2 * N>(n, f);
  }
  return hipErrorInvalidValue;
}

template <bool INV, int MODE, int NS>
static hipError_t launch_dphase(uint32_t n, dim3 g, const DecodeArgs &a, const PhaseArgs &q, hipStream_t s) {
  return for_size<NS>(n, [&](auto N) {
    hipLaunchKernelGGL((k_dphase<decltype(N)::value, INV, MODE>), g, dim3(kBlock), 0, s, a, q);
  });
}

// the first FFT phase with the IFFT's last phase fused in (64-point sub-problems)
static hipError_t launch_dphase_fused(uint32_t ni, dim3 g, const DecodeArgs &a, const PhaseArgs &q, hipStream_t s) {
  return for_size<126>(ni, [&](auto NI) {
    hipLaunchKernelGGL((k_dphase<64, false, kPhDeriv | kPhSplitB, decltype(NI)::value>), g, dim3(kBlock), 0, s, a, q);
  });
}

template <int MODE, int NS>
static hipError_t launch_ephase(uint32_t n, uint32_t ni, dim3 g, const EncodeArgs &a, const PhaseArgs &q, uint32_t subs,
                                uint32_t fc, hipStream_t s) {
  if (ni) {  // the first FFT phase with the IFFT's last phase: 64-point sub-problems
    if constexpr (MODE == kEpFft) {  // (never also the last phase, never an IFFT phase)
      if (n != 64) return hipErrorInvalidValue;
      return for_size<126>(ni, [&](auto NI) {
        hipLaunchKernelGGL((k_ephase<64, MODE, decltype(NI)::value>), g, dim3(kBlock), 0, s, a, q, subs, fc);
      });
    }
    return hipErrorInvalidValue;
  }
  return for_size<NS>(n, [&](auto N) {
    hipLaunchKernelGGL((k_ephase<decltype(N)::value, MODE, 0>), g, dim3(kBlock), 0, s, a, q, subs, fc);
  });
}

static hipError_t launch_lbfin1(uint32_t ni, dim3 g, uint64_t n, const PhaseArgs &q, uint32_t u, uint32_t acc,
                                hipStream_t s) {
  return for_size<126>(ni, [&](auto NI) {
    hipLaunchKernelGGL((k_lbfin1<decltype(NI)::value>), g, dim3(kBlock), 0, s, n, q, u, acc);
  });
}

static hipError_t launch_lbfinal(uint32_t ni, dim3 g, uint64_t n, const PhaseArgs &q, const RsTab *gamma, uint32_t u,
                                 uint32_t acc, hipStream_t s) {
  return for_size<126>(ni, [&](auto NI) {
    if (u || !acc) hipLaunchKernelGGL((k_lbfinal<decltype(NI)::value, 0>), g, dim3(kBlock), 0, s, n, q, gamma, u, acc);
    hipLaunchKernelGGL((k_lbfinal<decltype(NI)::value, 1>), g, dim3(kBlock), 0, s, n, q, gamma, u, acc);
  });
}

// what the phases of one launch sequence share: the transform in place on a stripe's rows at
// buf (`stride` bytes a stripe), the shard size, the transform size; every other field zero
static PhaseArgs phase_common(uint8_t *buf, uint64_t stride, uint64_t sb, uint64_t size) {
  PhaseArgs c;
  c.src = c.dst = buf;
  c.src_stride = c.dst_stride = stride;
  c.sb = sb, c.size = size, c.contig = contig_ok(sb, 1);
  return c;
}
// one phase of the transform with the tables `tabs`; n_src, n_dst and rmax are the caller's
static PhaseArgs phase_args(PhaseArgs q, const XPhase &ph, const RsTab *tabs) {
  q.ti = ph.ti, q.dlo_log = ph.dlo_log, q.tabs = tabs;
  return q;
}
// the first FFT phase with the last phase of the IFFT of tables tabs_i, truncation rmax_i, in its loads
static void fuse_ifft_last(PhaseArgs &q, const XPhase &last, const RsTab *tabs_i, uint64_t rmax_i) {
  q.tabs_i = tabs_i, q.ti_i = last.ti, q.rmax_i = rmax_i, q.dlo_i = last.dlo_log;
}

// The first `count` phases of an IFFT in place (q: phase_common, the tables, the truncation rmax
// and, as n_src, the rows the first phase reads). A phase writes only the positions below
// round_up(rmax, span) (a sub-problem past the truncation is all zero) and the next reads just
// those: on return q.n_src is what the last phase wrote. launch(i, q, g) starts phase i.
template <class L>
static hipError_t ifft_phases(const std::vector<XPhase> &iph, size_t count, PhaseArgs &q, dim3 g0, L &&launch) {
  for (size_t i = 0; i < count; i++) {
    q = phase_args(q, iph[i], q.tabs);
    q.n_dst = round_up(q.rmax, static_cast<uint64_t>(iph[i].n) << iph[i].dlo_log);
    const dim3 g(g0.x, static_cast<uint32_t>(q.n_dst / iph[i].n), g0.z);
    if (hipError_t e = launch(i, q, g)) return e;
    q.n_src = q.n_dst;
  }
  return hipSuccess;
}

// The FFT's phases after the first, in place on A (q: A with its rows as n_src and n_dst, the
// tables, the truncation rmax, and B as src2 and dst2, null where the derivative was applied whole
// before the FFT): LSUM in the second phase where there is a B, SCATTER in the last. No fourth
// FFT phase below W = 2^19.
static hipError_t fft_tail_phases(const std::vector<XPhase> &fph, const DecodeArgs &a, PhaseArgs q, dim3 g0,
                                  hipStream_t s) {
  const bool lsum = q.src2 != nullptr;
  for (size_t i = 1; i < fph.size(); i++) {
    const bool last = i + 1 == fph.size();
    const uint32_t n = fph[i].n;
    q = phase_args(q, fph[i], q.tabs);
    const dim3 g(g0.x, static_cast<uint32_t>(round_up(q.rmax, static_cast<uint64_t>(n) << fph[i].dlo_log) / n), g0.z);
    hipError_t e = lsum && i == 1 ? (last ? launch_dphase<false, kPhLsum | kPhScatter, 126>(n, g, a, q, s)
                                          : launch_dphase<false, kPhLsum, 64>(n, g, a, q, s))
                   : !last        ? hipErrorInvalidValue
                   : lsum         ? launch_dphase<false, kPhScatter, 30>(n, g, a, q, s)
                                  : launch_dphase<false, kPhScatter, 126>(n, g, a, q, s);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// Decoder.decode (root.zig:268-335) over any W as one launch per transform phase
// (a.scratch: decode_generic_rows positions per stripe)
hipError_t launch_decode_generic(const DecodeArgs &a, hipStream_t s) {
  const uint64_t W = a.work, sb = a.shard_bytes;
  if (W < 2 || (W & (W - 1)) || W > 65536 || sb % 64) return hipErrorInvalidValue;
  const uint64_t ri = std::min<uint64_t>(a.trunc, W), rf = std::min<uint64_t>(a.trunc_fft ? a.trunc_fft : a.trunc, W);
  const uint64_t ylen = decode_y_rows(W, rf);
  uint8_t *X = a.scratch, *B = X + W * sb;  // A in place over X (decode_generic_rows)
  const PhaseArgs c = phase_common(X, (W + ylen) * sb, sb, W);
  const dim3 g0(grid_for(sb, 1, 1).x, 1, static_cast<uint32_t>(std::min<uint64_t>(a.n_stripes, 65535)));
  std::vector<XPhase> fph, iph;
  xform_phases(W, true, iph);
  xform_phases(W, false, fph);
  // with two or more IFFT phases the last one runs inside the first FFT phase's loads (its
  // sub-problems are the union of G of the IFFT phase's): one pass over X less, and X read
  // before it is the previous phase's output
  const bool fuse = iph.size() >= 2;
  PhaseArgs qi = phase_args(c, iph[0], a.tab_ifft);
  qi.rmax = qi.n_src = ri;
  hipError_t e = ifft_phases(iph, fuse ? iph.size() - 1 : iph.size(), qi, g0, [&](size_t i, const PhaseArgs &q, dim3 g) {
    return i == 0 ? launch_dphase<true, kPhGather, 64>(iph[i].n, g, a, q, s)
                  : launch_dphase<true, 0, 64>(iph[i].n, g, a, q, s);
  });
  if (e != hipSuccess) return e;
  // the first FFT phase: W = 64 (one phase each way) or fused with the IFFT's last phase (W >= 128)
  const bool one = fph.size() == 1;
  if (fuse && (fph[0].n != 64 || one || (64u >> (iph.back().dlo_log - fph[0].dlo_log)) != iph.back().n))
    return hipErrorInvalidValue;  // the shapes xform_phases gives every W >= 128
  PhaseArgs q = phase_args(c, fph[0], a.tab_fft);
  q.n_src = fuse ? qi.n_src : W, q.n_dst = ylen, q.rmax = rf;
  q.src2 = q.dst2 = B;
  if (fuse) fuse_ifft_last(q, iph.back(), a.tab_ifft, ri);
  const uint64_t wl = round_up(rf, static_cast<uint64_t>(fph[0].n) << fph[0].dlo_log);
  const dim3 g(g0.x, static_cast<uint32_t>(wl / fph[0].n), g0.z);
  e = one    ? launch_dphase<false, kPhDeriv | kPhScatter, 64>(fph[0].n, g, a, q, s)
      : fuse ? launch_dphase_fused(iph.back().n, g, a, q, s)
             : hipErrorInvalidValue;
  if (e != hipSuccess) return e;
  q.n_src = ylen;
  return fft_tail_phases(fph, a, q, g0, s);
}

// rs_gf.hpp scalar_encode_low as phase launches (k_ephase); a.scratch: a.regions C-row
// regions per stripe (coefficients + one per recovery chunk of a launch), chunk groups of
// regions - 1 as launch_encode_low's generic path
hipError_t launch_encode_low_phases(const EncodeArgs &a, hipStream_t s) {
  const uint64_t C = a.chunk, sb = a.shard_bytes, k = a.k;
  if (C < 64 || (C & (C - 1)) || sb % 64) return hipErrorInvalidValue;
  const uint32_t R = a.regions ? a.regions : 1 + a.n_chunks, G = R - 1;
  if (G == 0) return hipErrorInvalidValue;
  const PhaseArgs c = phase_common(a.scratch, static_cast<uint64_t>(R) * C * sb, sb, C);
  const dim3 g0(grid_for(sb, 1, 1).x, 1, static_cast<uint32_t>(std::min<uint64_t>(a.n_stripes, 65535)));
  const uint64_t ri = std::min<uint64_t>(k, C);
  std::vector<XPhase> iph, fph;
  xform_phases(C, true, iph);
  xform_phases(C, false, fph);
  const bool fuse = iph.size() >= 2;
  PhaseArgs qi = phase_args(c, iph[0], a.tabs);
  qi.rmax = qi.n_src = ri;
  hipError_t e = ifft_phases(iph, fuse ? iph.size() - 1 : iph.size(), qi, g0, [&](size_t i, const PhaseArgs &q, dim3 g) {
    return i == 0 ? launch_ephase<kEpGather, 64>(iph[i].n, 0, g, a, q, 0, 0, s)
                  : launch_ephase<0, 64>(iph[i].n, 0, g, a, q, 0, 0, s);
  });
  if (e != hipSuccess) return e;
  const uint64_t TI = ifft_tab_count(C);
  for (uint32_t j0 = 0; j0 < a.n_chunks; j0 += G) {
    EncodeArgs b = a;
    b.chunk0 = j0;
    const uint32_t nc = std::min(G, a.n_chunks - j0);
    for (size_t i = 0; i < fph.size(); i++) {
      const bool first = i == 0, last = i + 1 == fph.size();
      const uint32_t subs = static_cast<uint32_t>(C / fph[i].n);
      if (static_cast<uint64_t>(subs) * nc > 65535) return hipErrorInvalidValue;
      // first: reads region 0 (the coefficients, with the IFFT's last phase fused in when
      // there is one); the others read their chunk's region. n_dst and rmax: per chunk, in the kernel
      PhaseArgs q = phase_args(c, fph[i], a.tabs + TI);
      const uint32_t ni = first && fuse ? iph.back().n : 0, fc = first ? 0u : 1u;
      if (ni && (fph[i].n != 64 || (64u >> (iph.back().dlo_log - fph[i].dlo_log)) != ni)) return hipErrorInvalidValue;
      q.n_src = ni ? qi.n_src : C;
      if (ni) fuse_ifft_last(q, iph.back(), a.tabs, ri);
      const dim3 g(g0.x, subs * nc, g0.z);
      e = last ? launch_ephase<kEpFft | kEpOut, 126>(fph[i].n, ni, g, b, q, subs, fc, s)
               : launch_ephase<kEpFft, 64>(fph[i].n, ni, g, b, q, subs, fc, s);
      if (e != hipSuccess) return e;
    }
  }
  return hipSuccess;
}

// per stripe: coefficients (C) | block K's transform (C) | A' and B' (the final FFT's first-phase
// rows the later phases read)
static uint64_t low_block_ylen(uint64_t C, uint64_t k) {
  std::vector<XPhase> fph;
  xform_phases(C, false, fph);
  return round_up(k, 1ull << fph[0].dlo_log);
}
// the derivative applied whole (k_ephase DLO + k_lbfin1) where the IFFT has two phases
static bool low_block_whole(uint64_t C) {
  std::vector<XPhase> iph, fph;
  xform_phases(C, true, iph);
  xform_phases(C, false, fph);
  return iph.size() == 2 && fph.size() == 2 && iph[0].n == 64 && iph[0].dlo_log == 0;
}
// per stripe: X (coefficients) | R1 (block K's transform) | then W (its (I + D_lo) copy) | A'
// for the whole derivative, A' | B' for the split one
uint64_t low_block_rows(uint64_t C, uint64_t k) {
  return low_block_whole(C) ? 3 * C + low_block_ylen(C, k) : 2 * C + 2 * low_block_ylen(C, k);
}

// rs_lowrate.cpp's block form as phase launches (scalar_reconstruct_low_blocks step by step):
//  1. coefficients of d' = IFFT_C(originals, erased ones zero, trunc k): its phases but the last
//     (k_ephase GATHER with a.skip), region 0;
//  2. per block K = j + 1 holding rows used: FFT_{C, skew KC}(coefficients) (the IFFT's last
//     phase fused into its first, as launch_encode_low_phases), its last phase forming the
//     syndromes (SYN) into region 1; the IFFT_{C, skew KC} of those, in place, but its last
//     phase, which runs inside k_lbfinal (the final FFT's first phase, accumulating A', B');
//  3. the final FFT's later phases: LSUM (A' + L B', D_C's low bits) and SCATTER (the erased
//     originals times exp(-L_g)) as launch_decode_generic's.
hipError_t launch_low_blocks(const LowBlockArgs &L, hipStream_t s) {
  const EncodeArgs &a = L.enc;
  const uint64_t C = a.chunk, sb = a.shard_bytes, k = a.k, mp = a.m;
  if (C < 128 || (C & (C - 1)) || C > 32768 || sb % 64 || k == 0 || k > C || mp == 0 || a.n_chunks == 0 ||
      mp > static_cast<uint64_t>(a.n_chunks) * C)
    return hipErrorInvalidValue;
  std::vector<XPhase> iph, fph;
  xform_phases(C, true, iph);
  xform_phases(C, false, fph);
  if (iph.size() < 2 || fph.size() < 2 || fph.size() > 3 || fph[0].n != 64 ||
      (64u >> (iph.back().dlo_log - fph[0].dlo_log)) != iph.back().n || (64ull << fph[0].dlo_log) != C)
    return hipErrorInvalidValue;  // the shapes xform_phases gives every C in [128, 32768]
  trace_launch("low_blocks");
  const uint64_t ylen = low_block_ylen(C, k);
  // two IFFT phases (C <= 4096): the derivative whole before the final FFT (k_ephase DLO +
  // k_lbfin1), so the final FFT's second phase is plain; else the A' / B' split (k_lbfinal, LSUM)
  const bool whole = low_block_whole(C);
  uint8_t *X = a.scratch, *R1 = X + C * sb, *Wr = whole ? X + 2 * C * sb : nullptr;
  uint8_t *Ap = X + (whole ? 3 : 2) * C * sb, *Bp = whole ? nullptr : Ap + ylen * sb;
  const PhaseArgs c = phase_common(X, low_block_rows(C, k) * sb, sb, C);
  const dim3 g0(grid_for(sb, 1, 1).x, 1, static_cast<uint32_t>(std::min<uint64_t>(a.n_stripes, 65535)));
  const uint64_t TI = ifft_tab_count(C);
  PhaseArgs qc = phase_args(c, iph[0], a.tabs);  // 1.
  qc.rmax = qc.n_src = k;
  hipError_t e = ifft_phases(iph, iph.size() - 1, qc, g0, [&](size_t i, const PhaseArgs &q, dim3 g) {
    return i == 0 ? launch_ephase<kEpGather, 64>(iph[i].n, 0, g, a, q, 0, 0, s)
                  : launch_ephase<0, 64>(iph[i].n, 0, g, a, q, 0, 0, s);
  });
  if (e != hipSuccess) return e;
  // 2. only the blocks holding a row used: an empty block's syndromes are zero and so is its
  // contribution (linear), so the first block run stores A' (B') and later ones accumulate
  bool stored = false;
  for (uint32_t j = 0; j < a.n_chunks; j++) {
    if (L.used && !L.used[j]) continue;
    EncodeArgs b = a;
    b.chunk0 = j;
    const uint64_t rj = std::min<uint64_t>(C, mp - static_cast<uint64_t>(j) * C);
    for (size_t i = 0; i < fph.size(); i++) {
      const bool first = i == 0, last = i + 1 == fph.size();
      const uint32_t subs = static_cast<uint32_t>(C / fph[i].n);
      PhaseArgs q = phase_args(c, fph[i], a.tabs + TI);
      q.n_src = first ? qc.n_src : C;
      if (first) fuse_ifft_last(q, iph.back(), a.tabs, k);
      q.rec = L.rec, q.rec_stride = L.rec_stripe_stride;
      q.syn_idx = L.syn_idx, q.syn_tab = L.syn_tab;
      const dim3 g(g0.x, subs, g0.z);
      e = last ? launch_ephase<kEpFft | kEpSyn, 126>(fph[i].n, 0, g, b, q, subs, 1, s)
               : launch_ephase<kEpFft, 64>(fph[i].n, first ? iph.back().n : 0, g, b, q, subs, first ? 0 : 1, s);
      if (e != hipSuccess) return e;
    }
    const RsTab *ti = L.tabs_i + static_cast<uint64_t>(j) * TI;
    PhaseArgs qr = phase_args(c, iph[0], ti);  // region 1 in place, rows past rj zero
    qr.src = qr.dst = R1;
    qr.rmax = qr.n_src = rj;
    qr.dst2 = Wr, qr.syn_tab = L.gamma1 + j;  // DLO: W and 1 + gamma of block K
    e = ifft_phases(iph, iph.size() - 1, qr, g0, [&](size_t i, const PhaseArgs &q, dim3 g) {
      return whole ? launch_ephase<kEpDlo, 64>(iph[i].n, 0, g, b, q, 0, 0, s)
                   : launch_ephase<0, 64>(iph[i].n, 0, g, b, q, 0, 0, s);
    });
    if (e != hipSuccess) return e;
    PhaseArgs q = phase_args(c, fph[0], L.dec.tab_fft);
    q.src = R1, q.src2 = Wr, q.n_src = qr.n_src;
    q.dst = Ap, q.dst2 = Bp, q.n_dst = ylen;
    q.rmax = k;
    fuse_ifft_last(q, iph.back(), ti, rj);
    const dim3 g(g0.x, static_cast<uint32_t>(C / 64), g0.z);
    e = whole ? launch_lbfin1(iph.back().n, g, a.n_stripes, q, L.u[j], stored ? 1u : 0u, s)
              : launch_lbfinal(iph.back().n, g, a.n_stripes, q, L.gamma + j, L.u[j], stored ? 1u : 0u, s);
    if (e != hipSuccess) return e;
    stored = true;
  }
  if (!stored) return hipErrorInvalidValue;  // no row used: the plan never asks for the block form
  DecodeArgs d = L.dec;  // 3.
  d.n_stripes = a.n_stripes;
  d.pattern_stride = 0;
  PhaseArgs q = phase_args(c, fph[1], L.dec.tab_fft);
  q.src = q.dst = Ap, q.src2 = q.dst2 = Bp;
  q.n_src = q.n_dst = ylen, q.rmax = k;
  return fft_tail_phases(fph, d, q, g0, s);
}

}  // namespace rs
