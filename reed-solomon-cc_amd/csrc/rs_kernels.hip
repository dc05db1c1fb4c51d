// rs_kernels.hip — HIP kernels for gfx950 (MI355X): Reed-Solomon encode and
// reconstruct over GF(2^16) with the additive FFT of usebeforefree/reed-solomon-cc.
//
// Parallelisation: every 64-byte chunk column of a stripe is an
// independent code, so a lane owns NV dword pairs (4*NV symbols) of one column
// and runs the WHOLE codec for it — no cross-lane exchange, no barriers, no LDS.
// Grid: x = column units of one stripe (256 lanes per block), y = stripes.
//
//  * k_encode_reg<C, NV>: fused encode, the chunk-sized transforms in VGPRs.
//    HBM traffic = k shards read + m shards written per stripe (the minimum).
//    Mirrors Encoder.encode (root.zig:136-173).
//  * k_decode_reg<W, NV>: fused reconstruct, the W-point transforms in VGPRs.
//    Reads the k+m-e received shards it needs, writes the e restored ones.
//    Mirrors Decoder.decode (root.zig:268-335).
//  * k_encode_generic: the same encode for any (k, m) through a global scratch work
//    buffer [stripe][W][shard_bytes] (the reference's Shards layout, root.zig:350-395),
//    each lane walking its column (xform_ph). The generic reconstruct and the low-rate
//    codes of 64 positions and more run as one launch per transform phase:
//    rs_phase_kernels.hip.
//  * k_verify_compare / k_verify_count: the compare of rs_verify_batch_dev (an encode into
//    a scratch compared with the stored recovery shards) and the count of its flags.
//  * k_engine_transform / k_mul_scalar: the Engine seam (Generic.zig) as test shims.
// The per-stripe plan kernels are in rs_plan_kernels.hip.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rs_device.hpp"
#include "rs_env.hpp"
#include "rs_internal.hpp"
#include "rs_xform.hpp"

namespace rs {
namespace {

using dev::Sym;
using dev::Tab;
using dev::fft_sub;
using dev::ifft_sub;
using dev::log2_u64;
using dev::opq;
using dev::opqu;
using dev::row_rsrc;

__host__ __device__ constexpr int ifft_tabs_ce(int size) {
  int n = 0, d = 1, d4 = 4;
  for (; d4 <= size; d = d4, d4 <<= 2) n += 3 * (size / d4);
  return n + (d < size ? 1 : 0);
}

// byte offset of this lane's data inside a shard (dev::lane_byte_offset); false
// if the lane's unit is past the shard end (whole waves, see the layouts).
template <int NV>
__device__ __forceinline__ bool lane_offset(uint64_t shard_bytes, bool contig, uint32_t &off) {
  const uint64_t unit = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (unit >= shard_bytes / 64 * (8 / NV)) return false;
  off = dev::lane_byte_offset<NV>(unit / 64, static_cast<uint32_t>(unit % 64), contig);
  return true;
}

// ============================================================ fused encode
template <int C, int NV>
__global__ __launch_bounds__(kBlock) void k_encode_reg(EncodeArgs a) {
  uint32_t off;
  if (!lane_offset<NV>(a.shard_bytes, a.contig, off)) return;
  constexpr int TI = ifft_tabs_ce(C);
  const uint64_t sb = a.shard_bytes;
  {  // one stripe per blockIdx.y (launches are split at 65535 stripes)
    const uint64_t s = blockIdx.y;
    const uint8_t *src = a.data + s * a.data_stripe_stride;
    Sym<NV> acc[C];
    // first chunk: root.zig:143-146
#pragma unroll
    for (int p = 0; p < C; p++) {
      if (static_cast<uint32_t>(p) < a.trunc_first && !skipped(a, p))
        dev::load_sym_raw(acc[p], src + p * sb, off, a.contig);
      else dev::zero(acc[p]);
    }
#pragma unroll
    for (int p = 0; p < C; p++) dev::pair_halves(acc[p], a.contig);
    dev::ifft_regs<C>(acc, a.tabs, a.trunc_first);
    // further chunks, IFFT + XOR-fold: root.zig:148-167
    for (uint32_t j = 1; j < a.n_chunks; j++) {
      const uint32_t t = (j + 1 == a.n_chunks) ? a.trunc_last : static_cast<uint32_t>(C);
      const uint8_t *cs = src + static_cast<uint64_t>(j) * C * sb;
      Sym<NV> cur[C];
#pragma unroll
      for (int p = 0; p < C; p++) {
        if (static_cast<uint32_t>(p) < t && !skipped(a, j * C + p)) dev::load_sym_raw(cur[p], cs + p * sb, off, a.contig);
        else dev::zero(cur[p]);
      }
#pragma unroll
      for (int p = 0; p < C; p++) dev::pair_halves(cur[p], a.contig);
      const RsTab *tj = a.tabs + j * TI;
      asm volatile("" : "+s"(tj));  // opaque base: no per-group pointer IVs (SGPR spills)
      dev::ifft_regs<C>(cur, tj, t);
#pragma unroll
      for (int p = 0; p < C; p++) dev::xor_into(acc[p], cur[p]);
    }
    // root.zig:169
    dev::fft_regs<C>(acc, a.tabs + a.n_chunks * TI, a.m);
    uint8_t *dst = a.parity + s * a.parity_stripe_stride;
#pragma unroll
    for (int p = 0; p < C; p++)
      if (static_cast<uint32_t>(p) < a.m) dev::store_sym(dst + p * sb, off, acc[p], a.contig);
  }
}

// ======================================================= fused reconstruct
// root.zig:309-315 formal derivative over W register slots
template <int W, int NV>
__device__ __forceinline__ void derivative_regs(Sym<NV> *w) {
#pragma unroll
  for (int i = 1; i < W; i++) {
    const int width = i & -i;
#pragma unroll
    for (int j = 0; j < width; j++) dev::xor_into(w[i - width + j], w[i + j]);
  }
}

template <int W, int NV>
__global__ __launch_bounds__(kBlock) void k_decode_reg(DecodeArgs a) {
  uint32_t off;
  if (!lane_offset<NV>(a.shard_bytes, a.contig, off)) return;
  const uint64_t sb = a.shard_bytes;
  {  // one stripe per blockIdx.y (launches are split at 65535 stripes)
    const uint64_t s = blockIdx.y;
    const uint8_t *orig = a.orig + s * a.orig_stripe_stride;
    const uint8_t *rec = a.rec + s * a.rec_stripe_stride;
    // shared plan, or this stripe's own (per-stripe erasure patterns)
    const RsTab *tab_pre = a.tab_pre + s * a.pattern_stride, *tab_post = a.tab_post + s * a.pattern_stride;
    const int32_t *pos_src = a.pos_src + s * a.pattern_stride, *pos_dst = a.pos_dst + s * a.pattern_stride;
    Sym<NV> w[W];
    // erasure masks on received shards, zero elsewhere: root.zig:291-303
#pragma unroll
    for (int p = 0; p < W; p++) {
      const int32_t src = ((const __attribute__((address_space(4))) int32_t *)pos_src)[p];
      if (src >= 0) {
        const uint8_t *base = (src & kSrcRecovery) ? rec : orig;
        dev::load_sym_raw(w[p], base + static_cast<uint64_t>(src & kSrcIndexMask) * sb, off, a.contig);
      } else {
        dev::zero(w[p]);
      }
    }
#pragma unroll
    for (int p = 0; p < W; p++) {  // all loads in flight before the first swap waits
      if (((const __attribute__((address_space(4))) int32_t *)pos_src)[p] >= 0) {
        dev::pair_halves(w[p], a.contig);
        dev::mul_inplace(w[p], dev::load_tab(tab_pre + p));
      }
    }
    dev::ifft_regs<W>(w, a.tab_ifft, a.trunc);  // root.zig:306
    derivative_regs<W>(w);                      // root.zig:309-315
    dev::fft_regs<W>(w, a.tab_fft, a.trunc_fft ? a.trunc_fft : a.trunc);  // root.zig:318
    uint8_t *out = a.out + s * a.out_stripe_stride;
#pragma unroll
    for (int p = 0; p < W; p++) {  // root.zig:321-326
      const int32_t dst = ((const __attribute__((address_space(4))) int32_t *)pos_dst)[p];
      if (dst >= 0) {
        dev::mul_inplace(w[p], dev::load_tab(tab_post + p));
        dev::store_sym(out + static_cast<uint64_t>(dst) * sb, off, w[p], a.contig);
      }
    }
  }
}

// ============================================ wave-split encode, chunk = 64
// For m in 33..64 the 64-point chunk transforms do not fit one lane's VGPRs.
// Four waves share the SAME 64 column units (lanes) and split the positions:
// layout A — wave w holds positions 16w+j (radix-4 stages on bits (0,1), (2,3)
// are wave-local); layout B — wave w holds positions i + 4w + 16q (stage on
// bits (4,5) wave-local). A <-> B is one LDS transpose per chunk. Every twiddle
// a wave needs is still wave-uniform (its group base depends only on w), so
// tables stay in SGPRs. Mirrors Encoder.encode (root.zig:136-173).
template <int NV>
struct LdsSym {
  uint32_t v[2 * NV];
};

template <int NV>
__device__ __forceinline__ void lds_put(LdsSym<NV> *row, uint32_t lane, const Sym<NV> &x) {
  LdsSym<NV> t;
#pragma unroll
  for (int v = 0; v < NV; v++) {
    t.v[2 * v] = x.l[v];
    t.v[2 * v + 1] = x.h[v];
  }
  row[lane] = t;
}

template <int NV>
__device__ __forceinline__ void lds_get(const LdsSym<NV> *row, uint32_t lane, Sym<NV> &x) {
  const LdsSym<NV> t = row[lane];
#pragma unroll
  for (int v = 0; v < NV; v++) {
    x.l[v] = t.v[2 * v];
    x.h[v] = t.v[2 * v + 1];
  }
}

// The scheduling barriers keep the compiler from hoisting the tables of many
// groups at once (each table is 21 SGPRs; hoisting spills SGPRs to VGPR lanes).
template <int NV>
__device__ __forceinline__ void ifft4(Sym<NV> &s0, Sym<NV> &s1, Sym<NV> &s2, Sym<NV> &s3, const RsTab *g) {
  __builtin_amdgcn_sched_barrier(0);
  const Tab m01 = dev::load_tab(g);
  dev::ifft_bf(s0, s1, m01);
  const Tab m23 = dev::load_tab(g + 2);
  dev::ifft_bf(s2, s3, m23);
  const Tab m02 = dev::load_tab(g + 1);
  dev::ifft_bf(s0, s2, m02);
  dev::ifft_bf(s1, s3, m02);
  __builtin_amdgcn_sched_barrier(0);
}

template <int NV>
__device__ __forceinline__ void fft4(Sym<NV> &s0, Sym<NV> &s1, Sym<NV> &s2, Sym<NV> &s3, const RsTab *g) {
  __builtin_amdgcn_sched_barrier(0);
  const Tab m02 = dev::load_tab(g + 1);
  dev::fft_bf(s0, s2, m02);
  dev::fft_bf(s1, s3, m02);
  const Tab m01 = dev::load_tab(g);
  dev::fft_bf(s0, s1, m01);
  const Tab m23 = dev::load_tab(g + 2);
  dev::fft_bf(s2, s3, m23);
  __builtin_amdgcn_sched_barrier(0);
}

// Four radix-4 groups that share one twiddle triple (stages d=4 and d=16 of a
// wave's layout): the three tables are loaded once for the four quads.
template <int NV>
__device__ __forceinline__ void ifft4x4(Sym<NV> *c, const RsTab *g) {
  __builtin_amdgcn_sched_barrier(0);
  const Tab m01 = dev::load_tab(g), m23 = dev::load_tab(g + 2), m02 = dev::load_tab(g + 1);
#pragma unroll
  for (int i = 0; i < 4; i++) {
    dev::ifft_bf(c[i], c[i + 4], m01);
    dev::ifft_bf(c[i + 8], c[i + 12], m23);
    dev::ifft_bf(c[i], c[i + 8], m02);
    dev::ifft_bf(c[i + 4], c[i + 12], m02);
  }
  __builtin_amdgcn_sched_barrier(0);
}

template <int NV>
__device__ __forceinline__ void fft4x4(Sym<NV> *c, const RsTab *g) {
  __builtin_amdgcn_sched_barrier(0);
  const Tab m02 = dev::load_tab(g + 1), m01 = dev::load_tab(g), m23 = dev::load_tab(g + 2);
#pragma unroll
  for (int i = 0; i < 4; i++) {
    dev::fft_bf(c[i], c[i + 8], m02);
    dev::fft_bf(c[i + 4], c[i + 12], m02);
    dev::fft_bf(c[i], c[i + 4], m01);
    dev::fft_bf(c[i + 8], c[i + 12], m23);
  }
  __builtin_amdgcn_sched_barrier(0);
}

// ---- the same encode with each chunk's 63 twiddle tables staged in LDS and read
// back as VGPRs (broadcast ds_read_b128): no SGPR->VGPR moves for the v_perm
// operands and no SGPR spills (k_encode_ws64 holds 3 x 21-SGPR tables and spills
// ~120 SGPRs to VGPR lanes).
__device__ __forceinline__ Tab lds_tab(const uint4 *t) {  // one RsTab = 6 x uint4
  const uint4 q0 = t[0], q1 = t[1], q2 = t[2], q3 = t[3], q4 = t[4], q5 = t[5];
  Tab r;
  const uint32_t lo[10] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y};
  const uint32_t hi[10] = {q2.z, q2.w, q3.x, q3.y, q3.z, q3.w, q4.x, q4.y, q4.z, q4.w};
#pragma unroll
  for (int i = 0; i < 10; i++) {
    r.lo[i] = lo[i];
    r.hi[i] = hi[i];
  }
  r.flags = __builtin_amdgcn_readfirstlane(q5.x);  // uniform: scalar branch on XOR-only twiddles
  return r;
}

// group tables in plan order m01, m02, m23 (push_ifft_tabs / push_fft_tabs)
template <int NV>
__device__ __forceinline__ void ifft4l(Sym<NV> &s0, Sym<NV> &s1, Sym<NV> &s2, Sym<NV> &s3, const uint4 *g) {
  const Tab m01 = lds_tab(g), m02 = lds_tab(g + 6), m23 = lds_tab(g + 12);
  dev::ifft_bf(s0, s1, m01);
  dev::ifft_bf(s2, s3, m23);
  dev::ifft_bf(s0, s2, m02);
  dev::ifft_bf(s1, s3, m02);
}

template <int NV>
__device__ __forceinline__ void fft4l(Sym<NV> &s0, Sym<NV> &s1, Sym<NV> &s2, Sym<NV> &s3, const uint4 *g) {
  const Tab m01 = lds_tab(g), m02 = lds_tab(g + 6), m23 = lds_tab(g + 12);
  dev::fft_bf(s0, s2, m02);
  dev::fft_bf(s1, s3, m02);
  dev::fft_bf(s0, s1, m01);
  dev::fft_bf(s2, s3, m23);
}

template <int NV>
__global__ __launch_bounds__(kBlock) void k_encode_ws64l(EncodeArgs a) {
  constexpr int TI = 63;  // ifft_tab_count(64) == fft_tab_count(64)
  __shared__ LdsSym<NV> lds[64][64];
  __shared__ uint4 tl[TI * 6];
  const uint64_t sb = a.shard_bytes;
  const uint64_t regions = sb / 64 * (8 / NV) / 64;
  if (blockIdx.x >= regions) return;  // whole block: every wave shares the region
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t off = dev::lane_byte_offset<NV>(blockIdx.x, lane, a.contig);
  auto stage = [&](const RsTab *src) {
    const uint4 *s4 = reinterpret_cast<const uint4 *>(src);
    for (uint32_t q = threadIdx.x; q < TI * 6; q += kBlock) tl[q] = s4[q];
  };
  const uint64_t s = blockIdx.y;
  const uint8_t *src = a.data + s * a.data_stripe_stride;
  Sym<NV> acc[16];
#pragma unroll
  for (int u = 0; u < 16; u++) dev::zero(acc[u]);
  for (uint32_t c = 0; c < a.n_chunks; c++) {
    const uint32_t t = c == 0 ? a.trunc_first : (c + 1 == a.n_chunks ? a.trunc_last : 64u);
    __syncthreads();  // previous chunk's readers of tl and lds are done
    stage(a.tabs + static_cast<uint64_t>(c) * TI);
    Sym<NV> cur[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {  // layout A
      const uint32_t pos = 16 * w + j;
      if (pos < t && !skipped(a, c * 64 + pos))
        dev::load_sym_raw(cur[j], src + (static_cast<uint64_t>(c) * 64 + pos) * sb, off, a.contig);
      else dev::zero(cur[j]);
    }
#pragma unroll
    for (int j = 0; j < 16; j++) dev::pair_halves(cur[j], a.contig);
    __syncthreads();  // tables staged
#pragma unroll
    for (int g = 0; g < 4; g++) {  // stage d=1, groups r = 16w + 4g
      const uint32_t r = 16 * w + 4 * g;
      if (r < t) ifft4l(cur[4 * g], cur[4 * g + 1], cur[4 * g + 2], cur[4 * g + 3], tl + (r / 4 * 3) * 6);
    }
    if (16 * w < t) {  // stage d=4, group r = 16w
#pragma unroll
      for (int i = 0; i < 4; i++) ifft4l(cur[i], cur[i + 4], cur[i + 8], cur[i + 12], tl + (48 + w * 3) * 6);
    }
#pragma unroll
    for (int j = 0; j < 16; j++) lds_put(lds[16 * w + j], lane, cur[j]);
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 16; u++) lds_get(lds[(u & 3) + 4 * w + 16 * (u >> 2)], lane, cur[u]);  // layout B
#pragma unroll
    for (int i = 0; i < 4; i++) ifft4l(cur[i], cur[i + 4], cur[i + 8], cur[i + 12], tl + 60 * 6);  // d=16
#pragma unroll
    for (int u = 0; u < 16; u++) dev::xor_into(acc[u], cur[u]);  // root.zig:153-155
  }
  // FFT(0, 64, trunc m) on acc, root.zig:169
  __syncthreads();
  stage(a.tabs + static_cast<uint64_t>(a.n_chunks) * TI);
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; i++) fft4l(acc[i], acc[i + 4], acc[i + 8], acc[i + 12], tl);  // d=16 (layout B)
#pragma unroll
  for (int u = 0; u < 16; u++) lds_put(lds[(u & 3) + 4 * w + 16 * (u >> 2)], lane, acc[u]);
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 16; j++) lds_get(lds[16 * w + j], lane, acc[j]);  // layout A
  if (16 * w < a.m) {  // d=4, group r = 16w
#pragma unroll
    for (int i = 0; i < 4; i++) fft4l(acc[i], acc[i + 4], acc[i + 8], acc[i + 12], tl + (3 + w * 3) * 6);
  }
#pragma unroll
  for (int g = 0; g < 4; g++) {  // d=1, groups r = 16w + 4g
    const uint32_t r = 16 * w + 4 * g;
    if (r < a.m) fft4l(acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3], tl + (15 + r / 4 * 3) * 6);
  }
  uint8_t *dst = a.parity + s * a.parity_stripe_stride;
#pragma unroll
  for (int j = 0; j < 16; j++) {
    const uint32_t pos = 16 * w + j;
    if (pos < a.m) dev::store_sym(dst + pos * sb, off, acc[j], a.contig);
  }
}

// ================================================= matrix reconstruct (e <= 8)
// restored_j = XOR_i M_ij(in_i): the reconstruct of root.zig:268-335 is
// GF(2)-linear in the received shards, so for one erasure pattern it is an
// n_out x n_in matrix of 16x16 GF(2) maps (host-derived, rs_plans.cpp). Each
// input is read once; its six bit-field selectors are shared by all n_out
// multiply-accumulates. Reads k shards, writes e: the algorithmic minimum.
template <int NV>
struct Sel {
  uint32_t a0[NV], a1[NV], a2[NV], b0[NV], b1[NV], b2[NV];
};

template <int NV>
__device__ __forceinline__ void make_sel(Sel<NV> &s, const Sym<NV> &y) {
#pragma unroll
  for (int v = 0; v < NV; v++) {
    s.a0[v] = y.l[v] & 0x07070707u;
    s.a1[v] = (y.l[v] >> 3) & 0x07070707u;
    s.a2[v] = (y.l[v] >> 6) & 0x03030303u;
    s.b0[v] = y.h[v] & 0x07070707u;
    s.b1[v] = (y.h[v] >> 3) & 0x07070707u;
    s.b2[v] = (y.h[v] >> 6) & 0x03030303u;
  }
}

template <int NV>
__device__ __forceinline__ void mac_sel(Sym<NV> &x, const Sel<NV> &s, const Tab &t) {
  using dev::perm;
  using dev::xor3;
#pragma unroll
  for (int v = 0; v < NV; v++) {
    uint32_t l = xor3(x.l[v], perm(t.lo[1], t.lo[0], s.a0[v]), perm(t.lo[3], t.lo[2], s.a1[v]));
    uint32_t h = xor3(x.h[v], perm(t.hi[1], t.hi[0], s.a0[v]), perm(t.hi[3], t.hi[2], s.a1[v]));
    l = xor3(l, perm(t.lo[4], t.lo[4], s.a2[v]), perm(t.lo[6], t.lo[5], s.b0[v]));
    h = xor3(h, perm(t.hi[4], t.hi[4], s.a2[v]), perm(t.hi[6], t.hi[5], s.b0[v]));
    x.l[v] = xor3(l, perm(t.lo[8], t.lo[7], s.b1[v]), perm(t.lo[9], t.lo[9], s.b2[v]));
    x.h[v] = xor3(h, perm(t.hi[8], t.hi[7], s.b1[v]), perm(t.hi[9], t.hi[9], s.b2[v]));
  }
}

// One received input of the matrix kernels: orig[idx] or rec[idx]; with
// kSrcXorScratch, rec[idx] ^ xs[idx] (a syndrome, reconstruct by syndromes).
// Split in two so a prefetched input keeps its loads in flight: issue_input only
// issues them, take_input waits, XORs the syndrome part and pairs the lane halves
// (the swap is a lane permutation, so it commutes with the XOR).
template <int NV>
struct InFlight {
  Sym<NV> y, z;
  bool x;
};

template <int NV>
__device__ __forceinline__ void issue_input(InFlight<NV> &f, int32_t src, const uint8_t *orig, const uint8_t *rec,
                                            const uint8_t *xs, uint64_t sb, uint32_t off, bool contig) {
  const uint64_t o = static_cast<uint64_t>(src & kSrcIndexMask) * sb;
  dev::load_sym_raw(f.y, ((src & kSrcRecovery) ? rec : orig) + o, off, contig);
  f.x = (src & kSrcXorScratch) != 0;
  if (f.x) dev::load_sym_raw(f.z, xs + o, off, contig);
}

template <int NV>
__device__ __forceinline__ void take_input(Sym<NV> &y, const InFlight<NV> &f, bool contig) {
  y = f.y;
  if (f.x) dev::xor_into(y, f.z);
  dev::pair_halves(y, contig);
}

template <int NV>
__device__ __forceinline__ void load_input(Sym<NV> &y, int32_t src, const uint8_t *orig, const uint8_t *rec,
                                           const uint8_t *xs, uint64_t sb, uint32_t off, bool contig) {
  InFlight<NV> f;
  issue_input(f, src, orig, rec, xs, sb, off, contig);
  take_input(y, f, contig);
}

template <int E, int NV, int D>
__global__ __launch_bounds__(kBlock) void k_decode_matrix(DecodeArgs a) {
  uint32_t off;
  if (!lane_offset<NV>(a.shard_bytes, a.contig, off)) return;
  const uint64_t sb = a.shard_bytes;
  typedef const __attribute__((address_space(4))) int32_t *CI;
  const uint32_t n_in = a.n_in;
  {  // one stripe per blockIdx.y (launches are split at 65535 stripes)
    const uint64_t s = blockIdx.y;
    const CI srcs = (CI)(a.pos_src + s * a.src_stride);
    const RsTab *mat = a.tab_mat + s * a.mat_stride;
    const uint32_t e_s = a.nout ? static_cast<uint32_t>(((CI)(a.nout))[s]) : static_cast<uint32_t>(E);
    const uint8_t *orig = a.orig + s * a.orig_stripe_stride;
    const uint8_t *rec = a.rec + s * a.rec_stripe_stride;
    const uint8_t *xs = a.xsrc + s * a.xsrc_stripe_stride;
    auto issue = [&](InFlight<NV> &f, uint32_t i) { issue_input(f, srcs[i], orig, rec, xs, sb, off, a.contig); };
    Sym<NV> acc[E];
#pragma unroll
    for (int j = 0; j < E; j++) dev::zero(acc[j]);
    if constexpr (D == 1) {
      // one input ahead: input i+1 in flight while input i is multiplied
      InFlight<NV> f;
      issue(f, 0);
      for (uint32_t i = 0; i < n_in; i++) {
        Sym<NV> y;
        take_input(y, f, a.contig);
        if (i + 1 < n_in) issue(f, i + 1);
        Sel<NV> sel;
        make_sel(sel, y);
        const RsTab *row = mat + static_cast<uint64_t>(i) * E;
#pragma unroll
        for (int j = 0; j < E; j++) mac_sel(acc[j], sel, dev::load_tab(row + j));
      }
    } else {
      // batches of D inputs: D loads in flight together, then D x E MACs
      for (uint32_t i0 = 0; i0 < n_in; i0 += D) {
        InFlight<NV> f[D];
#pragma unroll
        for (int d = 0; d < D; d++)
          if (i0 + d < n_in) issue(f[d], i0 + d);
#pragma unroll
        for (int d = 0; d < D; d++) {
          if (i0 + d >= n_in) break;
          Sym<NV> y;
          take_input(y, f[d], a.contig);
          Sel<NV> sel;
          make_sel(sel, y);
          const RsTab *row = mat + static_cast<uint64_t>(i0 + d) * E;
#pragma unroll
          for (int j = 0; j < E; j++) mac_sel(acc[j], sel, dev::load_tab(row + j));
        }
      }
    }
    uint8_t *out = a.out + s * a.out_stripe_stride;
#pragma unroll
    for (int j = 0; j < E; j++)
      if (static_cast<uint32_t>(j) < e_s) dev::store_sym(out + static_cast<uint64_t>(j) * sb, off, acc[j], a.contig);
  }
}

// ======================================= matrix reconstruct, output-tiled waves
// For 8 < e <= 64 (e.g. RS(200,55) losing all 55 data shards it can): a
// workgroup's 4 waves share the same 64 column units and split the e outputs,
// EW per wave ("per-wave output-shard tiling"); each wave streams all k inputs
// (the 4 waves read the same lines back to back: HBM once, L2 for the rest).
template <int NV>
__device__ __forceinline__ void mac_sel_v(Sym<NV> &x, const Sel<NV> &s, const uint32_t *lo, const uint32_t *hi) {
  using dev::perm;
  using dev::xor3;
#pragma unroll
  for (int v = 0; v < NV; v++) {
    uint32_t l = xor3(x.l[v], perm(lo[1], lo[0], s.a0[v]), perm(lo[3], lo[2], s.a1[v]));
    uint32_t h = xor3(x.h[v], perm(hi[1], hi[0], s.a0[v]), perm(hi[3], hi[2], s.a1[v]));
    l = xor3(l, perm(lo[4], lo[4], s.a2[v]), perm(lo[6], lo[5], s.b0[v]));
    h = xor3(h, perm(hi[4], hi[4], s.a2[v]), perm(hi[6], hi[5], s.b0[v]));
    x.l[v] = xor3(l, perm(lo[8], lo[7], s.b1[v]), perm(lo[9], lo[9], s.b2[v]));
    x.h[v] = xor3(h, perm(hi[8], hi[7], s.b1[v]), perm(hi[9], hi[9], s.b2[v]));
  }
}

// k_decode_mtile with the tables of each input row staged in LDS (double-buffered,
// one barrier per input) and read back as VGPRs by broadcast ds_read_b128; waves
// past n_out still stage and join the barriers, and padded outputs are skipped.
template <int EW, int NV>
__global__ __launch_bounds__(kBlock) void k_decode_mtile_lds(DecodeArgs a) {
  constexpr int kRow = 4 * EW;  // outputs per table row (4 waves)
  __shared__ uint4 tabs[2][kRow][5];  // lo[10] hi[10] of each RsTab
  const uint64_t sb = a.shard_bytes;
  if (blockIdx.x >= sb / 64 * (8 / NV) / 64) return;  // uniform over the block
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t j0 = w * EW;
  const uint32_t nj = j0 < a.n_out ? min(static_cast<uint32_t>(EW), a.n_out - j0) : 0u;
  const uint32_t off = dev::lane_byte_offset<NV>(blockIdx.x, lane, a.contig);
  const uint64_t s = blockIdx.y;
  typedef const __attribute__((address_space(4))) int32_t *CI;
  const CI srcs = (CI)(a.pos_src);
  const uint8_t *orig = a.orig + s * a.orig_stripe_stride;
  const uint8_t *rec = a.rec + s * a.rec_stripe_stride;
  const uint8_t *xs = a.xsrc + s * a.xsrc_stripe_stride;
  auto stage = [&](uint32_t i, int b) {
    const uint4 *src = reinterpret_cast<const uint4 *>(a.tab_mat + static_cast<uint64_t>(i) * kRow);
    for (uint32_t q = threadIdx.x; q < kRow * 5; q += kBlock) tabs[b][q / 5][q % 5] = src[q / 5 * 6 + q % 5];
  };
  Sym<NV> acc[EW];
#pragma unroll
  for (int j = 0; j < EW; j++) dev::zero(acc[j]);
  stage(0, 0);
  __syncthreads();
  InFlight<NV> f;
  if (nj) issue_input(f, srcs[0], orig, rec, xs, sb, off, a.contig);
  for (uint32_t i = 0; i < a.n_in; i++) {
    Sym<NV> y;
    if (nj) take_input(y, f, a.contig);
    if (i + 1 < a.n_in) {
      stage(i + 1, (i + 1) & 1);
      if (nj) issue_input(f, srcs[i + 1], orig, rec, xs, sb, off, a.contig);
    }
    if (nj) {
      Sel<NV> sel;
      make_sel(sel, y);
#pragma unroll
      for (int j = 0; j < EW; j++) {
        if (static_cast<uint32_t>(j) < nj) {  // uniform; keeps acc[] in registers (no dynamic index)
          const uint4 *t = tabs[i & 1][j0 + j];
          const uint4 q0 = t[0], q1 = t[1], q2 = t[2], q3 = t[3], q4 = t[4];
          const uint32_t lo[10] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y};
          const uint32_t hi[10] = {q2.z, q2.w, q3.x, q3.y, q3.z, q3.w, q4.x, q4.y, q4.z, q4.w};
          mac_sel_v(acc[j], sel, lo, hi);
        }
      }
    }
    __syncthreads();  // buffer (i & 1) free for input i + 2
  }
  uint8_t *out = a.out + s * a.out_stripe_stride;
#pragma unroll
  for (int j = 0; j < EW; j++)
    if (static_cast<uint32_t>(j) < nj) dev::store_sym(out + static_cast<uint64_t>(j0 + j) * sb, off, acc[j], a.contig);
}

// ============================================ generic: column walk in HBM scratch
template <int NV>
__device__ __forceinline__ void ld(Sym<NV> &s, const uint8_t *p) {
  typedef typename dev::VecT<NV>::type V;
  const V lo = *reinterpret_cast<const V *>(p), hi = *reinterpret_cast<const V *>(p + 32);
  if constexpr (NV == 1) {
    s.l[0] = lo;
    s.h[0] = hi;
  } else {
    for (int v = 0; v < NV; v++) {
      s.l[v] = lo[v];
      s.h[v] = hi[v];
    }
  }
}
template <int NV>
__device__ __forceinline__ void st(uint8_t *p, const Sym<NV> &s) {
  typedef typename dev::VecT<NV>::type V;
  V lo, hi;
  if constexpr (NV == 1) {
    lo = s.l[0];
    hi = s.h[0];
  } else {
    for (int v = 0; v < NV; v++) {
      lo[v] = s.l[v];
      hi[v] = s.h[v];
    }
  }
  *reinterpret_cast<V *>(p) = lo;
  *reinterpret_cast<V *>(p + 32) = hi;
}

// ---- the column transforms, phased (Generic.zig:15-147, runtime size / truncation).
// A layer-by-layer walk reads and writes the whole column once per layer (5 passes
// for 512 points). Here consecutive layers are grouped into phases whose butterflies
// close over n <= 64 positions pos0 + j*dlo (j < n): a phase loads such a set into
// VGPRs, runs its layers there (the j-space structure is exactly ifft_regs<n> /
// fft_regs<n>; twiddle groups and truncation use the real positions) and stores it
// back: 2 passes for 512 or 4,096 points. The first phase may read another buffer
// (positions >= n_src read as zero) and the last may write another (positions
// >= n_out dropped; out_sym: the shard layout of dev::store_sym), so a transform
// between buffers costs no copy pass.
struct XformIO {
  // buffers are wave-uniform bases; a lane adds `off` (global_load saddr + voffset form)
  const uint8_t *src;  // first phase input (positions >= n_src read as zero)
  uint64_t src_ps, n_src;
  uint8_t *work;       // intermediate phases (in place)
  uint64_t work_ps;
  uint8_t *out;        // last phase output (positions >= n_out not stored)
  uint64_t out_ps, n_out;
  bool out_sym, contig;  // out in the shard layout (dev::store_sym) instead of work's
  uint32_t off;          // the lane's byte offset in every buffer
};

template <int NV>
__device__ __forceinline__ void ldb(Sym<NV> &s, __amdgpu_buffer_rsrc_t r, uint32_t off) {
  static_assert(NV == 1, "generic column walk: one dword pair per lane");
  s.l[0] = __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0);
  s.h[0] = __builtin_amdgcn_raw_buffer_load_b32(r, off + 32u, 0, 0);
}
template <int NV>
__device__ __forceinline__ void stb(__amdgpu_buffer_rsrc_t r, uint32_t off, const Sym<NV> &s) {
  __builtin_amdgcn_raw_buffer_store_b32(s.l[0], r, off, 0, 0);
  __builtin_amdgcn_raw_buffer_store_b32(s.h[0], r, off + 32u, 0, 0);
}

template <int N, int NV, bool INV>
__device__ __forceinline__ void xform_phase(const XformIO &io, bool first, bool last, const RsTab *__restrict__ tabs,
                                         uint64_t ti, uint64_t size, uint64_t rmax, uint32_t dlo_log) {
  const uint8_t *src = first ? io.src : io.work;
  const uint64_t sps = first ? io.src_ps : io.work_ps, n_src = first ? io.n_src : size;
  uint8_t *dst = last ? io.out : io.work;
  const uint64_t dps = last ? io.out_ps : io.work_ps, n_dst = last ? io.n_out : size;
  const bool sym = last && io.out_sym;
  const uint64_t dlo = 1ull << dlo_log, span = static_cast<uint64_t>(N) << dlo_log;
  for (uint64_t blk = 0; blk < size; blk += span) {
    if (!INV && blk >= n_dst) break;  // FFT: a block past the stored outputs feeds nothing later
    for (uint64_t lo = 0; lo < dlo; lo++) {
      // opaque per sub-problem: the N row offsets (j << dlo_log) * ps and the group tables are
      // computed where used instead of hoisted out of the walk and spilled (see opq)
      const uint32_t dl = opqu(dlo_log);
      const RsTab *tb = opq(tabs);
      Sym<NV> s[N];
#pragma unroll
      for (int j = 0; j < N; j++) {
        const uint64_t p = blk + lo + (static_cast<uint64_t>(j) << dl);
        if (p < n_src) ldb(s[j], row_rsrc(src + p * sps), io.off);
        else dev::zero(s[j]);
      }
      if constexpr (INV) ifft_sub<N, NV>(s, tb, ti, size, rmax, blk, dl);
      else fft_sub<N, NV>(s, tb, ti, size, rmax, blk, dl);
#pragma unroll
      for (int j = 0; j < N; j++) {
        const uint64_t p = blk + lo + (static_cast<uint64_t>(j) << dl);
        if (p < n_dst) {
          if (sym) dev::store_sym(dst + p * dps, io.off, s[j], io.contig);
          else stb(row_rsrc(dst + p * dps), io.off, s[j]);
        }
      }
    }
  }
}

// the whole transform of `size` points (a power of two) with truncation `trunc`
template <int NV, bool INV>
__device__ __forceinline__ void xform_ph(const XformIO &io, uint64_t size, uint64_t trunc, const RsTab *__restrict__ tabs) {
  const uint32_t lg = log2_u64(size), n4 = lg / 2;
  const bool r2 = lg & 1;
  const uint64_t rmax = trunc < size ? trunc : size;
  uint64_t ti = 0;
  uint32_t layer = 0;  // radix-4 layers done (IFFT: from distance 1 up; FFT: from size/4 down)
  bool r2_done = !r2, first = true;
  do {
    const uint32_t c = n4 - layer < 3 ? n4 - layer : 3;
    const bool with_r2 = !r2_done && layer + c == n4 && c < 3;
    const uint32_t n = (1u << (2 * c)) << (with_r2 ? 1 : 0);
    const bool last = layer + c == n4 && (r2_done || with_r2);
    // lowest distance of the phase (its position stride)
    const uint32_t dlo_log = INV ? 2 * layer : (with_r2 || c == 0 ? 0 : lg - 2 * (layer + c));
#define RS_XF_CASE(N_) \
  case N_: xform_phase<N_, NV, INV>(io, first, last, tabs, ti, size, rmax, dlo_log); break;
    switch (n) {
      RS_XF_CASE(1) RS_XF_CASE(2) RS_XF_CASE(4) RS_XF_CASE(8) RS_XF_CASE(16) RS_XF_CASE(32) RS_XF_CASE(64)
    }
#undef RS_XF_CASE
    for (uint32_t l = layer; l < layer + c; l++) ti += INV ? 3 * (size >> (2 * l + 2)) : 3ull << (2 * l);
    layer += c;
    r2_done = r2_done || with_r2;
    first = false;
    if (c == 0) r2_done = true;  // the lone radix-2 phase (n == 2) just ran
  } while (layer < n4 || !r2_done);
}

// in place on positions w + p*ps + off (the former layer-by-layer ifft_mem / fft_mem)
template <int NV>
__device__ __forceinline__ void ifft_mem(uint8_t *w, uint32_t off, uint64_t ps, uint64_t size, uint64_t trunc,
                         const RsTab *__restrict__ tabs) {
  const XformIO io{w, ps, size, w, ps, w, ps, size, false, false, off};
  xform_ph<NV, true>(io, size, trunc, tabs);
}
template <int NV>
__device__ __forceinline__ void fft_mem(uint8_t *w, uint32_t off, uint64_t ps, uint64_t size, uint64_t trunc,
                        const RsTab *__restrict__ tabs) {
  const XformIO io{w, ps, size, w, ps, w, ps, size, false, false, off};
  xform_ph<NV, false>(io, size, trunc, tabs);
}

template <int NV>
__device__ __forceinline__ void xor_mem(uint8_t *a, const uint8_t *b) {
  Sym<NV> x, y;
  ld(x, a);
  ld(y, b);
  dev::xor_into(x, y);
  st(a, x);
}

template <int NV>
__global__ __launch_bounds__(kBlock) void k_encode_generic(EncodeArgs a) {
  uint32_t off;
  if (!lane_offset<NV>(a.shard_bytes, a.contig, off)) return;
  const uint64_t sb = a.shard_bytes, C = a.chunk;
  for (uint64_t s = blockIdx.y; s < a.n_stripes; s += gridDim.y) {
    const uint8_t *src = a.data + s * a.data_stripe_stride + off;
    uint8_t *work = a.scratch + s * a.work * sb + off;
    for (uint32_t j = 0; j < a.n_chunks; j++) {
      const uint64_t t = j == 0 ? a.trunc_first : (j + 1 == a.n_chunks ? a.trunc_last : C);
      for (uint64_t p = 0; p < C; p++) {
        Sym<NV> v;
        if (p < t && !skipped(a, static_cast<uint32_t>(j * C + p))) ld(v, src + (j * C + p) * sb);
        else dev::zero(v);
        st(work + (j * C + p) * sb, v);
      }
      ifft_mem<NV>(work - off + j * C * sb, off, sb, C, t, a.tabs + static_cast<uint64_t>(j) * a.tabs_per_chunk);
      if (j > 0)
        for (uint64_t p = 0; p < C; p++) xor_mem<NV>(work + p * sb, work + (j * C + p) * sb);
    }
    fft_mem<NV>(work - off, off, sb, C, a.m, a.tabs + static_cast<uint64_t>(a.n_chunks) * a.tabs_per_chunk);
    uint8_t *dst = a.parity + s * a.parity_stripe_stride + off;
    for (uint64_t p = 0; p < a.m; p++) {
      Sym<NV> v;
      ld(v, work + p * sb);
      dev::store_sym(dst + p * sb, 0u, v, a.contig);
    }
  }
}

// ======================================================= low-rate encode (§8 f4)
// The reference panics on low rate (root.zig:119-121); this is the encode of the
// algorithm it ports (rs_gf.hpp scalar_encode_low, parity unpinned): the k originals are
// positions [0, k) of one chunk C = ceilPow2(k), coefficients = IFFT(C, trunc k, skew 0),
// and recovery chunk j = FFT(coefficients, trunc min(C, m - jC), skew (j+1)C).
// Register kernel: the coefficients stay in VGPRs across the recovery chunks (each
// chunk's FFT runs on a copy), so a stripe's originals are read once and every
// recovery shard written once; twiddle tables are wave-uniform (SGPRs).
template <int C, int NV>
__global__ __launch_bounds__(kBlock) void k_encode_low_reg(EncodeArgs a) {
  uint32_t off;
  if (!lane_offset<NV>(a.shard_bytes, a.contig, off)) return;
  constexpr int TI = ifft_tabs_ce(C);
  const uint64_t sb = a.shard_bytes;
  const uint64_t s = blockIdx.y;  // launches are split at 65535 stripes
  const uint8_t *src = a.data + s * a.data_stripe_stride;
  Sym<NV> coef[C];
#pragma unroll
  for (int p = 0; p < C; p++) {
    if (static_cast<uint32_t>(p) < a.k) dev::load_sym_raw(coef[p], src + p * sb, off, a.contig);
    else dev::zero(coef[p]);
  }
#pragma unroll
  for (int p = 0; p < C; p++) dev::pair_halves(coef[p], a.contig);
  dev::ifft_regs<C>(coef, a.tabs, a.k);
  uint8_t *dst = a.parity + s * a.parity_stripe_stride;
  for (uint32_t j = 0; j < a.n_chunks; j++) {
    const uint32_t t = a.m - j * C < static_cast<uint32_t>(C) ? a.m - j * C : static_cast<uint32_t>(C);
    Sym<NV> cur[C];
#pragma unroll
    for (int p = 0; p < C; p++) cur[p] = coef[p];
    const RsTab *tj = a.tabs + TI + static_cast<uint64_t>(j) * a.tabs_per_chunk;
    asm volatile("" : "+s"(tj));  // opaque base: no per-group pointer IVs
    dev::fft_regs<C>(cur, tj, t);
    uint8_t *dj = dst + static_cast<uint64_t>(j) * C * sb;
#pragma unroll
    for (int p = 0; p < C; p++)
      if (static_cast<uint32_t>(p) < t) dev::store_sym(dj + p * sb, off, cur[p], a.contig);
  }
}

// Any C: each lane walks its column through a scratch [stripe][(1 + n_chunks) C][sb]
// (coefficients at [0, C), recovery chunk j's intermediate phases at [(1 + j) C, (2 + j) C)).
__device__ __forceinline__ uint64_t ifft_tab_count_d(uint64_t size) {
  uint64_t n = 0, d = 1, d4 = 4;
  for (; d4 <= size; d = d4, d4 <<= 2) n += 3 * (size / d4);
  return n + (d < size ? 1 : 0);
}

// Stage 1 (blockIdx.z == 0 of k_encode_low_coef): coefficients = the originals -> IFFT ->
// work[0, C) (no staging copy). Stage 2 (k_encode_low_generic, blockIdx.z = recovery chunk
// j): coefficients -> FFT (intermediate phases in work[(1 + j) C, (2 + j) C)) -> parity
// rows; the chunks run side by side (a lane's column walk is serial, so the grid's
// chunk dimension is the parallelism left at small batches).
template <int NV>
__global__ __launch_bounds__(kBlock) void k_encode_low_coef(EncodeArgs a) {
  uint32_t off;
  if (!lane_offset<NV>(a.shard_bytes, a.contig, off)) return;
  const uint64_t sb = a.shard_bytes, C = a.chunk, R = a.regions ? a.regions : 1 + a.n_chunks;
  for (uint64_t s = blockIdx.y; s < a.n_stripes; s += gridDim.y) {
    uint8_t *work = a.scratch + s * R * C * sb;
    const XformIO ic{a.data + s * a.data_stripe_stride, sb, a.k, work, sb, work, sb, C, false, false, off};
    xform_ph<NV, true>(ic, C, a.k, a.tabs);
  }
}

template <int NV>
__global__ __launch_bounds__(kBlock) void k_encode_low_generic(EncodeArgs a) {
  uint32_t off;
  if (!lane_offset<NV>(a.shard_bytes, a.contig, off)) return;
  const uint64_t sb = a.shard_bytes, C = a.chunk, TI = ifft_tab_count_d(C), j = a.chunk0 + blockIdx.z;
  const uint64_t R = a.regions ? a.regions : 1 + a.n_chunks;
  const uint64_t t = a.m - j * C < C ? a.m - j * C : C;
  for (uint64_t s = blockIdx.y; s < a.n_stripes; s += gridDim.y) {
    uint8_t *work = a.scratch + s * R * C * sb;
    uint8_t *dst = a.parity + s * a.parity_stripe_stride;
    const XformIO fc{work, sb, C, work + (1 + blockIdx.z) * C * sb, sb, dst + j * C * sb, sb, t, true, a.contig, off};
    xform_ph<NV, false>(fc, C, t, a.tabs + TI + j * a.tabs_per_chunk);
  }
}

// ======================================================= shard tails (sb % 64)
// The reference panics on tails (root.zig:385); its undoLastChunkEncoding
// (root.zig:338-348) implies the layout: a tail of t bytes is coded as one more
// chunk with bytes [0,t/2) as lo bytes [0,t/2) and [t/2,t) as hi bytes
// [32,32+t/2). Pack/unpack one shard's tail chunk for n stripes (one thread per
// byte of the 64-B chunk); whole chunks are moved with hipMemcpy2DAsync.
__global__ __launch_bounds__(256) void k_tail_pack(const uint8_t *__restrict__ src, uint64_t src_stripe_stride,
                                                   uint8_t *__restrict__ dst, uint64_t dst_stripe_stride,
                                                   uint64_t sb, uint64_t n, int unpack) {
  const uint64_t g = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (g >= n * 64) return;
  const uint64_t s = g / 64;
  const uint32_t j = static_cast<uint32_t>(g % 64);
  const uint32_t t = static_cast<uint32_t>(sb % 64), h = t / 2;
  const uint64_t whole = sb - t;
  if (!unpack) {  // real shard (sb bytes) -> padded tail chunk
    const uint8_t *in = src + s * src_stripe_stride + whole;
    uint8_t v = 0;
    if (j < h) v = in[j];
    else if (j >= 32 && j < 32 + h) v = in[h + j - 32];
    dst[s * dst_stripe_stride + whole + j] = v;
  } else if (j < t) {  // padded tail chunk -> real shard
    const uint8_t *in = src + s * src_stripe_stride + whole;
    dst[s * dst_stripe_stride + whole + j] = j < h ? in[j] : in[32 + j - h];
  }
}

// ================================================================== verify
// The compare of rs_verify_batch_dev: a = the encode of a slice's originals ([n][m][sb]),
// b = the stored recovery shards. A workgroup takes kVerifySeg bytes of one shard (work items
// flattened over stripe, shard, segment; grid-stride, 64-bit indices), ORs the XOR of the two
// and, where a wave saw a difference, its lane 0 stores 1 to the shard's flag (zeroed by the
// host; several waves may store the same 1). MODE 2: 16-byte loads, 1: dwords, 0: bytes
// (tails make shard starts 2-byte aligned).
constexpr uint32_t kVerifySeg = 16384;  // a multiple of 16: segment starts keep the shard's alignment

template <int MODE>
__global__ __launch_bounds__(256) void k_verify_compare(const uint8_t *__restrict__ a, uint64_t a_stride,
                                                        const uint8_t *__restrict__ b, uint64_t b_stride,
                                                        uint64_t sb, uint64_t n, uint32_t m, uint64_t segs,
                                                        uint8_t *__restrict__ bad, uint64_t bad_stride) {
  const uint64_t per_stripe = static_cast<uint64_t>(m) * segs, total = n * per_stripe;
  for (uint64_t w = blockIdx.x; w < total; w += gridDim.x) {
    const uint64_t s = w / per_stripe, rem = w % per_stripe;
    const uint64_t r = rem / segs, base = (rem % segs) * kVerifySeg;
    const uint32_t len = static_cast<uint32_t>(sb - base < kVerifySeg ? sb - base : kVerifySeg);
    const uint8_t *pa = a + s * a_stride + r * sb + base;
    const uint8_t *pb = b + s * b_stride + r * sb + base;
    uint32_t d = 0;
    if (MODE == 2) {
      typedef uint32_t v4u __attribute__((ext_vector_type(4)));
      for (uint32_t i = threadIdx.x * 16u; i + 16u <= len; i += 256u * 16u) {
        const v4u x = __builtin_nontemporal_load(reinterpret_cast<const v4u *>(pa + i));
        const v4u y = __builtin_nontemporal_load(reinterpret_cast<const v4u *>(pb + i));
        d |= (x[0] ^ y[0]) | (x[1] ^ y[1]) | (x[2] ^ y[2]) | (x[3] ^ y[3]);
      }
    } else if (MODE == 1) {
      for (uint32_t i = threadIdx.x * 4u; i + 4u <= len; i += 256u * 4u)
        d |= *reinterpret_cast<const uint32_t *>(pa + i) ^ *reinterpret_cast<const uint32_t *>(pb + i);
    } else {
      for (uint32_t i = threadIdx.x; i < len; i += 256u) d |= static_cast<uint32_t>(pa[i] ^ pb[i]);
    }
    if (__builtin_amdgcn_ballot_w64(d != 0u) != 0ull && (threadIdx.x & 63u) == 0u) bad[s * bad_stride + r] = 1;
  }
}

// The number of nonzero flags among [n][m]: per-workgroup partial sums added to *count
// (zeroed by the host on the stream).
__global__ __launch_bounds__(256) void k_verify_count(const uint8_t *__restrict__ bad, uint64_t bad_stride, uint64_t n,
                                                      uint32_t m, unsigned long long *count) {
  __shared__ uint32_t part;
  if (threadIdx.x == 0) part = 0;
  __syncthreads();
  const uint64_t total = n * m;
  uint32_t c = 0;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; i < total;
       i += static_cast<uint64_t>(gridDim.x) * 256u)
    c += bad[i / m * bad_stride + i % m] != 0;
  if (c) atomicAdd(&part, c);
  __syncthreads();
  if (threadIdx.x == 0 && part) atomicAdd(count, static_cast<unsigned long long>(part));
}

// ========================================================== engine test shims
__global__ __launch_bounds__(kBlock) void k_engine_transform(uint8_t *work, uint64_t sb, uint64_t pos, uint64_t size,
                                                             uint64_t trunc, const RsTab *tabs, int inverse) {
  uint32_t off;
  if (!lane_offset<1>(sb, false, off)) return;
  if (inverse) ifft_mem<1>(work + pos * sb, off, sb, size, trunc, tabs);
  else fft_mem<1>(work + pos * sb, off, sb, size, trunc, tabs);
}

__global__ __launch_bounds__(kBlock) void k_mul_scalar(uint8_t *chunks, uint64_t bytes, const RsTab *tab) {
  uint32_t off;
  if (!lane_offset<1>(bytes, false, off)) return;
  Sym<1> v;
  ld(v, chunks + off);
  dev::mul_inplace(v, dev::load_tab(tab));
  st(chunks + off, v);
}

}  // namespace

// ---------------------------------------------------------------- selection
// Instantiated register variants (see launch_*): encode keeps acc + one chunk
// (2*C slots) live with 2*C*2*NV <= 64 VGPRs of state; decode keeps W slots,
// W*2*NV <= 128.
static int clamp_nv(int nv, int size, bool enc) {
  const int live = enc ? 2 * size : size;  // symbol slots live at once
  const int limit = enc ? 64 : 128;
  while (nv > 1 && live * 2 * nv > limit) nv >>= 1;
  return nv;
}

// A wave of the register / matrix kernels covers 512 * NV bytes of a shard: when
// that leaves more than 1/8 of the lanes idle (small shards), halve NV.
// RS(32,32) 1 KiB x 65536, 4 erased: decode_matrix_e4 nv4 1.43 -> nv1 0.97 ms.
static int fit_nv(int nv, uint64_t shard_bytes) {
  while (nv > 1) {
    const uint64_t w = 512ull * nv, idle = (shard_bytes + w - 1) / w * w - shard_bytes;
    if (idle * 8 <= shard_bytes) break;
    nv >>= 1;
  }
  return nv;
}

static int env_nv(int dflt) {
  const int v = rs::env::num(rs::env::NV);
  return (v == 1 || v == 2 || v == 4) ? v : dflt;
}

static const char *reg_name(bool enc, int size, int nv) {
  static const char *kEnc[6][3] = {
      {"encode_reg_w1_nv1", "encode_reg_w1_nv2", "encode_reg_w1_nv4"},
      {"encode_reg_w2_nv1", "encode_reg_w2_nv2", "encode_reg_w2_nv4"},
      {"encode_reg_w4_nv1", "encode_reg_w4_nv2", "encode_reg_w4_nv4"},
      {"encode_reg_w8_nv1", "encode_reg_w8_nv2", "encode_reg_w8_nv4"},
      {"encode_reg_w16_nv1", "encode_reg_w16_nv2", "encode_reg_w16_nv4"},
      {"encode_reg_w32_nv1", "encode_reg_w32_nv2", "encode_reg_w32_nv4"}};
  static const char *kDec[6][3] = {
      {"decode_reg_w1_nv1", "decode_reg_w1_nv2", "decode_reg_w1_nv4"},
      {"decode_reg_w2_nv1", "decode_reg_w2_nv2", "decode_reg_w2_nv4"},
      {"decode_reg_w4_nv1", "decode_reg_w4_nv2", "decode_reg_w4_nv4"},
      {"decode_reg_w8_nv1", "decode_reg_w8_nv2", "decode_reg_w8_nv4"},
      {"decode_reg_w16_nv1", "decode_reg_w16_nv2", "decode_reg_w16_nv4"},
      {"decode_reg_w32_nv1", "decode_reg_w32_nv2", "decode_reg_w32_nv4"}};
  int si = 0;
  while ((1 << si) < size) si++;
  const int ni = nv == 1 ? 0 : nv == 2 ? 1 : 2;
  return enc ? kEnc[si][ni] : kDec[si][ni];
}

KernelChoice choose_encode(uint64_t k, uint64_t m, uint64_t shard_bytes, int max_nv) {
  (void)k;
  const uint64_t C = ceil_pow2(m);
  if (C <= 32) {  // C = 32: 64 live slots of one dword pair (NV = 1)
    const int c = static_cast<int>(C);
    const int nv = clamp_nv(fit_nv(std::min(env_nv(4), max_nv), shard_bytes), c, true);
    return {Variant::kRegister, c, nv, reg_name(true, c, nv)};
  }
  if (C == 64 && shard_bytes % 512 == 0) {
    int nv = std::min(std::min(env_nv(1), max_nv), 2);
    if (shard_bytes % (512 * nv)) nv = 1;  // whole 64-lane regions only
    return {Variant::kWaveSplit, 64, nv, nv == 1 ? "encode_ws64_nv1" : "encode_ws64_nv2"};
  }
  return {Variant::kGeneric, static_cast<int>(C), 1, "encode_generic_nv1"};
}

KernelChoice choose_decode(uint64_t k, uint64_t m, uint64_t shard_bytes, int max_nv) {
  return choose_decode_w(ceil_pow2(ceil_pow2(m) + k), shard_bytes, max_nv);
}

KernelChoice choose_decode_w(uint64_t W, uint64_t shard_bytes, int max_nv) {
  if (W <= 32) {
    const int w = static_cast<int>(W);
    const int nv = clamp_nv(fit_nv(std::min(env_nv(4), max_nv), shard_bytes), w, false);
    return {Variant::kRegister, w, nv, reg_name(false, w, nv)};
  }
  return {Variant::kGeneric, static_cast<int>(W), 1, "decode_generic_nv1"};
}

KernelChoice choose_encode_low(uint64_t C, uint64_t shard_bytes, int max_nv) {
  static const char *kNames[6][3] = {
      {"encode_low_reg_w1_nv1", "encode_low_reg_w1_nv2", "encode_low_reg_w1_nv4"},
      {"encode_low_reg_w2_nv1", "encode_low_reg_w2_nv2", "encode_low_reg_w2_nv4"},
      {"encode_low_reg_w4_nv1", "encode_low_reg_w4_nv2", "encode_low_reg_w4_nv4"},
      {"encode_low_reg_w8_nv1", "encode_low_reg_w8_nv2", "encode_low_reg_w8_nv4"},
      {"encode_low_reg_w16_nv1", "encode_low_reg_w16_nv2", "encode_low_reg_w16_nv4"},
      {"encode_low_reg_w32_nv1", "encode_low_reg_w32_nv2", "encode_low_reg_w32_nv4"}};
  if (C <= 32) {  // coefficients + one recovery chunk live: the encode register budget
    const int c = static_cast<int>(C);
    const int nv = clamp_nv(fit_nv(std::min(env_nv(4), max_nv), shard_bytes), c, true);
    int si = 0;
    while ((1 << si) < c) si++;
    return {Variant::kRegister, c, nv, kNames[si][nv == 1 ? 0 : nv == 2 ? 1 : 2]};
  }
  return {Variant::kGeneric, static_cast<int>(C), 1, "encode_low_generic_nv1"};
}

#define RS_ENC_LOW_CASE(C_, NV_)                                                  \
  if (kc.size == C_ && kc.nv == NV_) {                                            \
    hipLaunchKernelGGL((k_encode_low_reg<C_, NV_>), grid, dim3(kBlock), 0, s, b); \
    e = hipGetLastError();                                                        \
    if (e != hipSuccess) return e;                                                \
    continue;                                                                     \
  }

hipError_t launch_encode_low(const KernelChoice &kc, const EncodeArgs &a, hipStream_t s) {
  trace_launch(kc.name);
  // phase launches for every generic low-rate encode since the phase kernels stopped spilling
  // (round 5: RS(300,1000) 1 MiB x 16 33.1 -> 23.4 ms, 64 KiB x 8 1.25 -> 0.76 ms, RS(1000,4000)
  // 4 KiB x 64 2.74 -> 1.47 ms; profiles/r05/lowrate/encph.log). Round 4 kept the per-lane column
  // walk where it had enough waves (then 32.7 vs 41.7 ms at 1 MiB x 16); it stays for chunk < 64.
  if (kc.variant == Variant::kGeneric && a.chunk >= 64) return launch_encode_low_phases(a, s);
  if (kc.variant == Variant::kGeneric) {
    // a.scratch: `regions` C-position regions per stripe (low_encode): the coefficients, then
    // one per recovery chunk of a launch; the chunks run in groups of regions - 1
    const dim3 g = grid_for(a.shard_bytes, 1, a.n_stripes);
    hipLaunchKernelGGL(k_encode_low_coef<1>, g, dim3(kBlock), 0, s, a);
    if (hipError_t e = hipGetLastError()) return e;
    const uint32_t G = a.regions ? a.regions - 1 : a.n_chunks;
    if (G == 0 || G > 65535) return hipErrorInvalidValue;
    for (uint32_t j0 = 0; j0 < a.n_chunks; j0 += G) {
      EncodeArgs b = a;
      b.chunk0 = j0;
      hipLaunchKernelGGL(k_encode_low_generic<1>, dim3(g.x, g.y, std::min(G, a.n_chunks - j0)), dim3(kBlock), 0, s, b);
      if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
  }
  for (uint64_t s0 = 0; s0 < a.n_stripes; s0 += 65535) {
    EncodeArgs b = a;
    b.data += s0 * a.data_stripe_stride;
    b.parity += s0 * a.parity_stripe_stride;
    b.n_stripes = std::min<uint64_t>(65535, a.n_stripes - s0);
    const dim3 grid = grid_for(b.shard_bytes, kc.nv, b.n_stripes);
    hipError_t e = hipSuccess;
    RS_ENC_LOW_CASE(1, 1) RS_ENC_LOW_CASE(1, 2) RS_ENC_LOW_CASE(1, 4)
    RS_ENC_LOW_CASE(2, 1) RS_ENC_LOW_CASE(2, 2) RS_ENC_LOW_CASE(2, 4)
    RS_ENC_LOW_CASE(4, 1) RS_ENC_LOW_CASE(4, 2) RS_ENC_LOW_CASE(4, 4)
    RS_ENC_LOW_CASE(8, 1) RS_ENC_LOW_CASE(8, 2)
    RS_ENC_LOW_CASE(16, 1)
    RS_ENC_LOW_CASE(32, 1)
    return hipErrorInvalidValue;
  }
  return hipSuccess;
}
#undef RS_ENC_LOW_CASE

KernelChoice choose_decode_matrix(uint32_t n_out, uint64_t shard_bytes, int max_nv) {
  static const char *kNames[9][3] = {
      {"", "", ""},
      {"decode_matrix_e1_nv1", "decode_matrix_e1_nv2", "decode_matrix_e1_nv4"},
      {"decode_matrix_e2_nv1", "decode_matrix_e2_nv2", "decode_matrix_e2_nv4"},
      {"decode_matrix_e3_nv1", "decode_matrix_e3_nv2", "decode_matrix_e3_nv4"},
      {"decode_matrix_e4_nv1", "decode_matrix_e4_nv2", "decode_matrix_e4_nv4"},
      {"decode_matrix_e5_nv1", "decode_matrix_e5_nv2", "decode_matrix_e5_nv4"},
      {"decode_matrix_e6_nv1", "decode_matrix_e6_nv2", "decode_matrix_e6_nv4"},
      {"decode_matrix_e7_nv1", "decode_matrix_e7_nv2", "decode_matrix_e7_nv4"},
      {"decode_matrix_e8_nv1", "decode_matrix_e8_nv2", "decode_matrix_e8_nv4"}};
  const int nv = fit_nv(std::min(env_nv(4), max_nv), shard_bytes);
  const int ni = nv == 1 ? 0 : nv == 2 ? 1 : 2;
  KernelChoice kc{Variant::kMatrix, static_cast<int>(n_out), nv, kNames[n_out][ni]};
  kc.prefetch = 1;  // inputs in flight per lane (2 measured no faster)
  return kc;
}

KernelChoice choose_decode_mtile(uint32_t n_out, uint64_t shard_bytes, int max_nv) {
  (void)n_out;
  int nv = std::min(std::min(env_nv(1), max_nv), 2);
  if (shard_bytes % (512ull * nv)) nv = 1;
  return {Variant::kMatrixTiled, kMtileEW, nv, nv == 1 ? "decode_mtile16_nv1" : "decode_mtile16_nv2"};
}

#define RS_MAT_CASE(E_, NV_)                                                                  \
  if (kc.size == E_ && kc.nv == NV_) {                                                        \
    switch (kc.prefetch) {                                                                    \
      case 2: hipLaunchKernelGGL((k_decode_matrix<E_, NV_, 2>), grid, dim3(kBlock), 0, s, a); break; \
      default: hipLaunchKernelGGL((k_decode_matrix<E_, NV_, 1>), grid, dim3(kBlock), 0, s, a); break; \
    }                                                                                         \
    return hipGetLastError();                                                                 \
  }
#define RS_MAT_NV(E_) RS_MAT_CASE(E_, 1) RS_MAT_CASE(E_, 2) RS_MAT_CASE(E_, 4)

#define RS_ENC_CASE(C_, NV_)                                                  \
  if (kc.size == C_ && kc.nv == NV_) {                                        \
    hipLaunchKernelGGL((k_encode_reg<C_, NV_>), grid, dim3(kBlock), 0, s, a); \
    return hipGetLastError();                                                 \
  }
#define RS_DEC_CASE(W_, NV_)                                                  \
  if (kc.size == W_ && kc.nv == NV_) {                                        \
    hipLaunchKernelGGL((k_decode_reg<W_, NV_>), grid, dim3(kBlock), 0, s, a); \
    return hipGetLastError();                                                 \
  }

static hipError_t launch_encode_one(const KernelChoice &kc, const EncodeArgs &a, hipStream_t s);
static hipError_t launch_decode_one(const KernelChoice &kc, const DecodeArgs &a, hipStream_t s);

// The fused kernels map one stripe to one blockIdx.y (no stripe loop inside the
// kernel: a loop lets the compiler hoist every per-stripe-invariant uniform value
// into SGPRs and spill them), so batches are launched in slices of <= 65535 stripes.
hipError_t launch_encode(const KernelChoice &kc, const EncodeArgs &a, hipStream_t s) {
  trace_launch(kc.name);
  if (kc.variant == Variant::kGeneric) return launch_encode_one(kc, a, s);
  for (uint64_t s0 = 0; s0 < a.n_stripes; s0 += 65535) {
    EncodeArgs b = a;
    b.data += s0 * a.data_stripe_stride;
    b.parity += s0 * a.parity_stripe_stride;
    b.n_stripes = std::min<uint64_t>(65535, a.n_stripes - s0);
    hipError_t e = launch_encode_one(kc, b, s);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_decode(const KernelChoice &kc, const DecodeArgs &a, hipStream_t s) {
  trace_launch(kc.name);
  if (kc.variant == Variant::kGeneric) return launch_decode_one(kc, a, s);
  for (uint64_t s0 = 0; s0 < a.n_stripes; s0 += 65535) {
    DecodeArgs b = a;
    b.orig += s0 * a.orig_stripe_stride;
    b.rec += s0 * a.rec_stripe_stride;
    b.out += s0 * a.out_stripe_stride;
    if (b.xsrc) b.xsrc += s0 * a.xsrc_stripe_stride;
    b.tab_mat += s0 * a.mat_stride;
    b.pos_src += s0 * a.src_stride;
    if (b.nout) b.nout += s0;
    b.tab_pre += s0 * a.pattern_stride;
    b.tab_post += s0 * a.pattern_stride;
    b.pos_src += s0 * a.pattern_stride;
    b.pos_dst += s0 * a.pattern_stride;
    b.n_stripes = std::min<uint64_t>(65535, a.n_stripes - s0);
    hipError_t e = launch_decode_one(kc, b, s);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

static hipError_t launch_encode_one(const KernelChoice &kc, const EncodeArgs &a, hipStream_t s) {
  const dim3 grid = grid_for(a.shard_bytes, kc.nv, a.n_stripes);
  if (kc.variant == Variant::kRegister) {
    // live slots 2*C: NV <= 128 / (4*C)
    RS_ENC_CASE(1, 1) RS_ENC_CASE(1, 2) RS_ENC_CASE(1, 4)
    RS_ENC_CASE(2, 1) RS_ENC_CASE(2, 2) RS_ENC_CASE(2, 4)
    RS_ENC_CASE(4, 1) RS_ENC_CASE(4, 2) RS_ENC_CASE(4, 4)
    RS_ENC_CASE(8, 1) RS_ENC_CASE(8, 2)
    RS_ENC_CASE(16, 1)
    RS_ENC_CASE(32, 1)
    return hipErrorInvalidValue;
  }
  if (kc.variant == Variant::kWaveSplit) {
    // one block per 64-lane region; 4 waves split the 64 positions
    const uint64_t regions = a.shard_bytes / 64 * (8 / kc.nv) / 64;
    const dim3 g(static_cast<uint32_t>(regions), grid.y, 1);
    // LDS-staged VGPR tables (no SGPR->VGPR moves, no SGPR spills): RS(200,55) 256 KiB x 256
    // NV=1 7.36 vs 7.62 ms, NV=2 9.34 vs 11.5 ms against SGPR tables
    // (profiles/r01/sweep_rs200_55_ws64_lds.jsonl)
    if (kc.nv == 1) hipLaunchKernelGGL((k_encode_ws64l<1>), g, dim3(kBlock), 0, s, a);
    else hipLaunchKernelGGL((k_encode_ws64l<2>), g, dim3(kBlock), 0, s, a);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(k_encode_generic<1>, grid, dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

static hipError_t launch_decode_one(const KernelChoice &kc, const DecodeArgs &a, hipStream_t s) {
  const dim3 grid = grid_for(a.shard_bytes, kc.nv, a.n_stripes);
  if (kc.variant == Variant::kRegister) {
    // live slots W: NV <= 128 / (2*W)
    RS_DEC_CASE(2, 1) RS_DEC_CASE(2, 2) RS_DEC_CASE(2, 4)
    RS_DEC_CASE(4, 1) RS_DEC_CASE(4, 2) RS_DEC_CASE(4, 4)
    RS_DEC_CASE(8, 1) RS_DEC_CASE(8, 2) RS_DEC_CASE(8, 4)
    RS_DEC_CASE(16, 1) RS_DEC_CASE(16, 2) RS_DEC_CASE(16, 4)
    RS_DEC_CASE(32, 1) RS_DEC_CASE(32, 2)
    return hipErrorInvalidValue;
  }
  if (kc.variant == Variant::kMatrixTiled) {
    const uint64_t regions = a.shard_bytes / 64 * (8 / kc.nv) / 64;
    const dim3 g(static_cast<uint32_t>(regions), grid.y, 1);
    // LDS-staged VGPR tables: -13 % against SGPR tables at NV=1
    if (kc.nv == 1) hipLaunchKernelGGL((k_decode_mtile_lds<kMtileEW, 1>), g, dim3(kBlock), 0, s, a);
    else hipLaunchKernelGGL((k_decode_mtile_lds<kMtileEW, 2>), g, dim3(kBlock), 0, s, a);
    return hipGetLastError();
  }
  if (kc.variant == Variant::kMatrix) {
    RS_MAT_NV(1) RS_MAT_NV(2) RS_MAT_NV(3) RS_MAT_NV(4)
    RS_MAT_NV(5) RS_MAT_NV(6) RS_MAT_NV(7) RS_MAT_NV(8)
    return hipErrorInvalidValue;
  }
  return launch_decode_generic(a, s);
}

hipError_t launch_tail_pack(const uint8_t *src, uint64_t src_stripe_stride, uint8_t *dst, uint64_t dst_stripe_stride,
                            uint64_t sb, uint64_t n, bool unpack, hipStream_t s) {
  if (sb % 64 == 0 || n == 0) return hipSuccess;
  trace_launch("k_tail_pack");
  const uint64_t blocks = (n * 64 + 255) / 256;
  hipLaunchKernelGGL(k_tail_pack, dim3(static_cast<uint32_t>(blocks)), dim3(256), 0, s, src, src_stripe_stride, dst,
                     dst_stripe_stride, sb, n, unpack ? 1 : 0);
  return hipGetLastError();
}

hipError_t launch_verify_compare(const uint8_t *a, uint64_t a_stripe_stride, const uint8_t *b,
                                 uint64_t b_stripe_stride, uint64_t sb, uint64_t n, uint32_t m, uint8_t *bad,
                                 uint64_t bad_stride, hipStream_t s) {
  if (n == 0 || m == 0 || sb == 0) return hipSuccess;
  trace_launch("k_verify_compare");
  const uint64_t segs = (sb + kVerifySeg - 1) / kVerifySeg, total = n * m * segs;
  // grid-stride over the work items: the grid stays inside the launch limits for any batch
  const dim3 grid(static_cast<uint32_t>(std::min<uint64_t>(total, 1u << 20)));
  with_int(load_mode(a, a_stripe_stride, b, b_stripe_stride, sb), kModes, [&](auto mode) {
    hipLaunchKernelGGL(k_verify_compare<decltype(mode)::value>, grid, dim3(256), 0, s, a, a_stripe_stride, b,
                       b_stripe_stride, sb, n, m, segs, bad, bad_stride);
  });
  return hipGetLastError();
}

hipError_t launch_verify_count(const uint8_t *bad, uint64_t bad_stride, uint64_t n, uint32_t m, uint64_t *count,
                               hipStream_t s) {
  hipError_t e = hipMemsetAsync(count, 0, sizeof(uint64_t), s);
  if (e != hipSuccess || n == 0 || m == 0) return e;
  trace_launch("k_verify_count");
  const uint64_t blocks = std::min<uint64_t>((n * m + 255) / 256, 1024);
  hipLaunchKernelGGL(k_verify_count, dim3(static_cast<uint32_t>(blocks)), dim3(256), 0, s, bad, bad_stride, n, m,
                     reinterpret_cast<unsigned long long *>(count));
  return hipGetLastError();
}

hipError_t launch_engine_fft(uint8_t *work, uint64_t sb, uint64_t pos, uint64_t size, uint64_t trunc,
                             const RsTab *tabs, bool inverse, hipStream_t s) {
  const dim3 grid = grid_for(sb, 1, 1);
  trace_launch("k_engine_transform");
  hipLaunchKernelGGL(k_engine_transform, grid, dim3(kBlock), 0, s, work, sb, pos, size, trunc, tabs,
                     inverse ? 1 : 0);
  return hipGetLastError();
}

hipError_t launch_mul_scalar(uint8_t *chunks, uint64_t bytes, const RsTab *tab, hipStream_t s) {
  const dim3 grid = grid_for(bytes, 1, 1);
  trace_launch("k_mul_scalar");
  hipLaunchKernelGGL(k_mul_scalar, grid, dim3(kBlock), 0, s, chunks, bytes, tab);
  return hipGetLastError();
}

}  // namespace rs
