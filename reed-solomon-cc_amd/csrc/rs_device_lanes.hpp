// rs_device_lanes.hpp — what the locate and the update kernels (rs_locate_kernels.hip,
// rs_locate_multi_kernels.hip, rs_update_kernels.hip) share on the device: one lane's dword pairs of
// a shard in the chunk layout at three access widths (16-byte vectors, dwords, bytes), the tail
// chunk by bytes, and the multiply tables of a field element built from its log. The pass over a
// stripe's syndromes that the two locates run on these loads is rs_device_span.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "rs_device.hpp"
#include "rs_gf.hpp"

namespace rs {
namespace dev {

// ---- loads of one lane's dword pairs. a / b point at the lane's low bytes; the high bytes lie 32
// further (one 64-byte chunk). MODE 2: 16-byte accesses (NV 4), 1: dwords, 0: bytes.
template <int MODE>
struct Lanes {
  static constexpr int NV = MODE == 2 ? 4 : 1;
};

__device__ __forceinline__ uint32_t ld4_bytes(const uint8_t *p) {
  return static_cast<uint32_t>(p[0]) | static_cast<uint32_t>(p[1]) << 8 | static_cast<uint32_t>(p[2]) << 16 |
         static_cast<uint32_t>(p[3]) << 24;
}

// s = a ^ b
template <int MODE>
__device__ __forceinline__ void ld_xor(Sym<Lanes<MODE>::NV> &s, const uint8_t *__restrict__ a,
                                       const uint8_t *__restrict__ b) {
  if constexpr (MODE == 2) {
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    const v4u al = __builtin_nontemporal_load(reinterpret_cast<const v4u *>(a));
    const v4u ah = __builtin_nontemporal_load(reinterpret_cast<const v4u *>(a + 32));
    const v4u bl = __builtin_nontemporal_load(reinterpret_cast<const v4u *>(b));
    const v4u bh = __builtin_nontemporal_load(reinterpret_cast<const v4u *>(b + 32));
#pragma unroll
    for (int v = 0; v < 4; v++) {
      s.l[v] = al[v] ^ bl[v];
      s.h[v] = ah[v] ^ bh[v];
    }
  } else if constexpr (MODE == 1) {
    s.l[0] = *reinterpret_cast<const uint32_t *>(a) ^ *reinterpret_cast<const uint32_t *>(b);
    s.h[0] = *reinterpret_cast<const uint32_t *>(a + 32) ^ *reinterpret_cast<const uint32_t *>(b + 32);
  } else {
    s.l[0] = ld4_bytes(a) ^ ld4_bytes(b);
    s.h[0] = ld4_bytes(a + 32) ^ ld4_bytes(b + 32);
  }
}

// s = a
template <int MODE>
__device__ __forceinline__ void ld(Sym<Lanes<MODE>::NV> &s, const uint8_t *a) {
  if constexpr (MODE == 2) {
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    const v4u al = __builtin_nontemporal_load(reinterpret_cast<const v4u *>(a));
    const v4u ah = __builtin_nontemporal_load(reinterpret_cast<const v4u *>(a + 32));
#pragma unroll
    for (int v = 0; v < 4; v++) {
      s.l[v] = al[v];
      s.h[v] = ah[v];
    }
  } else if constexpr (MODE == 1) {
    s.l[0] = *reinterpret_cast<const uint32_t *>(a);
    s.h[0] = *reinterpret_cast<const uint32_t *>(a + 32);
  } else {
    s.l[0] = ld4_bytes(a);
    s.h[0] = ld4_bytes(a + 32);
  }
}

__device__ __forceinline__ void st4_bytes(uint8_t *p, uint32_t v) {
  p[0] = static_cast<uint8_t>(v);
  p[1] = static_cast<uint8_t>(v >> 8);
  p[2] = static_cast<uint8_t>(v >> 16);
  p[3] = static_cast<uint8_t>(v >> 24);
}

// the stores that match ld
template <int MODE>
__device__ __forceinline__ void st(uint8_t *a, const Sym<Lanes<MODE>::NV> &s) {
  if constexpr (MODE == 2) {
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    v4u l, h;
#pragma unroll
    for (int v = 0; v < 4; v++) {
      l[v] = s.l[v];
      h[v] = s.h[v];
    }
    __builtin_nontemporal_store(l, reinterpret_cast<v4u *>(a));
    __builtin_nontemporal_store(h, reinterpret_cast<v4u *>(a + 32));
  } else if constexpr (MODE == 1) {
    *reinterpret_cast<uint32_t *>(a) = s.l[0];
    *reinterpret_cast<uint32_t *>(a + 32) = s.h[0];
  } else {
    st4_bytes(a, s.l[0]);
    st4_bytes(a + 32, s.h[0]);
  }
}

// The tail chunk (k_tail_pack's layout): t = sb % 64 bytes at `whole`, h = t / 2 symbols, low
// bytes at [0, h), high bytes at [h, t). Lane `lane` (< 8) takes symbols [4 lane, 4 lane + 4).
__device__ __forceinline__ void ld_xor_tail(Sym<1> &s, const uint8_t *__restrict__ a, const uint8_t *__restrict__ b,
                                            uint32_t h, uint32_t lane) {
  s.l[0] = s.h[0] = 0;
#pragma unroll
  for (uint32_t q = 0; q < 4; q++) {
    const uint32_t i = 4 * lane + q;
    if (i < h) {
      s.l[0] |= static_cast<uint32_t>(a[i] ^ b[i]) << (8 * q);
      s.h[0] |= static_cast<uint32_t>(a[h + i] ^ b[h + i]) << (8 * q);
    }
  }
}

// the same for one source, and the store that matches it (bytes past the tail are not touched)
__device__ __forceinline__ void ld_tail(Sym<1> &s, const uint8_t *a, uint32_t h, uint32_t lane) {
  s.l[0] = s.h[0] = 0;
#pragma unroll
  for (uint32_t q = 0; q < 4; q++) {
    const uint32_t i = 4 * lane + q;
    if (i < h) {
      s.l[0] |= static_cast<uint32_t>(a[i]) << (8 * q);
      s.h[0] |= static_cast<uint32_t>(a[h + i]) << (8 * q);
    }
  }
}

__device__ __forceinline__ void st_tail(uint8_t *a, const Sym<1> &s, uint32_t h, uint32_t lane) {
#pragma unroll
  for (uint32_t q = 0; q < 4; q++) {
    const uint32_t i = 4 * lane + q;
    if (i < h) {
      a[i] = static_cast<uint8_t>(s.l[0] >> (8 * q));
      a[h + i] = static_cast<uint8_t>(s.h[0] >> (8 * q));
    }
  }
}

// rs_gf.cpp make_tab (corrected multiply) on the device: the v_perm tables of the multiplication
// by exp[lm], from the images of the 16 basis symbols 1 << b.
__device__ inline void build_tab(RsTab *out, uint32_t lm, const uint16_t *__restrict__ d_exp,
                                 const uint16_t *__restrict__ d_log) {
  uint32_t img[16];
#pragma unroll
  for (int b = 0; b < 16; b++) {
    const uint32_t sum = static_cast<uint32_t>(d_log[1u << b]) + lm;
    img[b] = d_exp[(sum + (sum >> 16)) & 0xFFFFu];  // rs_gf.hpp add_mod
  }
  constexpr int kOff[6] = {0, 3, 6, 8, 11, 14}, kBits[6] = {3, 3, 2, 3, 3, 2}, kSlot[6] = {0, 2, 4, 5, 7, 9};
  uint32_t lo[10], hi[10];
#pragma unroll
  for (int i = 0; i < 10; i++) lo[i] = hi[i] = 0;
#pragma unroll
  for (int f = 0; f < 6; f++) {
#pragma unroll
    for (uint32_t v = 0; v < (1u << kBits[f]); v++) {
      uint32_t p = 0;
#pragma unroll
      for (int b = 0; b < kBits[f]; b++)
        if (v >> b & 1) p ^= img[kOff[f] + b];
      const int w = kSlot[f] + (v >> 2), sh = 8 * (v & 3);
      lo[w] |= (p & 0xFFu) << sh;
      hi[w] |= (p >> 8) << sh;
    }
  }
#pragma unroll
  for (int i = 0; i < 10; i++) {
    out->lo[i] = lo[i];
    out->hi[i] = hi[i];
  }
  out->flags = 0;
  out->log_m = lm;
  out->pad[0] = out->pad[1] = 0;
}

}  // namespace dev
}  // namespace rs
