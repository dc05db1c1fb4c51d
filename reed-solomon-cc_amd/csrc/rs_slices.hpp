// rs_slices.hpp — how many stripes share one device scratch: the two rules every sliced path
// uses (in_scratch_slices, rs_host.hpp). Plain C++, HIP-free, so a host-only program can call
// them (tests/host/ring_main.cpp).
#pragma once
#include <algorithm>
#include <cstdint>

#include "rs_env.hpp"

namespace rs {
namespace host {

constexpr uint64_t kScratchCap = 2ull << 30;  // generic path: scratch per launch
static_assert(env::kTable[env::SCRATCH_CAP_MB].def == kScratchCap >> 20, "the knob's default is kScratchCap");
// the generic kernels' scratch cap per launch: kScratchCap, or RS_AMD_SCRATCH_CAP_MB
inline uint64_t scratch_cap() { return static_cast<uint64_t>(env::num(env::SCRATCH_CAP_MB)) << 20; }

// greedy: as many stripes as fit cap_bytes, at least one, at most n (the last slice may be
// short). The callers with a constant cap (kScratchCap, kTailSliceBytes, 1 GiB, 4 GiB) do not
// honour RS_AMD_SCRATCH_CAP_MB.
inline uint64_t fit_stripes(uint64_t n, uint64_t cap_bytes, uint64_t per_stripe_bytes) {
  return std::max<uint64_t>(1, std::min<uint64_t>(n, cap_bytes / per_stripe_bytes));
}

// stripes per scratch slice: as many as fit the cap, spread evenly over the slices (a short
// last slice runs its launches at lower occupancy)
inline uint64_t slice_stripes(uint64_t n, uint64_t per_stripe_bytes) {
  const uint64_t fit = fit_stripes(n, scratch_cap(), per_stripe_bytes);
  const uint64_t slices = (n + fit - 1) / fit;
  return (n + slices - 1) / slices;
}

}  // namespace host
}  // namespace rs
