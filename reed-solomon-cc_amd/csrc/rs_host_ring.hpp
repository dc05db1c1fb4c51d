// rs_host_ring.hpp — the HIP-free parts of the host-batch ring (rs_host_batch.cpp): the
// threaded staging copies, the runs of present rows and the reconstruct slice size. Plain
// C++, so a host-only program can call them (tests/host/ring_main.cpp).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <thread>
#include <utility>
#include <vector>

#include "rs_env.hpp"

namespace rs {
namespace host {

inline int stage_threads() {
  const int v = env::num(env::HOST_THREADS), hw = static_cast<int>(std::thread::hardware_concurrency());
  return v != env::kAuto ? v : std::max(1, std::min(16, hw));
}

// strided host-to-host copies (rows of `w` bytes), split into <= 4 MiB pieces over host threads
struct CopyJob {
  uint8_t *d;
  uint64_t ds;
  const uint8_t *s;
  uint64_t ss, w, rows;
};
inline void host_copy(const std::vector<CopyJob> &jobs) {
  struct Piece {
    uint8_t *d;
    const uint8_t *s;
    uint64_t len;
  };
  std::vector<Piece> pieces;
  for (const CopyJob &j : jobs)
    for (uint64_t r = 0; r < j.rows; r++)
      for (uint64_t o = 0; o < j.w; o += 4ull << 20)
        pieces.push_back({j.d + r * j.ds + o, j.s + r * j.ss + o, std::min<uint64_t>(4ull << 20, j.w - o)});
  const int T = static_cast<int>(std::min<uint64_t>(static_cast<uint64_t>(stage_threads()), pieces.size()));
  auto work = [&](int t) {
    for (size_t i = static_cast<size_t>(t); i < pieces.size(); i += static_cast<size_t>(T))
      std::memcpy(pieces[i].d, pieces[i].s, pieces[i].len);
  };
  if (T <= 1) {
    if (T == 1) work(0);
    return;
  }
  struct Joiner {  // every thread that started is joined, also when starting a later one throws
    std::vector<std::thread> th;
    ~Joiner() {
      for (auto &x : th) x.join();
    }
  } j;
  j.th.reserve(T - 1);
  for (int t = 1; t < T; t++) j.th.emplace_back(work, t);
  work(0);
}

// [first, last) runs of present[0, rows): a slice's present shards cross PCIe as one strided
// copy per run (bridging gaps and one copy per row both measured slower: DESIGN.md §6 e2e)
inline std::vector<std::pair<uint64_t, uint64_t>> present_runs(const uint8_t *present, uint64_t rows) {
  std::vector<std::pair<uint64_t, uint64_t>> runs;
  for (uint64_t j = 0; j < rows; j++) {
    if (!present[j]) continue;
    if (!runs.empty() && runs.back().second == j)
      runs.back().second = j + 1;
    else
      runs.emplace_back(j, j + 1);
  }
  return runs;
}

constexpr uint64_t kHostSliceMiB = 256;  // input MiB per slice unless RS_AMD_HOST_SLICE_MB says otherwise
inline uint64_t host_slice_bytes(int slice_mb) {
  return (slice_mb != env::kAuto ? static_cast<uint64_t>(slice_mb) : kHostSliceMiB) << 20;
}
// Stripes per reconstruct slice: the default 256 MiB, widened (up to 1 GiB) until the narrowest
// run's copy moves >= 8 MiB — c4 with every third data shard lost copies 2-row runs of 256 KiB
// shards: 46.7 / 48.9 / 49.3 GiB/s at 256 / 512 / 1024 MiB slices, where RS(10,4)'s 6-row runs of
// 1 MiB shards want 256 (50.0 / 49.3 / 47.8; profiles/r06/e2e/slice/). A slice_mb other than
// env::kAuto (RS_AMD_HOST_SLICE_MB) fixes it.
inline uint64_t reconstruct_slice_stripes(uint64_t n, uint64_t stripe_bytes, uint64_t sb,
                                          const std::vector<std::pair<uint64_t, uint64_t>> &runs, int slice_mb) {
  uint64_t S = std::max<uint64_t>(1, host_slice_bytes(slice_mb) / stripe_bytes);
  if (slice_mb == env::kAuto) {
    uint64_t narrow = UINT64_MAX;
    for (const auto &r : runs) narrow = std::min(narrow, (r.second - r.first) * sb);
    if (narrow != UINT64_MAX) {
      const uint64_t want = ((8ull << 20) + narrow - 1) / narrow;
      S = std::max(S, std::min(want, std::max<uint64_t>(1, (1ull << 30) / stripe_bytes)));
    }
  }
  return std::min(S, n);
}

}  // namespace host
}  // namespace rs
