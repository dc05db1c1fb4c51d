// ring_main.cpp — host-only checks of the knob table (rs_env.hpp) and of the HIP-free parts of
// the host-batch ring (rs_host_ring.hpp) and of the scratch slicing (rs_slices.hpp). Built and run by tests/test_host_ring.py; exits 0
// when every check holds and prints each failed one otherwise.
#include <cstdio>

#include "rs_env.hpp"
#include "rs_host_ring.hpp"
#include "rs_slices.hpp"

using namespace rs;
using Runs = std::vector<std::pair<uint64_t, uint64_t>>;

static int g_failed = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      g_failed++;                                                     \
    }                                                                 \
  } while (0)

static void set(env::Knob k, const char *v) {
  if (v)
    setenv(env::kTable[k].name, v, 1);
  else
    unsetenv(env::kTable[k].name);
}

static void check_env() {
  // every numeric knob: default when unset or empty, clamped to its row's range when set
  for (int i = 0; i < env::kKnobs; i++) {
    const env::Knob k = static_cast<env::Knob>(i);
    const env::Row &r = env::kTable[i];
    if (r.kind != env::NUM) continue;
    set(k, nullptr);
    CHECK(env::num(k) == r.def && !env::given(k));
    set(k, "");
    CHECK(env::num(k) == r.def && env::given(k));
    if (r.lo > INT_MIN) {
      set(k, std::to_string(static_cast<long long>(r.lo) - 1).c_str());
      CHECK(env::num(k) == r.lo);
    }
    if (r.hi < INT_MAX) {
      set(k, std::to_string(static_cast<long long>(r.hi) + 1).c_str());
      CHECK(env::num(k) == r.hi);
    }
    set(k, "99999999999999999999");
    CHECK(env::num(k) == r.hi);
    set(k, std::to_string(r.lo).c_str());
    CHECK(env::num(k) == r.lo);
    set(k, nullptr);
  }
  set(env::HOST_SLOTS, "99");
  CHECK(env::num(env::HOST_SLOTS) == 8);
  set(env::HOST_SLOTS, "0");
  CHECK(env::num(env::HOST_SLOTS) == 1);
  set(env::HOST_SLOTS, "3");
  CHECK(env::num(env::HOST_SLOTS) == 3);
  set(env::HOST_SLOTS, nullptr);
  CHECK(env::num(env::HOST_SLOTS) == 2);
  // flags: off exactly for a whole number equal to 0, default when unset or empty; read at every use
  for (env::Knob k : {env::HOST_STAGE, env::JIT_SYNC}) {
    const bool def = env::kTable[k].def != 0;
    set(k, nullptr);
    CHECK(env::on(k) == def);
    set(k, "");
    CHECK(env::on(k) == def);
    for (const char *v : {"0", "00", "-0"}) {
      set(k, v);
      CHECK(!env::on(k));
    }
    for (const char *v : {"1", "2", "false", "0x", "on"}) {
      set(k, v);
      CHECK(env::on(k));
    }
    set(k, nullptr);
  }
  CHECK(env::on(env::HOST_STAGE) && !env::on(env::JIT_SYNC));
  // text and presence: an empty value is still "given"
  set(env::CACHE_DIR, nullptr);
  CHECK(!env::given(env::CACHE_DIR) && std::string(env::text(env::CACHE_DIR)).empty());
  set(env::CACHE_DIR, "");
  CHECK(env::given(env::CACHE_DIR) && std::string(env::text(env::CACHE_DIR)).empty());
  set(env::CACHE_DIR, "/x y");
  CHECK(std::string(env::text(env::CACHE_DIR)) == "/x y");
  set(env::CACHE_DIR, nullptr);
}

// host_copy against a plain loop, guard bytes between the rows included
struct Shape {
  uint64_t w, rows, ss, ds;  // row width, rows, source and destination strides
};
static void check_copy(const std::vector<Shape> &shapes) {
  std::vector<std::vector<uint8_t>> src, got, exp;
  std::vector<host::CopyJob> jobs;
  uint32_t x = 12345;
  for (const auto &sh : shapes) {
    const uint64_t w = sh.w, rows = sh.rows, ss = sh.ss, ds = sh.ds;
    src.emplace_back(rows * ss + 1);
    for (auto &b : src.back()) b = static_cast<uint8_t>((x = x * 1664525u + 1013904223u) >> 24);
    got.emplace_back(rows * ds + 1, 0xA5);
    exp.emplace_back(rows * ds + 1, 0xA5);
    for (uint64_t r = 0; r < rows; r++)
      for (uint64_t i = 0; i < w; i++) exp.back()[r * ds + i] = src.back()[r * ss + i];
  }
  for (size_t j = 0; j < shapes.size(); j++)  // after the vectors stopped moving
    jobs.push_back({got[j].data(), shapes[j].ds, src[j].data(), shapes[j].ss, shapes[j].w, shapes[j].rows});
  host::host_copy(jobs);
  for (size_t j = 0; j < shapes.size(); j++) CHECK(got[j] == exp[j]);
}

static void check_host_copy() {
  const uint64_t w = (4ull << 20) + 1;  // two pieces per row, the second of one byte
  for (const char *threads : {"1", "3", "64"}) {
    set(env::HOST_THREADS, threads);
    CHECK(host::stage_threads() == std::atoi(threads));
    check_copy({{w, 3, w + 64, w + 128}});                                       // 6 pieces
    check_copy({{w, 0, w + 64, w + 128}});                                       // zero rows
    check_copy({});                                                              // no job
    check_copy({{100, 1, 100, 100}});                                            // one piece
    check_copy({{4096, 5, 8192, 4096}, {w, 1, w, w + 7}, {1, 9, 3, 2}, {0, 4, 8, 8}});  // several jobs
  }
  set(env::HOST_THREADS, "1000");
  CHECK(host::stage_threads() == 64);
  set(env::HOST_THREADS, "0");
  CHECK(host::stage_threads() == 1);
  set(env::HOST_THREADS, nullptr);
  const int hw = static_cast<int>(std::thread::hardware_concurrency());
  CHECK(host::stage_threads() == std::max(1, std::min(16, hw)));
  check_copy({{w, 3, w + 64, w + 128}});
}

static void check_present_runs() {
  const uint8_t a[14] = {0, 1, 0, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1};  // test_host_batch_pipeline's patterns
  const uint8_t b[14] = {0, 1, 0, 1, 1, 1, 1, 0, 1, 1, 1, 0, 1, 1};
  CHECK(host::present_runs(a, 10) == (Runs{{1, 2}, {3, 7}, {8, 10}}));
  CHECK(host::present_runs(a + 10, 4) == (Runs{{0, 4}}));
  CHECK(host::present_runs(b, 10) == (Runs{{1, 2}, {3, 7}, {8, 10}}));
  CHECK(host::present_runs(b + 10, 4) == (Runs{{0, 1}, {2, 4}}));
  const uint8_t ones[6] = {1, 1, 1, 1, 1, 1}, zeros[6] = {}, alt[6] = {1, 0, 1, 0, 1, 0}, alt2[6] = {0, 1, 0, 1, 0, 1};
  CHECK(host::present_runs(ones, 6) == (Runs{{0, 6}}));
  CHECK(host::present_runs(zeros, 6).empty());
  CHECK(host::present_runs(ones, 0).empty());
  CHECK(host::present_runs(alt, 6) == (Runs{{0, 1}, {2, 3}, {4, 5}}));
  CHECK(host::present_runs(alt2, 6) == (Runs{{1, 2}, {3, 4}, {5, 6}}));
}

// The rule, worked out here: a slice holds 256 MiB of originals; if the narrowest run moves less
// than 8 MiB per copy, the slice grows until it does, up to 1 GiB of originals; never more than n.
static void check_slice_stripes() {
  const uint64_t MiB = 1ull << 20;
  {  // RS(10,4), 1 MiB shards, originals 0-3 lost: runs of 6 and 4 rows -> 4 MiB per stripe, 2 stripes reach 8 MiB
    const uint64_t sb = MiB, k = 10;
    const Runs runs{{4, 10}, {0, 4}};
    const uint64_t base = 256 * MiB / (k * sb);  // 25
    CHECK(base == 25);
    CHECK(host::reconstruct_slice_stripes(512, k * sb, sb, runs, env::kAuto) == base);
    CHECK(host::reconstruct_slice_stripes(7, k * sb, sb, runs, env::kAuto) == 7);
  }
  {  // RS(200,55), 256 KiB shards, every third data shard lost: the narrowest run is one 256 KiB row, which
     // wants 32 stripes per 8 MiB copy, more than the 256 MiB slice holds (5) and than 1 GiB / 50 MiB = 20
    const uint64_t sb = 256 << 10, k = 200, m = 55;
    std::vector<uint8_t> present(k + m, 1);
    for (uint64_t i = 0; i < k; i += 3) present[i] = 0;
    Runs runs = host::present_runs(present.data(), k);
    const Runs rec = host::present_runs(present.data() + k, m);
    runs.insert(runs.end(), rec.begin(), rec.end());
    uint64_t narrow_rows = UINT64_MAX;
    for (uint64_t i = 0; i < k;) {  // narrowest run of present rows, counted directly
      if (!present[i]) {
        i++;
        continue;
      }
      uint64_t j = i;
      while (j < k && present[j]) j++;
      narrow_rows = std::min(narrow_rows, j - i);
      i = j;
    }
    CHECK(narrow_rows == 1);  // shard 199 = 3 * 66 + 1 stands alone after the lost 198
    const uint64_t base = 256 * MiB / (k * sb), cap = 1024 * MiB / (k * sb);
    const uint64_t want = (8 * MiB + narrow_rows * sb - 1) / (narrow_rows * sb);
    CHECK(base == 5 && cap == 20 && want == 32);
    CHECK(host::reconstruct_slice_stripes(4096, k * sb, sb, runs, env::kAuto) == cap);
    CHECK(host::reconstruct_slice_stripes(12, k * sb, sb, runs, env::kAuto) == 12);  // capped at n
    CHECK(host::reconstruct_slice_stripes(4096, k * sb, sb, runs, 256) == base);      // the knob set: no widening
    CHECK(host::reconstruct_slice_stripes(4096, k * sb, sb, runs, 1) == 1);
    // without the lone last shard and the recovery rows: 2-row runs only, which want 16 stripes
    Runs two(runs.begin(), runs.end() - 1 - static_cast<long>(rec.size()));
    CHECK(host::reconstruct_slice_stripes(4096, k * sb, sb, two, env::kAuto) == 16);
  }
}

// The two rules of rs_slices.hpp, worked out here. Greedy (fit_stripes): floor(cap / stripe) stripes
// per slice, at least 1, at most n. Balanced (slice_stripes): the fewest slices the greedy rule
// allows under RS_AMD_SCRATCH_CAP_MB, then the stripes spread evenly over them.
static void check_scratch_slices() {
  const uint64_t GiB = 1ull << 30, MiB = 1ull << 20;
  CHECK(host::fit_stripes(100, 1000, 1001) == 1);       // one stripe exceeds the cap
  CHECK(host::fit_stripes(100, 1000, 1000) == 1);
  CHECK(host::fit_stripes(7, GiB, 1000) == 7);          // everything fits
  CHECK(host::fit_stripes(100, 1000, 10) == 100);       // exactly
  CHECK(host::fit_stripes(101, 1000, 10) == 100);
  // RS(10,4) and RS(10,4) + 2 restored rows, shards padded to 65600 bytes, 1200 stripes in 1 GiB:
  // 1073741824 / 918400 = 1169.1..., 1073741824 / 1049600 = 1023.0009...
  CHECK(14 * 65600 == 918400 && 1169ull * 918400 <= GiB && 1170ull * 918400 > GiB);
  CHECK(16 * 65600 == 1049600 && 1023ull * 1049600 <= GiB && 1024ull * 1049600 > GiB);
  CHECK(host::fit_stripes(1200, GiB, 14 * 65600) == 1169);
  CHECK(host::fit_stripes(1200, GiB, 16 * 65600) == 1023);

  set(env::SCRATCH_CAP_MB, "1");
  CHECK(host::scratch_cap() == MiB);
  CHECK(host::slice_stripes(9, 256 << 10) == 3);   // 4 fit: 3 slices of 3, not 4 + 4 + 1
  CHECK(host::slice_stripes(8, 256 << 10) == 4);   // 2 slices of 4
  CHECK(host::slice_stripes(5, 256 << 10) == 3);   // 2 slices: 3 + 2
  CHECK(host::slice_stripes(4, 256 << 10) == 4);   // one slice
  CHECK(host::slice_stripes(5, 2 * MiB) == 1);     // one stripe exceeds the cap: one per slice
  for (uint64_t stripe : std::vector<uint64_t>{1, 1000, 65600, 300000, MiB, MiB + 1})
    for (uint64_t n : std::vector<uint64_t>{1, 2, 3, 9, 16, 17, 1000, 65541}) {
      const uint64_t per = host::slice_stripes(n, stripe);
      const uint64_t fit = std::max<uint64_t>(1, MiB / stripe);  // stripes the cap holds
      const uint64_t fewest = (n + std::min(fit, n) - 1) / std::min(fit, n), slices = (n + per - 1) / per;
      CHECK(per >= 1 && per <= n);
      if (stripe <= MiB) CHECK(per * stripe <= MiB);
      CHECK(slices * per >= n);
      CHECK(slices == fewest);              // no more slices than the cap forces
      CHECK(slices * per - n < slices);     // even: no slice is short by a whole round
    }
  set(env::SCRATCH_CAP_MB, nullptr);
  CHECK(host::scratch_cap() == host::kScratchCap);
}

int main() {
  check_env();
  check_host_copy();
  check_present_runs();
  check_slice_stripes();
  check_scratch_slices();
  if (g_failed) return 1;
  std::printf("ring_main: ok\n");
  return 0;
}
