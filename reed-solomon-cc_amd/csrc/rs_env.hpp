// rs_env.hpp — every environment variable librs_amd.so reads, and the only getenv calls.
//
// One rule for all knobs: a value is read at every use (never cached: callers and tests
// change knobs inside one process). An unset or empty variable gives the table's default to
// num() and on(). num() parses a decimal integer (anything else counts as 0) and clamps it
// to [lo, hi]. on() is false exactly when the value is a whole decimal number equal to 0
// ("0", "00", "-0"); any other non-empty text is true. text() returns the value as written
// ("" when unset) and given() tells "set at all", an empty value included.
// A default of kAuto means the caller computes it at run time (the row says how).
#pragma once
#include <climits>
#include <cstdlib>
#include <string>

namespace rs {
namespace env {

enum Knob {
  CACHE_DIR, FDEC, HOST_SLICE_MB, HOST_SLOTS, HOST_STAGE, HOST_THREADS, JIT, JIT_CACHE_MAX, JIT_SYNC, JIT_VERBOSE,
  LOW_BLOCK, PDEC, PDEC_AFTER, PDEC_MAX, PDEC_QUEUE, PLAN_CACHE, SCRATCH_CAP_MB,
  DECODE, FFT, FFT_ALLOW_SPILL, FFT_DEBUG, FFT_PREFETCH, JIT_DUMP, LOW_TRIM, NET_ASYNC_AFTER, NET_ASYNC_BLOCKS,
  NET_BALANCE, NET_SHARED, NET_SMALL, NET_SMALL_ENCODE, NET_TILE, NV, PATTERNS,
  FFT_CHECK_INVERSE, FFT_CHECK_PIECES, INJECT_HOST_FAIL, NET_CHECK_PIECES,
  kKnobs
};

// PUBLIC: documented in include/reedsol.h. MEASURE: selects another kernel family or code
// shape for measurements and for the tests that reach those forms (code-shape knobs are part
// of the kernels' cache keys). TEST: fault injection and compile-check-only knobs.
enum Class { PUBLIC, MEASURE, TEST };
enum Kind { NUM, FLAG, TEXT, SET };

constexpr int kAuto = -1;
constexpr int kMax = INT_MAX;

struct Row {
  const char *name;
  Class cls;
  Kind kind;
  int def, lo, hi;  // NUM: default and clamp; FLAG: def 0 / 1; TEXT, SET (only given() is asked): unused
  const char *doc;
};

// Rows in the order of Knob. Keep one row per line: tests/test_env_knobs.py parses this text.
inline constexpr Row kTable[] = {
    {"RS_AMD_CACHE_DIR", PUBLIC, TEXT, 0, 0, 0, "directory of the on-disk code-object cache; empty: no disk cache; unset: $XDG_CACHE_HOME/rs_amd or ~/.cache/rs_amd"},
    {"RS_AMD_FDEC", PUBLIC, TEXT, 0, 0, 0, "0: never the fused FFT reconstruct; 1: whenever it applies, and no pattern-compiled kernels; anything else: auto"},
    {"RS_AMD_HOST_SLICE_MB", PUBLIC, NUM, kAuto, 1, kMax, "input MiB per host-batch slice; unset: 256, and reconstructs widen it for narrow row runs"},
    {"RS_AMD_HOST_SLOTS", PUBLIC, NUM, 2, 1, 8, "slices in flight in the host-batch ring"},
    {"RS_AMD_HOST_STAGE", PUBLIC, FLAG, 1, 0, 1, "0: pageable host buffers go to the runtime as they are, without the ring's pinned staging"},
    {"RS_AMD_HOST_THREADS", PUBLIC, NUM, kAuto, 1, 64, "host threads of the staging copies; unset: min(16, hardware threads)"},
    {"RS_AMD_JIT", PUBLIC, FLAG, 1, 0, 1, "0: no hipRTC kernels at all, every call runs on the precompiled table kernels"},
    {"RS_AMD_JIT_CACHE_MAX", PUBLIC, NUM, 1024, 0, kMax, "loaded hipRTC modules per process; past it new maps run on the table kernels"},
    {"RS_AMD_JIT_SYNC", PUBLIC, FLAG, 0, 0, 1, "1: background compiles run in the calling thread instead"},
    {"RS_AMD_JIT_VERBOSE", PUBLIC, SET, 0, 0, 0, "set at all: report every compile and disk-cache hit on stderr"},
    {"RS_AMD_LOW_BLOCK", PUBLIC, FLAG, 1, 0, 1, "0: low-rate reconstructs keep the W-point decode instead of the block form"},
    {"RS_AMD_PDEC", PUBLIC, FLAG, 1, 0, 1, "0: no pattern-compiled fused reconstruct kernels"},
    {"RS_AMD_PDEC_AFTER", PUBLIC, NUM, 2, 1, kMax, "a pattern is compiled in on its n-th use"},
    {"RS_AMD_PDEC_MAX", PUBLIC, NUM, 32, 0, kMax, "pattern-compiled kernels per code and device"},
    {"RS_AMD_PDEC_QUEUE", PUBLIC, NUM, 2, 0, kMax, "pattern compiles waiting on the worker before new ones are put off"},
    {"RS_AMD_PLAN_CACHE", PUBLIC, NUM, 4096, 1, kMax, "plans kept per kind before the least recently used are dropped"},
    {"RS_AMD_SCRATCH_CAP_MB", PUBLIC, NUM, 2048, 1, kMax, "scratch MiB per launch of the generic kernels"},
    {"RS_AMD_DECODE", MEASURE, TEXT, 0, 0, 0, "reconstruct family: auto (unset), net, fft or matrix"},
    {"RS_AMD_FFT", MEASURE, FLAG, 1, 0, 1, "0: no bit-sliced FFT kernels"},
    {"RS_AMD_FFT_ALLOW_SPILL", MEASURE, SET, 0, 0, 0, "set at all: run an FFT kernel build that spills registers"},
    {"RS_AMD_FFT_DEBUG", MEASURE, NUM, 0, 0, 255, "measurement builds of the FFT kernels, a bit mask (rs_fftnet.cpp debug_of)"},
    {"RS_AMD_FFT_PREFETCH", MEASURE, NUM, 4, 0, 8, "next-chunk positions the FFT kernels load early"},
    {"RS_AMD_JIT_DUMP", MEASURE, TEXT, 0, 0, 0, "set at all: directory that receives the source of compile-checked kernels"},
    {"RS_AMD_LOW_TRIM", MEASURE, FLAG, 1, 0, 1, "0: low-rate reconstructs read every present recovery row"},
    {"RS_AMD_NET_ASYNC_AFTER", MEASURE, NUM, 2, 1, kMax, "a background network compile starts at a map's n-th use"},
    {"RS_AMD_NET_ASYNC_BLOCKS", MEASURE, NUM, kAuto, -1, kMax, "input-block cap of background-compiled networks (0: none); unset: jit::kMaxAsyncBlocks"},
    {"RS_AMD_NET_BALANCE", MEASURE, FLAG, 1, 0, 1, "0: one wave per 8-output tile in the shared-input networks"},
    {"RS_AMD_NET_SHARED", MEASURE, NUM, kAuto, INT_MIN, kMax, "0: the classic networks instead of the shared-input form; unset: shared for 2..8 tiles"},
    {"RS_AMD_NET_SMALL", MEASURE, FLAG, 1, 0, 1, "0: 1 / 2 KiB shards stay on the table kernels"},
    {"RS_AMD_NET_SMALL_ENCODE", MEASURE, FLAG, 0, 0, 1, "1: encodes of 1 / 2 KiB shards take the networks too"},
    {"RS_AMD_NET_TILE", MEASURE, NUM, 8, 4, 8, "network outputs per workgroup: 8, below 8 means 4"},
    {"RS_AMD_NV", MEASURE, NUM, kAuto, INT_MIN, kMax, "16-byte vectors per lane of the table kernels: 1, 2 or 4; anything else: chosen per shape"},
    {"RS_AMD_PATTERNS", MEASURE, TEXT, 0, 0, 0, "fft / matrix / ...: per-stripe reconstruct family; empty, auto or psyn: chosen per shape"},
    {"RS_AMD_FFT_CHECK_INVERSE", TEST, FLAG, 0, 0, 1, "1: rs_fft_compile_check takes the inverse form where one exists"},
    {"RS_AMD_FFT_CHECK_PIECES", TEST, NUM, 1, 1, 2, "2: rs_fft_compile_check takes the 1 KiB-shard variant"},
    {"RS_AMD_INJECT_HOST_FAIL", TEST, NUM, kAuto, -1, kMax, "slice index of a host batch that fails with RS_ERR_DEVICE"},
    {"RS_AMD_NET_CHECK_PIECES", TEST, NUM, 1, 1, 4, "2 / 4: rs_net_compile_check takes that small-shard variant"},
};
static_assert(sizeof(kTable) / sizeof(kTable[0]) == kKnobs, "one table row per Knob, in the same order");

inline bool given(Knob k) { return std::getenv(kTable[k].name) != nullptr; }

inline const char *text(Knob k) {
  const char *e = std::getenv(kTable[k].name);
  return e ? e : "";
}

inline int num(Knob k) {
  const Row &r = kTable[k];
  const char *e = text(k);
  if (!*e) return r.def;
  const long v = std::strtol(e, nullptr, 10);
  return v < r.lo ? r.lo : v > r.hi ? r.hi : static_cast<int>(v);
}

inline bool on(Knob k) {
  const char *e = text(k);
  if (!*e) return kTable[k].def != 0;
  char *end = nullptr;
  const long v = std::strtol(e, &end, 10);
  return !(end != e && *end == '\0' && v == 0);
}

// where the code-object cache lives when RS_AMD_CACHE_DIR is unset ("" if nowhere)
inline std::string user_cache_dir() {
  if (const char *x = std::getenv("XDG_CACHE_HOME"))
    if (*x) return std::string(x) + "/rs_amd";
  if (const char *h = std::getenv("HOME"))
    if (*h) return std::string(h) + "/.cache/rs_amd";
  return "";
}

}  // namespace env
}  // namespace rs
