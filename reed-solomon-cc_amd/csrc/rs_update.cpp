// rs_update.cpp — rs_update_batch_dev: the small write. Some originals of a
// stripe change and the stored recovery shards follow in place: recovery[r] ^= sum over the
// changed originals j of c[r][j] * (old_j ^ new_j), c the coefficients of the corrected encode.
// The plan of a code holds the logs of c, 2 k m bytes; per slice of stripes k_update_prepare
// validates the index rows and builds the multiply tables of the named originals on the device,
// then k_update_apply walks the parity (rs_update_kernels.hip).
#include "rs_host.hpp"

namespace rs {
namespace host {

bool coef_logs(uint64_t k, uint64_t m, std::vector<uint16_t> &cl) {
  const Tables &t = tables();
  const bool low = is_low_rate(k, m);
  std::vector<uint16_t> in(k, 0), out(m);
  cl.assign(k * m, 0);
  for (uint64_t j = 0; j < k; j++) {
    in[j] = 1;  // symbol 1 is the field's one
    if (low) scalar_encode_low(in.data(), k, m, false, out.data());
    else scalar_encode(in.data(), k, m, false, false, out.data());
    in[j] = 0;
    for (uint64_t r = 0; r < m; r++) {
      if (out[r] == 0) return false;
      cl[j * m + r] = t.log[out[r]];
    }
  }
  return true;
}

void encode_columns(int hr, uint64_t k, uint64_t m, uint64_t P, const std::vector<uint16_t> &d,
                    std::vector<uint16_t> &p) {
  std::vector<uint16_t> col(k), out(m);
  for (uint64_t q = 0; q < P; q++) {
    for (uint64_t j = 0; j < k; j++) col[j] = d[j * P + q];
    if (hr == 0) scalar_encode_low(col.data(), k, m, false, out.data());
    else scalar_encode(col.data(), k, m, false, false, out.data());
    for (uint64_t r = 0; r < m; r++) p[r * P + q] = out[r];
  }
}

namespace {

static_assert(RS_UPDATE_NONE == kUpdateNone && RS_ERR_INVALID_SHARD_INDEX == kUpdateInvalidIndex &&
                  RS_ERR_DUPLICATE_SHARD_INDEX == kUpdateDuplicateIndex,
              "the kernels' values are the ABI's");

// Per (device, k, m): cl [k][m], the logs of the encode's coefficients
int get_update_plan(int dev, uint64_t k, uint64_t m, std::shared_ptr<CodePlan> &out) {
  return get_code_plan(g_update_plans, dev, k, m, [&](std::vector<uint16_t> &cl) -> int {
    if (!coef_logs(k, m, cl)) return fail(RS_ERR_DEVICE, "update: the code has a zero coefficient");
    return RS_OK;
  }, out);
}

// The scratch of one slice, per stripe: the tables of max_u slots, the slot list and the live
// count. Everything counts against RS_AMD_SCRATCH_CAP_MB.
struct Scratch {
  uint64_t per, list, live, bytes;
  Scratch(uint64_t n, uint64_t m, uint64_t max_u) {
    per = slice_stripes(n, max_u * m * sizeof(RsTab) + max_u * sizeof(uint32_t) + sizeof(uint32_t));
    list = per * max_u * m * sizeof(RsTab);
    live = list + per * max_u * sizeof(uint32_t);
    bytes = live + per * sizeof(uint32_t);
  }
};

int update_slices(int dev, uint64_t k, uint64_t m, uint64_t sb, uint64_t n, uint32_t max_u, const uint32_t *index,
                  uint64_t istride, const uint8_t *d_old, const uint8_t *d_new, uint64_t cstride, uint8_t *rec,
                  uint64_t rstride, int32_t *status, hipStream_t s) {
  std::shared_ptr<CodePlan> plan;
  const uint16_t *dexp = nullptr, *dlog = nullptr, *dlw = nullptr;
  int st;
  if ((st = get_update_plan(dev, k, m, plan))) return st;
  if ((st = device_tables(dev, &dexp, &dlog, &dlw))) return st;
  const Scratch L(n, m, max_u);
  const uint32_t k32 = static_cast<uint32_t>(k), m32 = static_cast<uint32_t>(m);
  return in_scratch_slices(n, L.per, L.bytes, s, [&](uint64_t s0, uint64_t cnt, uint8_t *base) {
    RsTab *tabs = reinterpret_cast<RsTab *>(base);
    uint32_t *list = reinterpret_cast<uint32_t *>(base + L.list), *live = reinterpret_cast<uint32_t *>(base + L.live);
    const char *what = "launch_update_prepare";
    hipError_t e = launch_update_prepare(index + s0 * istride, istride, max_u, cnt, k32, m32, plan->u16(), dexp, dlog,
                                         tabs, list, live, status ? status + s0 : nullptr, s);
    if (e == hipSuccess) {
      what = "launch_update_apply";
      e = launch_update_apply(d_old ? d_old + s0 * cstride : nullptr, d_new + s0 * cstride, cstride,
                              rec + s0 * rstride, rstride, sb, cnt, m32, max_u, list, live, tabs, s);
    }
    return hip_status(e, what);
  });
}

bool overlap(const void *a, uint64_t a_bytes, const void *b, uint64_t b_bytes) {
  const uint64_t a0 = reinterpret_cast<uint64_t>(a), b0 = reinterpret_cast<uint64_t>(b);
  return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

}  // namespace

}  // namespace host
}  // namespace rs

using namespace rs;
using namespace rs::host;

extern "C" {

int rs_update_batch_dev(uint64_t k, uint64_t m, size_t sb, uint64_t n_stripes, uint32_t max_u, const uint32_t *d_index,
                        uint64_t index_stride, const void *d_old, const void *d_new, uint64_t change_stride,
                        void *d_recovery, uint64_t rec_stride, int32_t *d_status, uint32_t flags, rs_stream_t stream) {
  TraceScope ts;
  return guarded([&]() -> int {
    if (k == 0) return fail(RS_ERR_TOO_FEW_ORIGINAL_SHARDS, "original_count == 0");
    int st = check_codec(k, m, sb);
    if (st) return st;
    if (n_stripes == 0 || max_u == 0) return RS_OK;
    if (!d_index || !d_new || !d_recovery) return fail(RS_ERR_INVALID_ARGUMENT, "NULL device pointer");
    if (max_u > k) return fail(RS_ERR_INVALID_ARGUMENT, "max_u above original_count");
    if (index_stride == 0) index_stride = max_u;
    if (change_stride == 0) change_stride = max_u * sb;
    if (rec_stride == 0) rec_stride = m * sb;
    if (index_stride < max_u) return fail(RS_ERR_INVALID_ARGUMENT, "index_stride below max_u");
    if (change_stride < max_u * sb || rec_stride < m * sb)
      return fail(RS_ERR_INVALID_ARGUMENT, "stripe stride too small");
    // the delta of a recovery shard is c[r][j] * (old ^ new) only where the encode is linear and
    // reads every original
    if (flags != 0) return fail(RS_ERR_INVALID_ARGUMENT, "update needs the corrected arithmetic (flags == 0)");
    if (sb % 64 == 0 && !align_nv({reinterpret_cast<uint64_t>(d_old), reinterpret_cast<uint64_t>(d_new),
                                   reinterpret_cast<uint64_t>(d_recovery), change_stride, rec_stride}))
      return fail(RS_ERR_INVALID_ARGUMENT, "d_old / d_new / d_recovery and their strides must be 4-byte aligned");
    // in place: a change buffer inside the recovery range would be read after it was written
    if (overlap(d_recovery, n_stripes * rec_stride, d_new, n_stripes * change_stride) ||
        (d_old && overlap(d_recovery, n_stripes * rec_stride, d_old, n_stripes * change_stride)))
      return fail(RS_ERR_INVALID_ARGUMENT, "d_recovery overlaps d_old / d_new");
    int dev;
    if ((st = current_device(&dev))) return st;
    return update_slices(dev, k, m, sb, n_stripes, max_u, d_index, index_stride, static_cast<const uint8_t *>(d_old),
                         static_cast<const uint8_t *>(d_new), change_stride, static_cast<uint8_t *>(d_recovery),
                         rec_stride, d_status, static_cast<hipStream_t>(stream));
  });
}

int rs_update_selftest(uint64_t k, uint64_t m, uint32_t max_u, int trials, uint64_t seed, uint64_t *mismatches) {
  return guarded([&]() -> int {
    if (k == 0) return fail(RS_ERR_INVALID_ARGUMENT, "original_count == 0");
    const int hr = use_high_rate(k, m);
    if (hr < 0) return fail(-hr, "unsupported shard count (root.zig:397-415)");
    SplitMix64 rnd(seed);
    uint64_t bad = 0;
    std::vector<uint16_t> cl;
    if (!coef_logs(k, m, cl)) bad++;  // a zero coefficient
    constexpr uint64_t P = 4;         // symbols per shard
    std::vector<uint16_t> data(k * P), stored(m * P), want(m * P);
    const uint64_t u_max = std::min<uint64_t>(max_u, k);
    std::vector<uint64_t> pick(k);
    for (int t = 0; bad == 0 && u_max > 0 && t < trials; t++) {
      for (auto &x : data) x = static_cast<uint16_t>(rnd());
      encode_columns(hr, k, m, P, data, stored);
      // 1..u_max distinct originals: the head of a partial Fisher-Yates shuffle
      const uint64_t u = 1 + rnd() % u_max;
      for (uint64_t j = 0; j < k; j++) pick[j] = j;
      for (uint64_t i = 0; i < u; i++) {
        std::swap(pick[i], pick[i + rnd() % (k - i)]);
        const uint64_t j = pick[i];
        for (uint64_t q = 0; q < P; q++) {
          const uint16_t delta = static_cast<uint16_t>(rnd());
          data[j * P + q] ^= delta;
          for (uint64_t r = 0; r < m; r++) stored[r * P + q] ^= mul16(delta, cl[j * m + r]);
        }
      }
      encode_columns(hr, k, m, P, data, want);
      for (uint64_t i = 0; i < m * P; i++) bad += stored[i] != want[i];
    }
    if (mismatches) *mismatches = bad;
    return RS_OK;
  });
}

}  // extern "C"
