// rs_locate.cpp — rs_locate_batch_dev: name the one corrupt shard of an inconsistent stripe
// (DESIGN.md §3.10). Per slice of stripes: rs_encode_batch_dev into a scratch and
// k_verify_compare, as rs_verify_batch_dev does, then the locate kernels (rs_locate_kernels.hip)
// on the syndromes S_r = encode(originals)[r] ^ stored[r]. The plan of a code holds the logs of
// its coefficient ratios c[r][j] / c[0][j]; the multiply tables of a candidate are built on the
// device from them, so a plan is 2 k m bytes whatever the code's rate.
#include "rs_host.hpp"

namespace rs {
namespace host {

namespace {

static_assert(RS_LOCATE_CLEAN == kLocClean && RS_LOCATE_RECOVERY_SET == kLocRecoverySet &&
                  RS_LOCATE_UNLOCATED == kLocUnlocated,
              "the kernels' classes are the ABI's");

// dl[j * (m - 1) + r - 1] = log(c[r][j] / c[0][j]) in [0, 65535), r in [1, m): from the logs of the
// coefficients c (coef_logs). false if a coefficient is zero or two originals share the ratio of
// row 1 (neither happens in an MDS code).
bool ratio_logs(uint64_t k, uint64_t m, std::vector<uint16_t> &dl) {
  std::vector<uint16_t> cl;
  if (!coef_logs(k, m, cl)) return false;
  dl.assign(k * (m - 1), 0);
  for (uint64_t j = 0; j < k; j++)
    for (uint64_t r = 1; r < m; r++)
      dl[j * (m - 1) + r - 1] = static_cast<uint16_t>((uint32_t(cl[j * m + r]) + kModulus - cl[j * m]) % kModulus);
  if (m < 2) return true;
  std::vector<uint16_t> first(k);
  for (uint64_t j = 0; j < k; j++) first[j] = dl[j * (m - 1)];
  std::sort(first.begin(), first.end());
  return std::adjacent_find(first.begin(), first.end()) == first.end();
}

// Per (device, k, m): rlog [k] (the row-1 ratio logs, contiguous for the candidate match), then
// dl [k][m - 1]
int get_locate_plan(int dev, uint64_t k, uint64_t m, std::shared_ptr<CodePlan> &out) {
  return get_code_plan(g_locate_plans, dev, k, m, [&](std::vector<uint16_t> &blob) -> int {
    std::vector<uint16_t> dl;
    if (!ratio_logs(k, m, dl)) return fail(RS_ERR_DEVICE, "locate: the code's coefficient ratios are not distinct");
    blob.resize(k + dl.size());
    for (uint64_t j = 0; j < k; j++) blob[j] = dl[j * (m - 1)];
    std::copy(dl.begin(), dl.end(), blob.begin() + k);
    return RS_OK;
  }, out);
}

// The scratch of one slice: the encode, then per stripe the candidate's tables, its class, the
// compare's flags and the reject byte. Everything counts against RS_AMD_SCRATCH_CAP_MB.
struct Scratch {
  uint64_t per, tabs, cls, bad, reject, bytes;
  Scratch(uint64_t n, uint64_t m, uint64_t sb) {
    const uint64_t per_stripe = m * sb + (m - 1) * sizeof(RsTab) + sizeof(int32_t) + m + 1;
    per = slice_stripes(n, per_stripe);
    tabs = (per * m * sb + 15) / 16 * 16;
    cls = tabs + per * (m - 1) * sizeof(RsTab);
    bad = cls + per * sizeof(int32_t);
    reject = bad + per * m;
    bytes = reject + per;
  }
};

int locate_slices(int dev, uint64_t k, uint64_t m, uint64_t sb, uint64_t n, const uint8_t *orig, uint64_t ostride,
                  const uint8_t *rec, uint64_t rstride, int32_t *located, uint8_t *present, uint64_t pstride,
                  uint64_t *counts, hipStream_t s) {
  std::shared_ptr<CodePlan> plan;
  const uint16_t *dexp = nullptr, *dlog = nullptr, *dlw = nullptr;
  int st;
  if (m >= 2) {  // m == 1 has no ratio: a disagreeing stripe is unlocated
    if ((st = get_locate_plan(dev, k, m, plan))) return st;
    if ((st = device_tables(dev, &dexp, &dlog, &dlw))) return st;
  }
  const uint16_t *rlog = plan ? plan->u16() : nullptr;  // then dl at rlog + k
  const Scratch L(n, m, sb);
  const uint32_t k32 = static_cast<uint32_t>(k), m32 = static_cast<uint32_t>(m);
  return in_scratch_slices(n, L.per, L.bytes, s, [&](uint64_t s0, uint64_t cnt, uint8_t *base) {
    RsTab *tabs = reinterpret_cast<RsTab *>(base + L.tabs);
    int32_t *cls = reinterpret_cast<int32_t *>(base + L.cls);
    uint8_t *bad = base + L.bad, *reject = base + L.reject;
    if (s0 == 0 && counts)
      if (int st = hip_status(hipMemsetAsync(counts, 0, 4 * sizeof(uint64_t), s), "hipMemsetAsync(d_counts)")) return st;
    const uint8_t *rec0 = rec + s0 * rstride;
    // the compare and the confirm only ever store 1: flags and reject bytes start at 0
    if (int st = hip_status(hipMemsetAsync(bad, 0, L.per * (m + 1), s), "hipMemsetAsync(flags)")) return st;
    if (int st = encode_and_compare(k, m, sb, cnt, orig + s0 * ostride, ostride, base, rec0, rstride, bad, m, 0, s))
      return st;
    const char *what = "launch_locate_classify";
    hipError_t e = launch_locate_classify(base, m * sb, rec0, rstride, sb, cnt, k32, m32, bad, rlog,
                                          rlog ? rlog + k : nullptr, dexp, dlog, tabs, cls, s);
    if (e == hipSuccess) {
      what = "launch_locate_confirm";
      e = launch_locate_confirm(base, m * sb, rec0, rstride, sb, cnt, k32, m32, cls, tabs, reject, s);
    }
    if (e == hipSuccess) {
      what = "launch_locate_finish";
      e = launch_locate_finish(cls, bad, reject, k32, m32, cnt, located + s0, present ? present + s0 * pstride : nullptr,
                               pstride, counts, s);
    }
    return hip_status(e, what);
  });
}

// ---- the same algorithm on the host, P symbols per shard (rs_locate_selftest): S [m][P]
int64_t locate_scalar(uint64_t k, uint64_t m, uint64_t P, const uint16_t *S, const std::vector<uint16_t> &dl) {
  const Tables &t = tables();
  auto nonzero = [&](uint64_t r) { return std::any_of(S + r * P, S + (r + 1) * P, [](uint16_t v) { return v != 0; }); };
  uint64_t cnt = 0, first = 0;
  for (uint64_t r = m; r-- > 0;)
    if (nonzero(r)) cnt++, first = r;
  if (cnt == 0) return RS_LOCATE_CLEAN;
  if (m < 2) return RS_LOCATE_UNLOCATED;
  if (cnt == 1) return static_cast<int64_t>(k + first);
  if (cnt < m) return RS_LOCATE_RECOVERY_SET;
  uint64_t p = 0;
  while (S[p] == 0) p++;
  if (S[P + p] == 0) return RS_LOCATE_UNLOCATED;
  const uint32_t want = (uint32_t(t.log[S[P + p]]) + kModulus - t.log[S[p]]) % kModulus;
  int64_t cand = -1;
  for (uint64_t j = 0; j < k; j++)
    if (dl[j * (m - 1)] == want) cand = static_cast<int64_t>(j);
  if (cand < 0) return RS_LOCATE_UNLOCATED;
  for (uint64_t r = 1; r < m; r++)
    for (uint64_t q = 0; q < P; q++)
      if (mul16(S[q], dl[cand * (m - 1) + r - 1]) != S[r * P + q]) return RS_LOCATE_UNLOCATED;
  return cand;
}

}  // namespace

}  // namespace host
}  // namespace rs

using namespace rs;
using namespace rs::host;

extern "C" {

int rs_locate_batch_dev(uint64_t k, uint64_t m, size_t sb, uint64_t n_stripes, const void *d_original,
                        uint64_t orig_stride, const void *d_recovery, uint64_t rec_stride, int32_t *d_located,
                        uint8_t *d_present, uint64_t present_stride, uint64_t *d_counts, uint32_t flags,
                        rs_stream_t stream) {
  TraceScope ts;
  return guarded([&]() -> int {
    int st = check_scrub_args(k, m, sb, n_stripes, d_original, &orig_stride, d_recovery, &rec_stride, d_located);
    if (st || n_stripes == 0) return st;
    if (present_stride == 0) present_stride = k + m;
    if (present_stride < k + m) return fail(RS_ERR_INVALID_ARGUMENT, "present_stride below the shard count");
    // the syndrome ratios need a linear encode that reads every original
    if (flags != 0) return fail(RS_ERR_INVALID_ARGUMENT, "locate needs the corrected arithmetic (flags == 0)");
    if (sb % 64 == 0 && !align_nv({reinterpret_cast<uint64_t>(d_original), orig_stride}))
      return fail(RS_ERR_INVALID_ARGUMENT, "d_original / orig_stride must be 4-byte aligned");
    int dev;
    if ((st = current_device(&dev))) return st;
    return locate_slices(dev, k, m, sb, n_stripes, static_cast<const uint8_t *>(d_original), orig_stride,
                         static_cast<const uint8_t *>(d_recovery), rec_stride, d_located, d_present, present_stride,
                         d_counts, static_cast<hipStream_t>(stream));
  });
}

const char *rs_locate_kernel_name(uint64_t k, uint64_t m, size_t sb) {
  thread_local std::string name;
  name = std::string(rs_encode_kernel_name(k, m, sb)) + "+verify_compare+locate";
  return name.c_str();
}

int rs_locate_selftest(uint64_t k, uint64_t m, int trials, uint64_t seed, uint64_t *mismatches) {
  return guarded([&]() -> int {
    if (k == 0) return fail(RS_ERR_INVALID_ARGUMENT, "original_count == 0");
    const int hr = use_high_rate(k, m);
    if (hr < 0) return fail(-hr, "unsupported shard count (root.zig:397-415)");
    SplitMix64 rnd(seed);
    uint64_t bad = 0;
    std::vector<uint16_t> dl;
    if (m >= 2 && !ratio_logs(k, m, dl)) bad++;  // a zero coefficient or a repeated ratio
    constexpr uint64_t P = 4;  // symbols per shard
    std::vector<uint16_t> data(k * P), par(m * P), S(m * P);
    // a nonzero error at symbol q0 of the shard at x, and with probability 1/2 at each other symbol
    auto corrupt = [&](uint16_t *x) {
      const uint64_t q0 = rnd() % P;
      for (uint64_t q = 0; q < P; q++)
        if (q == q0 || (rnd() & 1)) x[q] ^= static_cast<uint16_t>(1 + rnd() % 65535);
    };
    for (int t = 0; bad == 0 && t < trials; t++) {
      for (auto &x : data) x = static_cast<uint16_t>(rnd());
      encode_columns(hr, k, m, P, data, par);
      for (int mode = 0; mode < 5; mode++) {
        std::vector<uint16_t> d2 = data, stored = par;
        int64_t want = RS_LOCATE_CLEAN;
        bool any_but_single = false;
        if (mode == 1) {  // one original
          const uint64_t j = rnd() % k;
          corrupt(&d2[j * P]);
          want = m >= 2 ? static_cast<int64_t>(j) : RS_LOCATE_UNLOCATED;
        } else if (mode == 2) {  // one recovery shard
          const uint64_t r = rnd() % m;
          corrupt(&stored[r * P]);
          want = m >= 2 ? static_cast<int64_t>(k + r) : RS_LOCATE_UNLOCATED;
        } else if (mode == 3) {  // two originals: never reported as one shard (m >= 3)
          if (m < 3 || k < 2) continue;
          const uint64_t a = rnd() % k, b = (a + 1 + rnd() % (k - 1)) % k;
          corrupt(&d2[a * P]);
          corrupt(&d2[b * P]);
          any_but_single = true;
        } else if (mode == 4) {  // two recovery shards of m >= 3
          if (m < 3) continue;
          const uint64_t a = rnd() % m, b = (a + 1 + rnd() % (m - 1)) % m;
          corrupt(&stored[a * P]);
          corrupt(&stored[b * P]);
          want = RS_LOCATE_RECOVERY_SET;
        }
        encode_columns(hr, k, m, P, d2, S);
        for (uint64_t i = 0; i < m * P; i++) S[i] ^= stored[i];
        const int64_t got = locate_scalar(k, m, P, S.data(), dl);
        if (any_but_single ? got >= 0 : got != want) bad++;
      }
    }
    if (mismatches) *mismatches = bad;
    return RS_OK;
  });
}

}  // extern "C"
