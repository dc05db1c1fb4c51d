// rs_verify.cpp — rs_verify_batch_dev (scrub): do the stored recovery shards of every stripe
// still agree with its originals? Slices of stripes are encoded into a scratch by
// rs_encode_batch_dev itself, then k_verify_compare (rs_kernels.hip) compares the scratch with
// the stored shards and k_verify_count sums the flags. Also the shell the scrub
// family shares (rs_host.hpp): the argument front and the encode-and-compare step of verify and
// locate, and the per-code plans of locate, the multi-shard locate and update.
#include "rs_host.hpp"

namespace rs {
namespace host {

int check_scrub_args(uint64_t k, uint64_t m, size_t sb, uint64_t n, const void *d_original, uint64_t *orig_stride,
                     const void *d_recovery, uint64_t *rec_stride, const void *third) {
  if (k == 0) return fail(RS_ERR_TOO_FEW_ORIGINAL_SHARDS, "original_count == 0");
  int st = check_codec(k, m, sb);
  if (st || n == 0) return st;
  if (!d_original || !d_recovery || !third) return fail(RS_ERR_INVALID_ARGUMENT, "NULL device pointer");
  if (*orig_stride == 0) *orig_stride = k * sb;
  if (*rec_stride == 0) *rec_stride = m * sb;
  if (*orig_stride < k * sb || *rec_stride < m * sb) return fail(RS_ERR_INVALID_ARGUMENT, "stripe stride too small");
  return RS_OK;
}

// The encode call handles tails, low rate, small shards and every kernel family.
int encode_and_compare(uint64_t k, uint64_t m, uint64_t sb, uint64_t cnt, const uint8_t *orig, uint64_t ostride,
                       uint8_t *scratch, const uint8_t *rec, uint64_t rstride, uint8_t *bad, uint64_t bad_stride,
                       uint32_t flags, hipStream_t s) {
  if (int st = rs_encode_batch_dev(k, m, sb, cnt, orig, ostride, scratch, 0, flags, s)) return st;
  return hip_status(launch_verify_compare(scratch, m * sb, rec, rstride, sb, cnt, static_cast<uint32_t>(m), bad,
                                          bad_stride, s),
                    "launch_verify_compare");
}

PlanCache<CodePlan> g_locate_plans, g_locate_multi_plans, g_update_plans;

int get_code_plan(PlanCache<CodePlan> &cache, int dev, uint64_t k, uint64_t m,
                  const std::function<int(std::vector<uint16_t> &)> &build, std::shared_ptr<CodePlan> &out) {
  const std::string key = std::to_string(dev) + "/" + std::to_string(k) + "/" + std::to_string(m);
  {
    std::lock_guard<std::mutex> lk(g_plan_mu);
    if ((out = cache.find(key))) return RS_OK;
  }
  alloc_point();
  auto p = std::make_shared<CodePlan>();
  std::vector<uint16_t> blob;
  if (int st = build(blob)) return st;
  if (int st = upload(blob.data(), blob.size() * sizeof(uint16_t), dev, p->buf)) return st;
  std::lock_guard<std::mutex> lk(g_plan_mu);
  out = cache.insert(key, p);
  return RS_OK;
}

void release_code_plans() {
  std::lock_guard<std::mutex> lk(g_plan_mu);
  g_locate_plans.clear();
  g_locate_multi_plans.clear();
  g_update_plans.clear();
}

}  // namespace host
}  // namespace rs

using namespace rs;
using namespace rs::host;

extern "C" {

int rs_verify_batch_dev(uint64_t k, uint64_t m, size_t sb, uint64_t n_stripes, const void *d_original,
                        uint64_t orig_stride, const void *d_recovery, uint64_t rec_stride, uint8_t *d_bad,
                        uint64_t bad_stride, uint64_t *d_bad_count, uint32_t flags, rs_stream_t stream) {
  TraceScope ts;
  return guarded([&]() -> int {
    int st = check_scrub_args(k, m, sb, n_stripes, d_original, &orig_stride, d_recovery, &rec_stride, d_bad);
    if (st || n_stripes == 0) return st;
    if (bad_stride == 0) bad_stride = m;
    if (bad_stride < m) return fail(RS_ERR_INVALID_ARGUMENT, "bad_stride below recovery_count");
    // what the inner encode would reject, before anything is written (d_bad below); d_recovery
    // only feeds the compare, which takes any alignment
    if (sb % 64 == 0 && !align_nv({reinterpret_cast<uint64_t>(d_original), orig_stride}))
      return fail(RS_ERR_INVALID_ARGUMENT, "d_original / orig_stride must be 4-byte aligned");
    int dev;
    if ((st = current_device(&dev))) return st;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // the compare only ever stores 1: the flag rows start at 0 (bytes between rows are not touched)
    if (bad_stride == m) HIP_TRY(hipMemsetAsync(d_bad, 0, n_stripes * m, s));
    else HIP_TRY(hipMemset2DAsync(d_bad, bad_stride, 0, m, n_stripes, s));
    // each slice of stripes is encoded into a scratch of at most scratch_cap() bytes
    const uint8_t *orig = static_cast<const uint8_t *>(d_original), *rec = static_cast<const uint8_t *>(d_recovery);
    const uint64_t per = slice_stripes(n_stripes, m * sb);
    st = in_scratch_slices(n_stripes, per, per * m * sb, s, [&](uint64_t s0, uint64_t cnt, uint8_t *scratch) {
      return encode_and_compare(k, m, sb, cnt, orig + s0 * orig_stride, orig_stride, scratch, rec + s0 * rec_stride,
                                rec_stride, d_bad + s0 * bad_stride, bad_stride, flags, s);
    });
    if (st) return st;
    if (d_bad_count)
      HIP_TRY(launch_verify_count(d_bad, bad_stride, n_stripes, static_cast<uint32_t>(m), d_bad_count, s));
    return RS_OK;
  });
}

const char *rs_verify_kernel_name(uint64_t k, uint64_t m, size_t sb) {
  thread_local std::string name;
  name = std::string(rs_encode_kernel_name(k, m, sb)) + "+verify_compare";
  return name.c_str();
}

}  // extern "C"
