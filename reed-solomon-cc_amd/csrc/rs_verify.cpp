// rs_verify.cpp — rs_verify_batch_dev (scrub): do the stored recovery shards of every stripe
// still agree with its originals? Slices of stripes are encoded into a scratch by
// rs_encode_batch_dev itself, then k_verify_compare (rs_kernels.hip) compares the scratch with
// the stored shards and k_verify_count sums the flags.
#include "rs_host.hpp"

namespace rs {
namespace host {

namespace {

// Encode each slice of stripes into a scratch of at most scratch_cap() bytes and compare it
// with the stored recovery shards. The encode call handles tails, low rate, small shards and
// every kernel family; on any failure the scratch is freed on the stream.
int verify_slices(uint64_t k, uint64_t m, uint64_t sb, uint64_t n, const uint8_t *orig, uint64_t ostride,
                  const uint8_t *rec, uint64_t rstride, uint8_t *bad, uint64_t bad_stride, uint32_t flags,
                  hipStream_t s) {
  const uint64_t per = slice_stripes(n, m * sb);
  void *scratch = nullptr;
  HIP_TRY(dev_malloc_async(&scratch, per * m * sb, s));
  int st = RS_OK;
  for (uint64_t s0 = 0; st == RS_OK && s0 < n; s0 += per) {
    const uint64_t cnt = std::min(per, n - s0);
    st = rs_encode_batch_dev(k, m, sb, cnt, orig + s0 * ostride, ostride, scratch, 0, flags, s);
    if (st != RS_OK) break;
    const hipError_t e = launch_verify_compare(static_cast<const uint8_t *>(scratch), m * sb, rec + s0 * rstride,
                                               rstride, sb, cnt, static_cast<uint32_t>(m), bad + s0 * bad_stride,
                                               bad_stride, s);
    if (e != hipSuccess) st = hip_fail(e, "launch_verify_compare");
  }
  (void)hipFreeAsync(scratch, s);
  return st;
}

}  // namespace

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
    if (k == 0) return fail(RS_ERR_TOO_FEW_ORIGINAL_SHARDS, "original_count == 0");
    int st = check_codec(k, m, sb);
    if (st) return st;
    if (n_stripes == 0) return RS_OK;
    if (!d_original || !d_recovery || !d_bad) return fail(RS_ERR_INVALID_ARGUMENT, "NULL device pointer");
    if (orig_stride == 0) orig_stride = k * sb;
    if (rec_stride == 0) rec_stride = m * sb;
    if (bad_stride == 0) bad_stride = m;
    if (orig_stride < k * sb || rec_stride < m * sb) return fail(RS_ERR_INVALID_ARGUMENT, "stripe stride too small");
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
    if ((st = verify_slices(k, m, sb, n_stripes, static_cast<const uint8_t *>(d_original), orig_stride,
                            static_cast<const uint8_t *>(d_recovery), rec_stride, d_bad, bad_stride, flags, s)))
      return st;
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
