// rs_rebuild.cpp — rs_rebuild_batch_dev: every lost shard of a stripe comes back, recovery shards
// included. With E the missing originals, Q the missing recovery shards and R the
// first |E| present recovery rows of a stripe, the syndromes s_r = p_r ^ Enc_r(d') (d' the data with
// E read as zero, a missing p_r read as zero) give x_E = A^-1 s_R with A = G[R][E], and
// p_q = s_q ^ sum_t G[q][E_t] x_t for q in Q.
//  * Fast form: one pass on the code's syndrome network (psyn::Spec::rebuild, plan from
//    k_psyn_rebuild_plan): k + e_s shard rows of traffic per stripe.
//  * General form, everything else, in slices of stripes: the per-stripe reconstruct into slots
//    [0, e_o), k_rebuild_gather of the stripe's originals into a scratch, the encode of that scratch,
//    k_rebuild_pick of rows Q into slots [e_o, e_s) (rs_rebuild_kernels.hip): about
//    3k + m + e_o + 2 e_r rows per stripe.
#include "rs_host.hpp"

namespace rs {
namespace host {
namespace {

// One slice of the general form: the meta blocks (a multiple of 16 bytes each, so what follows
// keeps the alignment sb allows), the gathered originals [per][k][sb], their encode [per][m][sb].
// Everything counts against RS_AMD_SCRATCH_CAP_MB, and nothing else is allocated here.
struct Scratch {
  uint64_t per, data, par, bytes;
  Scratch(uint64_t n, uint64_t k, uint64_t m, uint64_t sb) {
    const uint64_t mw = rebuild_meta_words(k, m) * sizeof(uint32_t);
    per = slice_stripes(n, (k + m) * sb + mw);
    data = per * mw;
    par = data + per * k * sb;
    bytes = par + per * m * sb;
  }
};

int rebuild_slices(uint64_t k, uint64_t m, uint64_t sb, uint64_t n, const uint8_t *d_present, uint64_t pstride,
                   uint32_t max_e, const uint8_t *orig, uint64_t ostride, const uint8_t *rec, uint64_t rstride,
                   uint8_t *out, uint64_t outstride, int32_t *status, hipStream_t s) {
  const Scratch L(n, k, m, sb);
  const uint32_t k32 = static_cast<uint32_t>(k), m32 = static_cast<uint32_t>(m);
  return in_scratch_slices(n, L.per, L.bytes, s, [&](uint64_t s0, uint64_t cnt, uint8_t *base) {
    uint8_t *data = base + L.data, *par = base + L.par, *ro = out + s0 * outstride;
    uint32_t *meta = reinterpret_cast<uint32_t *>(base);
    const uint8_t *pr = d_present + s0 * pstride;
    // the missing originals into slots [0, min(e_o, max_e)); its status gives way to the final one
    int st = rs_reconstruct_batch_dev_patterns(k, m, sb, cnt, pr, pstride, max_e, orig + s0 * ostride, ostride,
                                               rec + s0 * rstride, rstride, ro, outstride, nullptr, 0, s);
    if (st) return st;
    hipError_t e = launch_rebuild_prepare(pr, pstride, k32, m32, max_e, cnt, meta, status ? status + s0 : nullptr, s);
    if (e == hipSuccess)
      e = launch_rebuild_gather(orig + s0 * ostride, ostride, ro, outstride, sb, cnt, k32, m32, meta, data, s);
    if (e != hipSuccess) return hip_fail(e, "launch_rebuild_gather");
    // the rows of skipped stripes are encoded from whatever the scratch holds and never read
    if ((st = rs_encode_batch_dev(k, m, sb, cnt, data, k * sb, par, m * sb, 0, s))) return st;
    return hip_status(launch_rebuild_pick(par, sb, cnt, k32, m32, max_e, meta, ro, outstride, s), "launch_rebuild_pick");
  });
}

bool overlap(const void *a, uint64_t a_bytes, const void *b, uint64_t b_bytes) {
  const uint64_t a0 = reinterpret_cast<uint64_t>(a), b0 = reinterpret_cast<uint64_t>(b);
  return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

bool rebuild_spec(uint64_t k, uint64_t m, psyn::Spec &spec) {
  if (k == 0 || use_high_rate(k, m) != 1 || !psyn::supports(k, m, jit::kUnitBytes)) return false;
  jit::NetSpec map;
  encode_map(k, m, 0, map);
  spec.k = static_cast<uint32_t>(k);
  spec.m = static_cast<uint32_t>(m);
  spec.flags = 0;
  spec.images = std::move(map.images);
  spec.cantor.assign(cantor_basis(), cantor_basis() + 16);
  spec.rebuild = true;
  return true;
}

// ---- the plan kernel's algebra on the host, P symbols per shard (rs_rebuild_selftest)
struct Field {
  const Tables &t = tables();
  uint16_t mul(uint16_t a, uint16_t b) const { return b ? mul16(a, t.log[b]) : 0; }
  uint16_t inv(uint16_t a) const { return t.exp[(kModulus - t.log[a]) % kModulus]; }
};

// G [m][k]; data [k][P] and par [m][P] with the missing shards' symbols poisoned by the caller;
// out [e_s][P]: the missing originals, then the missing recovery shards. false: singular.
bool rebuild_scalar(int hr, uint64_t k, uint64_t m, uint64_t P, const std::vector<uint16_t> &G,
                    const std::vector<uint8_t> &present, const std::vector<uint16_t> &data,
                    const std::vector<uint16_t> &par, std::vector<uint16_t> &out) {
  const Field f;
  std::vector<uint64_t> E, Q, R;
  for (uint64_t j = 0; j < k; j++)
    if (!present[j]) E.push_back(j);
  for (uint64_t r = 0; r < m; r++) {
    if (!present[k + r]) Q.push_back(r);
    else if (R.size() < E.size()) R.push_back(r);
  }
  const uint64_t e = E.size();
  // syndromes of every row: erased originals and absent rows read as zero
  std::vector<uint16_t> d0 = data, syn(m * P);
  for (uint64_t j : E) std::fill(d0.begin() + j * P, d0.begin() + (j + 1) * P, 0);
  encode_columns(hr, k, m, P, d0, syn);
  for (uint64_t r = 0; r < m; r++)
    if (present[k + r])
      for (uint64_t q = 0; q < P; q++) syn[r * P + q] ^= par[r * P + q];
  // Gauss-Jordan on [A | I]
  std::vector<uint16_t> A(e * 2 * e);
  for (uint64_t i = 0; i < e; i++)
    for (uint64_t j = 0; j < 2 * e; j++) A[i * 2 * e + j] = j < e ? G[R[i] * k + E[j]] : (j - e == i ? 1 : 0);
  for (uint64_t c = 0; c < e; c++) {
    uint64_t piv = c;
    while (piv < e && A[piv * 2 * e + c] == 0) piv++;
    if (piv == e) return false;
    for (uint64_t j = 0; j < 2 * e; j++) std::swap(A[c * 2 * e + j], A[piv * 2 * e + j]);
    const uint16_t iv = f.inv(A[c * 2 * e + c]);
    for (uint64_t j = 0; j < 2 * e; j++) A[c * 2 * e + j] = f.mul(A[c * 2 * e + j], iv);
    for (uint64_t i = 0; i < e; i++) {
      const uint16_t fr = A[i * 2 * e + c];
      if (i == c || fr == 0) continue;
      for (uint64_t j = 0; j < 2 * e; j++) A[i * 2 * e + j] ^= f.mul(fr, A[c * 2 * e + j]);
    }
  }
  // coefficient of s_r in output j, as k_psyn_rebuild_plan lays them out
  out.assign((e + Q.size()) * P, 0);
  for (uint64_t j = 0; j < e + Q.size(); j++)
    for (uint64_t r = 0; r < m; r++) {
      int64_t ir = -1;
      for (uint64_t i = 0; i < e; i++) ir = R[i] == r ? static_cast<int64_t>(i) : ir;
      uint16_t c = 0;
      if (j < e) {
        c = ir >= 0 ? A[j * 2 * e + e + ir] : 0;
      } else if (ir >= 0) {
        for (uint64_t t = 0; t < e; t++) c ^= f.mul(G[Q[j - e] * k + E[t]], A[t * 2 * e + e + ir]);
      } else if (r == Q[j - e]) {
        c = 1;
      }
      if (c)
        for (uint64_t q = 0; q < P; q++) out[j * P + q] ^= f.mul(syn[r * P + q], c);
    }
  return true;
}

}  // namespace
}  // namespace host
}  // namespace rs

using namespace rs;
using namespace rs::host;

extern "C" {

int rs_rebuild_batch_dev(uint64_t k, uint64_t m, size_t sb, uint64_t n_stripes, const uint8_t *d_present,
                         uint64_t present_stride, uint32_t max_e, const void *d_original, uint64_t orig_stride,
                         const void *d_recovery, uint64_t rec_stride, void *d_rebuilt, uint64_t out_stride,
                         int32_t *d_status, uint32_t flags, rs_stream_t stream) {
  TraceScope ts;
  return guarded([&]() -> int {
    if (k == 0) return fail(RS_ERR_TOO_FEW_ORIGINAL_SHARDS, "original_count == 0");
    int st = check_codec(k, m, sb);
    if (st) return st;
    if (n_stripes == 0 || max_e == 0) return RS_OK;
    if (!d_present || !d_original || !d_recovery || !d_rebuilt)
      return fail(RS_ERR_INVALID_ARGUMENT, "NULL device pointer");
    if (max_e > m) return fail(RS_ERR_INVALID_ARGUMENT, "max_e above recovery_count");
    if (present_stride == 0) present_stride = k + m;
    if (orig_stride == 0) orig_stride = k * sb;
    if (rec_stride == 0) rec_stride = m * sb;
    if (out_stride == 0) out_stride = static_cast<uint64_t>(max_e) * sb;
    if (present_stride < k + m) return fail(RS_ERR_INVALID_ARGUMENT, "present_stride below the shard count");
    if (orig_stride < k * sb || rec_stride < m * sb || out_stride < static_cast<uint64_t>(max_e) * sb)
      return fail(RS_ERR_INVALID_ARGUMENT, "stripe stride too small");
    // a lost recovery shard is the encode of the restored originals only where the encode is linear
    // and reads every original
    if (flags != 0) return fail(RS_ERR_INVALID_ARGUMENT, "rebuild needs the corrected arithmetic (flags == 0)");
    if (sb % 64 == 0 && !align_nv({reinterpret_cast<uint64_t>(d_original), reinterpret_cast<uint64_t>(d_recovery),
                                   reinterpret_cast<uint64_t>(d_rebuilt), orig_stride, rec_stride, out_stride}))
      return fail(RS_ERR_INVALID_ARGUMENT, "device pointers/strides must be 4-byte aligned");
    if (overlap(d_rebuilt, n_stripes * out_stride, d_original, n_stripes * orig_stride) ||
        overlap(d_rebuilt, n_stripes * out_stride, d_recovery, n_stripes * rec_stride))
      return fail(RS_ERR_INVALID_ARGUMENT, "d_rebuilt overlaps d_original / d_recovery");
    int dev;
    if ((st = current_device(&dev))) return st;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint8_t *orig = static_cast<const uint8_t *>(d_original), *rec = static_cast<const uint8_t *>(d_recovery);
    uint8_t *out = static_cast<uint8_t *>(d_rebuilt);
    // high rate only: the network and G come from the high-rate construction (encode_map), and a
    // low-rate code is encoded by another one (rs_lowrate.cpp)
    if (!is_low_rate(k, m) && psyn_enabled(k, m, sb, 0) &&
        align_nv({reinterpret_cast<uint64_t>(d_original), reinterpret_cast<uint64_t>(d_recovery),
                  reinterpret_cast<uint64_t>(d_rebuilt), orig_stride, rec_stride, out_stride}) == 4) {
      bool ran = false;
      st = psyn_rebuild(dev, k, m, sb, n_stripes, d_present, present_stride, max_e, orig, orig_stride, rec, rec_stride,
                        out, out_stride, d_status, s, &ran);
      if (st || ran) return st;
    }
    return rebuild_slices(k, m, sb, n_stripes, d_present, present_stride, max_e, orig, orig_stride, rec, rec_stride, out,
                          out_stride, d_status, s);
  });
}

const char *rs_rebuild_kernel_name(uint64_t k, uint64_t m, size_t sb, uint32_t max_e) {
  thread_local std::string name;
  if (k != 0 && use_high_rate(k, m) == 1 && psyn_enabled(k, m, sb, 0))
    name = "psyn_rebuild_k" + std::to_string(k) + "_m" + std::to_string(m);
  else
    name = std::string(rs_patterns_kernel_name(k, m, sb, max_e, 0)) + "+rebuild_gather+" +
           rs_encode_kernel_name(k, m, sb) + "+rebuild_pick";
  return name.c_str();
}

int rs_rebuild_compile_check(uint64_t k, uint64_t m, double *compile_ms, uint64_t *code_bytes) {
  return guarded([&]() -> int {
    if (k == 0) return fail(RS_ERR_INVALID_ARGUMENT, "original_count == 0");
    int st = check_codec(k, m, jit::kUnitBytes);
    if (st) return st;
    psyn::Spec spec;
    if (!rebuild_spec(k, m, spec)) return fail(RS_ERR_INVALID_ARGUMENT, "no rebuild syndrome network for this code");
    std::string err;
    size_t bytes = 0;
    if (!psyn::compile_check(spec, err, compile_ms, &bytes)) return fail(RS_ERR_DEVICE, err);
    if (code_bytes) *code_bytes = bytes;
    return RS_OK;
  });
}

int rs_rebuild_selftest(uint64_t k, uint64_t m, int trials, uint64_t seed, uint64_t *mismatches) {
  return guarded([&]() -> int {
    if (k == 0) return fail(RS_ERR_INVALID_ARGUMENT, "original_count == 0");
    const int hr = use_high_rate(k, m);
    if (hr < 0) return fail(-hr, "unsupported shard count (root.zig:397-415)");
    const Tables &t = tables();
    SplitMix64 rnd(seed);
    uint64_t bad = 0;
    std::vector<uint16_t> cl, G(m * k);
    if (!coef_logs(k, m, cl)) bad++;  // a zero coefficient
    for (uint64_t j = 0; j < k; j++)
      for (uint64_t r = 0; r < m; r++) G[r * k + j] = t.exp[cl[j * m + r]];
    constexpr uint64_t P = 4;  // symbols per shard
    std::vector<uint16_t> data(k * P), par(m * P), got;
    std::vector<uint64_t> pick(std::max(k, m));
    for (int tr = 0; bad == 0 && tr < trials; tr++) {
      for (auto &x : data) x = static_cast<uint16_t>(rnd());
      encode_columns(hr, k, m, P, data, par);
      // e_s in [1, m] split into e_o originals and e_r recovery shards; the first three trials are
      // parity only, originals only, and as many as the code bears
      uint64_t es = 1 + rnd() % m, eo = rnd() % (es + 1);
      if (tr % 4 == 0) eo = 0;
      if (tr % 4 == 1) eo = es;
      if (tr % 4 == 2) es = m, eo = rnd() % (es + 1);
      eo = std::min(eo, k);
      const uint64_t er = es - eo;
      std::vector<uint8_t> present(k + m, 1);
      // the heads of two partial Fisher-Yates shuffles
      for (uint64_t j = 0; j < k; j++) pick[j] = j;
      for (uint64_t i = 0; i < eo; i++) {
        std::swap(pick[i], pick[i + rnd() % (k - i)]);
        present[pick[i]] = 0;
      }
      for (uint64_t r = 0; r < m; r++) pick[r] = r;
      for (uint64_t i = 0; i < er; i++) {
        std::swap(pick[i], pick[i + rnd() % (m - i)]);
        present[k + pick[i]] = 0;
      }
      std::vector<uint16_t> pd = data, pp = par;  // the missing slots hold poison
      for (uint64_t i = 0; i < k + m; i++)
        if (!present[i])
          for (uint64_t q = 0; q < P; q++) (i < k ? pd[i * P + q] : pp[(i - k) * P + q]) = static_cast<uint16_t>(rnd());
      if (!rebuild_scalar(hr, k, m, P, G, present, pd, pp, got)) {
        bad++;
        break;
      }
      uint64_t slot = 0;
      for (uint64_t i = 0; i < k + m; i++)
        if (!present[i]) {
          const uint16_t *want = i < k ? &data[i * P] : &par[(i - k) * P];
          for (uint64_t q = 0; q < P; q++) bad += got[slot * P + q] != want[q];
          slot++;
        }
    }
    if (mismatches) *mismatches = bad;
    return RS_OK;
  });
}

}  // extern "C"
