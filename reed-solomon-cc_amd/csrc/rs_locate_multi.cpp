// rs_locate_multi.cpp — rs_locate_multi_batch_dev: name up to max_t corrupt shards of an
// inconsistent stripe. Every symbol of a stripe shares the set T of corrupt
// shards, so the syndrome vectors S(p) = sum_{i in T} G_i * err_i(p), G = [C | I_m], span a
// subspace of dimension rho <= |T|, and the columns of G in that subspace are T. Per slice of
// stripes: rs_encode_batch_dev into a scratch and k_verify_compare, as rs_verify_batch_dev does,
// then max_t + 1 rounds of k_mloc_check / k_mloc_extend that grow a reduced basis of the span,
// k_mloc_match and k_mloc_finish (rs_locate_multi_kernels.hip). The plan of a code holds the logs
// of its coefficients, 2 k m bytes; the unit columns of G are implicit.
#include "rs_host.hpp"

namespace rs {
namespace host {

namespace {

static_assert(RS_LOCATE_MAX_T == kMlocMaxT && RS_LOCATE_UNLOCATED == kLocUnlocated, "the kernels' values are the ABI's");

// Per (device, k, m): cl [k][m], the logs of the encode's coefficients
int get_mloc_plan(int dev, uint64_t k, uint64_t m, std::shared_ptr<CodePlan> &out) {
  return get_code_plan(g_locate_multi_plans, dev, k, m, [&](std::vector<uint16_t> &cl) -> int {
    if (!coef_logs(k, m, cl)) return fail(RS_ERR_DEVICE, "locate: the code has a zero coefficient");
    return RS_OK;
  }, out);
}

// The scratch of one slice: the encode, then per stripe the basis' tables, the failing position,
// the state, the pivot rows, the columns found and their number, the basis and the compare's
// flags (widest alignment first). Everything counts against RS_AMD_SCRATCH_CAP_MB.
struct Scratch {
  uint64_t per, tabs, pos, state, piv, found, nfound, basis, bad, bytes;
  Scratch(uint64_t n, uint64_t m, uint64_t sb, uint64_t max_t) {
    const uint64_t per_stripe = m * sb + max_t * m * (sizeof(RsTab) + sizeof(uint16_t)) + sizeof(uint64_t) +
                                2 * max_t * sizeof(uint32_t) + 2 * sizeof(uint32_t) + m;
    per = slice_stripes(n, per_stripe);
    tabs = (per * m * sb + 15) / 16 * 16;
    pos = tabs + per * max_t * m * sizeof(RsTab);
    state = pos + per * sizeof(uint64_t);  // right behind pos: one memset starts both
    piv = state + per * sizeof(int32_t);
    found = piv + per * max_t * sizeof(uint32_t);
    nfound = found + per * max_t * sizeof(int32_t);
    basis = nfound + per * sizeof(uint32_t);
    bad = basis + per * max_t * m * sizeof(uint16_t);
    bytes = bad + per * m;
  }
};

int mloc_slices(int dev, uint64_t k, uint64_t m, uint64_t sb, uint64_t n, uint32_t max_t, const uint8_t *orig,
                uint64_t ostride, const uint8_t *rec, uint64_t rstride, int32_t *count, int32_t *located,
                uint64_t lstride, uint8_t *present, uint64_t pstride, uint64_t *counts, hipStream_t s) {
  std::shared_ptr<CodePlan> plan;
  const uint16_t *dexp = nullptr, *dlog = nullptr, *dlw = nullptr;
  int st;
  if ((st = get_mloc_plan(dev, k, m, plan))) return st;
  if ((st = device_tables(dev, &dexp, &dlog, &dlw))) return st;
  const Scratch L(n, m, sb, max_t);
  const uint32_t k32 = static_cast<uint32_t>(k), m32 = static_cast<uint32_t>(m);
  return in_scratch_slices(n, L.per, L.bytes, s, [&](uint64_t s0, uint64_t cnt, uint8_t *base) {
    RsTab *tabs = reinterpret_cast<RsTab *>(base + L.tabs);
    uint64_t *pos = reinterpret_cast<uint64_t *>(base + L.pos);
    uint32_t *piv = reinterpret_cast<uint32_t *>(base + L.piv), *nfound = reinterpret_cast<uint32_t *>(base + L.nfound);
    int32_t *found = reinterpret_cast<int32_t *>(base + L.found), *state = reinterpret_cast<int32_t *>(base + L.state);
    uint16_t *basis = reinterpret_cast<uint16_t *>(base + L.basis);
    uint8_t *bad = base + L.bad;
    if (s0 == 0 && counts)
      if (int st = hip_status(hipMemsetAsync(counts, 0, (max_t + 2) * sizeof(uint64_t), s), "hipMemsetAsync(d_counts)"))
        return st;
    const uint8_t *rec0 = rec + s0 * rstride;
    // the compare only ever stores 1: the flags start at 0. Every stripe starts active
    // (kMlocActive) with no failing position (kMlocNoPos): both are 0xFF bytes.
    if (int st = hip_status(hipMemsetAsync(bad, 0, L.per * m, s), "hipMemsetAsync(flags)")) return st;
    if (int st = hip_status(hipMemsetAsync(pos, 0xFF, L.per * (sizeof(uint64_t) + sizeof(int32_t)), s),
                            "hipMemsetAsync(pos, state)"))
      return st;
    if (int st = encode_and_compare(k, m, sb, cnt, orig + s0 * ostride, ostride, base, rec0, rstride, bad, m, 0, s))
      return st;
    const char *what = "launch_mloc_check";
    hipError_t e = hipSuccess;
    for (uint32_t round = 0; e == hipSuccess && round <= max_t; round++) {
      what = "launch_mloc_check";
      e = launch_mloc_check(base, m * sb, rec0, rstride, sb, cnt, m32, round, max_t, state, bad, piv, tabs, pos, s);
      if (e != hipSuccess) break;
      what = "launch_mloc_extend";
      e = launch_mloc_extend(base, m * sb, rec0, rstride, sb, cnt, m32, round, max_t, dexp, dlog, state, pos, piv,
                             basis, tabs, s);
    }
    if (e == hipSuccess) {
      what = "launch_mloc_match";
      e = launch_mloc_match(cnt, k32, m32, max_t, plan->u16(), dexp, dlog, state, piv, basis, found, nfound, s);
    }
    if (e == hipSuccess) {
      what = "launch_mloc_finish";
      e = launch_mloc_finish(state, found, nfound, k32, m32, max_t, cnt, count + s0,
                             located ? located + s0 * lstride : nullptr, lstride,
                             present ? present + s0 * pstride : nullptr, pstride, counts, s);
    }
    return hip_status(e, what);
  });
}

// ---- the same algorithm on the host, P symbols per shard (rs_locate_multi_selftest): S [m][P],
// cl [k][m]. Returns the number of located shards (ascending in `out`) or RS_LOCATE_UNLOCATED.
int32_t mloc_scalar(uint64_t k, uint64_t m, uint64_t P, const uint16_t *S, const std::vector<uint16_t> &cl,
                    uint32_t max_t, std::vector<int32_t> &out) {
  const Tables &t = tables();
  auto mul = [&](uint16_t a, uint16_t b) -> uint16_t { return b == 0 ? 0 : mul16(a, t.log[b]); };
  std::vector<std::vector<uint16_t>> B;
  std::vector<uint64_t> piv;
  out.clear();
  for (uint32_t round = 0;; round++) {
    // the check: the smallest symbol outside the span
    uint64_t p = P;
    for (uint64_t q = 0; q < P && p == P; q++)
      for (uint64_t r = 0; r < m; r++) {
        uint16_t sum = 0;
        for (size_t j = 0; j < B.size(); j++) sum ^= mul(B[j][r], S[piv[j] * P + q]);
        if (sum != S[r * P + q]) {
          p = q;
          break;
        }
      }
    if (p == P) break;  // rank = round
    if (round == max_t) return RS_LOCATE_UNLOCATED;
    // extend: reduce S(p), normalise at its first nonzero row, reduce the earlier vectors
    std::vector<uint16_t> v(m);
    for (uint64_t r = 0; r < m; r++) {
      v[r] = S[r * P + p];
      for (size_t j = 0; j < B.size(); j++) v[r] ^= mul(B[j][r], S[piv[j] * P + p]);
    }
    uint64_t rho = 0;
    while (v[rho] == 0) rho++;
    const uint16_t inv_log = static_cast<uint16_t>((kModulus - t.log[v[rho]]) % kModulus);
    for (auto &x : v) x = mul16(x, inv_log);
    for (auto &b : B) {
      const uint16_t c = b[rho];
      for (uint64_t r = 0; r < m; r++) b[r] ^= mul(v[r], c);
    }
    B.push_back(v);
    piv.push_back(rho);
  }
  // match: the columns of G = [C | I] in the span
  for (uint64_t c = 0; c < k + m; c++) {
    bool in = true;
    if (c < k) {
      for (uint64_t r = 0; r < m && in; r++) {
        uint16_t sum = 0;
        for (size_t l = 0; l < B.size(); l++) sum ^= mul16(B[l][r], cl[c * m + piv[l]]);
        in = sum == t.exp[cl[c * m + r]];
      }
    } else {
      in = false;
      for (size_t l = 0; l < B.size(); l++)
        if (piv[l] == c - k) {
          in = true;
          for (uint64_t r = 0; r < m; r++)
            if (r != c - k && B[l][r]) in = false;
        }
    }
    if (in) out.push_back(static_cast<int32_t>(c));
  }
  if (out.size() != B.size()) {
    out.clear();
    return RS_LOCATE_UNLOCATED;
  }
  return static_cast<int32_t>(out.size());
}

}  // namespace

}  // namespace host
}  // namespace rs

using namespace rs;
using namespace rs::host;

extern "C" {

int rs_locate_multi_batch_dev(uint64_t k, uint64_t m, size_t sb, uint64_t n_stripes, uint32_t max_t,
                              const void *d_original, uint64_t orig_stride, const void *d_recovery,
                              uint64_t rec_stride, int32_t *d_count, int32_t *d_located, uint64_t located_stride,
                              uint8_t *d_present, uint64_t present_stride, uint64_t *d_counts, uint32_t flags,
                              rs_stream_t stream) {
  TraceScope ts;
  return guarded([&]() -> int {
    int st = check_scrub_args(k, m, sb, n_stripes, d_original, &orig_stride, d_recovery, &rec_stride, d_count);
    if (st || n_stripes == 0) return st;
    // the span argument needs a linear encode that reads every original
    if (flags != 0) return fail(RS_ERR_INVALID_ARGUMENT, "locate needs the corrected arithmetic (flags == 0)");
    if (sb % 64 == 0 && !align_nv({reinterpret_cast<uint64_t>(d_original), orig_stride}))
      return fail(RS_ERR_INVALID_ARGUMENT, "d_original / orig_stride must be 4-byte aligned");
    if (max_t == 0 || max_t > std::min<uint64_t>(m / 2, RS_LOCATE_MAX_T))
      return fail(RS_ERR_INVALID_ARGUMENT, "max_t outside [1, min(recovery_count / 2, RS_LOCATE_MAX_T)]");
    if (located_stride == 0) located_stride = max_t;
    if (located_stride < max_t) return fail(RS_ERR_INVALID_ARGUMENT, "located_stride below max_t");
    if (present_stride == 0) present_stride = k + m;
    if (present_stride < k + m) return fail(RS_ERR_INVALID_ARGUMENT, "present_stride below the shard count");
    int dev;
    if ((st = current_device(&dev))) return st;
    return mloc_slices(dev, k, m, sb, n_stripes, max_t, static_cast<const uint8_t *>(d_original), orig_stride,
                       static_cast<const uint8_t *>(d_recovery), rec_stride, d_count, d_located, located_stride,
                       d_present, present_stride, d_counts, static_cast<hipStream_t>(stream));
  });
}

const char *rs_locate_multi_kernel_name(uint64_t k, uint64_t m, size_t sb, uint32_t max_t) {
  thread_local std::string name;
  name = std::string(rs_encode_kernel_name(k, m, sb)) + "+verify_compare+locate_multi_t" + std::to_string(max_t);
  return name.c_str();
}

int rs_locate_multi_selftest(uint64_t k, uint64_t m, uint32_t max_t, int trials, uint64_t seed, uint64_t *mismatches) {
  return guarded([&]() -> int {
    if (k == 0) return fail(RS_ERR_INVALID_ARGUMENT, "original_count == 0");
    const int hr = use_high_rate(k, m);
    if (hr < 0) return fail(-hr, "unsupported shard count (root.zig:397-415)");
    if (max_t == 0 || max_t > std::min<uint64_t>(m / 2, RS_LOCATE_MAX_T))
      return fail(RS_ERR_INVALID_ARGUMENT, "max_t outside [1, min(recovery_count / 2, RS_LOCATE_MAX_T)]");
    SplitMix64 rnd(seed);
    uint64_t bad = 0;
    std::vector<uint16_t> cl;
    if (!coef_logs(k, m, cl)) bad++;  // a zero coefficient
    constexpr uint64_t P = 12;        // symbols per shard: room for max_t + 1 distinct positions
    static_assert(P > RS_LOCATE_MAX_T, "one symbol per corrupt shard");
    std::vector<uint16_t> data(k * P), par(m * P), S(m * P);
    std::vector<uint64_t> pick(k + m), at(P);
    std::vector<int32_t> got, want;
    for (int t = 0; bad == 0 && t < trials; t++) {
      for (auto &x : data) x = static_cast<uint16_t>(rnd());
      encode_columns(hr, k, m, P, data, par);
      // cases 0 .. max_t: that many corrupt shards with errors of full rank; max_t + 1: a pair
      // whose errors are proportional; max_t + 2: max_t + 1 shards, each with its own symbol
      for (uint32_t mode = 0; mode <= max_t + 2; mode++) {
        const bool pair = mode == max_t + 1;
        if (pair && m < 4) continue;  // two corrupt shards are beyond m / 2
        const uint64_t c = pair ? 2 : mode == max_t + 2 ? max_t + 1 : mode;
        std::vector<uint16_t> d2 = data, stored = par;
        for (uint64_t i = 0; i < k + m; i++) pick[i] = i;
        for (uint64_t i = 0; i < P; i++) at[i] = i;
        for (uint64_t i = 0; i < c; i++) {  // the heads of two partial Fisher-Yates shuffles
          std::swap(pick[i], pick[i + rnd() % (k + m - i)]);
          std::swap(at[i], at[i + rnd() % (P - i)]);
        }
        auto shard = [&](uint64_t i) { return pick[i] < k ? &d2[pick[i] * P] : &stored[(pick[i] - k) * P]; };
        if (pair) {  // err_b = alpha * err_a at every symbol: rank 1, two shards
          const uint16_t alpha_log = static_cast<uint16_t>(rnd() % kModulus);
          for (uint64_t q = 0; q < P; q++) {
            const uint16_t e = static_cast<uint16_t>(1 + rnd() % 65535);
            shard(0)[q] ^= e;
            shard(1)[q] ^= mul16(e, alpha_log);
          }
        } else {
          // shard i alone is wrong at symbol at[i] (so the errors have rank c); the symbols
          // that belong to no shard are wrong in each with probability 1/2, except in the last case
          for (uint64_t i = 0; i < c; i++) {
            shard(i)[at[i]] ^= static_cast<uint16_t>(1 + rnd() % 65535);
            for (uint64_t q = c; q < P && mode <= max_t; q++)
              if (rnd() & 1) shard(i)[at[q]] ^= static_cast<uint16_t>(1 + rnd() % 65535);
          }
        }
        want.assign(pick.begin(), pick.begin() + (mode <= max_t ? c : 0));
        std::sort(want.begin(), want.end());
        const int32_t want_count = mode <= max_t ? static_cast<int32_t>(c) : RS_LOCATE_UNLOCATED;
        encode_columns(hr, k, m, P, d2, S);
        for (uint64_t i = 0; i < m * P; i++) S[i] ^= stored[i];
        if (mloc_scalar(k, m, P, S.data(), cl, max_t, got) != want_count || got != want) bad++;
      }
    }
    if (mismatches) *mismatches = bad;
    return RS_OK;
  });
}

}  // extern "C"
