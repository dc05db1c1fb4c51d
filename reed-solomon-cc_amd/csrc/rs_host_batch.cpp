// rs_host_batch.cpp — host-resident batches (end to end through a persistent 2-slot
// H2D -> kernel -> D2H ring per device) and their multi-GPU split.
#include <cstdint>
#include <cstring>
#include <thread>
#include <utility>
#include <vector>

#include "rs_host.hpp"
#include "rs_host_ring.hpp"

using namespace rs;
using namespace rs::host;

extern "C" int rs_encode_batch_dev(uint64_t, uint64_t, size_t, uint64_t, const void *, uint64_t, void *, uint64_t,
                                   uint32_t, rs_stream_t);
extern "C" int rs_reconstruct_batch_dev(uint64_t, uint64_t, size_t, uint64_t, const uint8_t *, const void *, uint64_t,
                                        const void *, uint64_t, void *, uint64_t, uint32_t, rs_stream_t);

namespace {

// Copy `rows` rows of `row_bytes` between (possibly strided) buffers, always in the 2D form: for
// pinned host memory it moves contiguous slices faster than hipMemcpyAsync does (RS(10,4) 1 MiB
// encode 41.5 -> 52.3 GiB/s of data, 62 -> 79 GB/s over PCIe; c4 encode 44.6 -> 52.4;
// profiles/r06/e2e/copy2d/).
hipError_t copy_rows(void *dst, uint64_t dst_stride, const void *src, uint64_t src_stride, uint64_t row_bytes,
                     uint64_t rows, hipMemcpyKind kind, hipStream_t s) {
  if (rows == 0 || row_bytes == 0) return hipSuccess;
  return hipMemcpy2DAsync(dst, dst_stride, src, src_stride, row_bytes, rows, kind, s);
}

// Pageable host buffers go through the ring's own pinned staging (RS_AMD_HOST_STAGE, default
// on): host threads copy a slice's rows into it while the previous slice is on PCIe, and the
// device copies run from pinned memory in the 2D form; the runtime's own pageable path stages
// through a smaller buffer one copy at a time.
bool is_pinned(const void *p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeHost || a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged ||
         a.type == hipMemoryTypeUnified;
}

// Per-device staging ring of the host-batch calls: `slots` slices, each on its own
// stream (H2D -> kernel -> D2H in order; slices on different streams overlap both
// PCIe directions with the kernels). Buffers and streams persist across calls and
// grow on demand; the ring's mutex serialises host-batch calls on one device.
struct Pipeline {
  static constexpr int kMaxSlots = 8;  // the upper bound of RS_AMD_HOST_SLOTS (rs_env.hpp)
  std::mutex mu;
  int slots = 0;  // ring depth in use (RS_AMD_HOST_SLOTS, default 2)
  hipStream_t st[kMaxSlots] = {};
  void *buf[kMaxSlots][3] = {};
  uint64_t cap[3] = {};
  void *hst[kMaxSlots][3] = {};  // pinned host staging of pageable callers' slices
  uint64_t hcap[3] = {};
  int hslots = 0;
  int ensure_stage(const uint64_t bytes[3], int want) {
    bool grow = want > hslots;
    for (int j = 0; j < 3; j++) grow = grow || bytes[j] > hcap[j];
    if (!grow) return RS_OK;
    for (int i = 0; i < kMaxSlots; i++)
      for (int j = 0; j < 3; j++) {
        if (hst[i][j]) HIP_TRY(hipHostFree(hst[i][j]));
        hst[i][j] = nullptr;
      }
    hslots = 0;
    for (int j = 0; j < 3; j++) hcap[j] = std::max(hcap[j], bytes[j]);
    for (int i = 0; i < want; i++)
      for (int j = 0; j < 3; j++)
        if (hcap[j]) HIP_TRY(pinned_malloc(&hst[i][j], hcap[j]));
    hslots = want;
    return RS_OK;
  }
  int ensure(const uint64_t bytes[3], int want) {
    for (int i = 0; i < want; i++)
      if (!st[i]) HIP_TRY(hipStreamCreateWithFlags(&st[i], hipStreamNonBlocking));
    bool grow = want > slots;  // fewer slots wanted: the call uses the first `want`
    for (int j = 0; j < 3; j++) grow = grow || bytes[j] > cap[j];
    if (!grow) return RS_OK;
    for (int i = 0; i < kMaxSlots; i++)
      for (int j = 0; j < 3; j++) {
        if (buf[i][j]) HIP_TRY(hipFree(buf[i][j]));
        buf[i][j] = nullptr;
      }
    slots = 0;
    for (int j = 0; j < 3; j++) cap[j] = std::max(cap[j], bytes[j]);
    for (int i = 0; i < want; i++)
      for (int j = 0; j < 3; j++)
        if (cap[j]) HIP_TRY(dev_malloc(&buf[i][j], cap[j]));
    slots = std::max(slots, want);
    return RS_OK;
  }
  int finish() {
    for (int i = 0; i < slots; i++) HIP_TRY(hipStreamSynchronize(st[i]));
    return RS_OK;
  }
};
static_assert(env::kTable[env::HOST_SLOTS].hi == Pipeline::kMaxSlots, "RS_AMD_HOST_SLOTS is clamped to the ring's slots");

// Fault injection for the error-path test (the reference's checkAllAllocationFailures,
// tests.zig:131-156, in spirit): RS_AMD_INJECT_HOST_FAIL=i fails slice i of a host batch.
bool inject_host_failure(uint64_t slice) {
  const int i = env::num(env::INJECT_HOST_FAIL);
  return i != env::kAuto && static_cast<uint64_t>(i) == slice;
}

// process-lifetime rings (never freed: the HIP runtime reclaims them at exit)
std::mutex g_pipe_mu;
std::map<int, Pipeline *> g_pipes;

struct Pipelines {
  static Pipeline &of(int dev) {
    std::lock_guard<std::mutex> lk(g_pipe_mu);
    Pipeline *&p = g_pipes[dev];
    if (!p) p = new Pipeline();
    return *p;
  }
};

// What a host batch moves per slice of stripes. Ring buffer j holds rows[j] shard rows per
// stripe (originals, recovery, restored). `In`: shard rows [first, last) of buffer `buf` come
// from the caller's array at `host` (stripes `stride` bytes apart); `Out`: all of buffer `buf`
// goes back to the caller.
struct In {
  int buf;
  uint64_t first, last;
  const uint8_t *host;
  uint64_t stride;
};
struct Out {
  int buf;
  uint8_t *host;
  uint64_t stride;
};

// The slice loop of both host batches: n stripes in slices of S through the device's ring
// (RS_AMD_HOST_SLOTS slices in flight, read per call). Pinned RS(10,4) 1 MiB x 512 encode /
// reconstruct GiB/s: 1 slot 37.5 / 37.0, 2 slots 49.3 / 49.8, 3 slots 44.6 / 48.8,
// 6 x 64 MiB 46.4 / 46.2 (profiles/r01/e2e_shapes): two slices keep one H2D, one
// kernel and one D2H in flight; more streams only contend for the copy engines.
// kernel(cnt, bufs, stream) runs one slice on the slot's device buffers.
template <class K>
int run_ring(int dev, uint64_t n, uint64_t S, uint64_t sb, const uint64_t (&rows)[3], bool pinned,
             const std::vector<In> &in, const Out &out, K &&kernel) {
  const int slots = env::num(env::HOST_SLOTS);
  Pipeline &p = Pipelines::of(dev);
  std::lock_guard<std::mutex> lk(p.mu);
  const uint64_t bytes[3] = {S * rows[0] * sb, S * rows[1] * sb, S * rows[2] * sb};
  int st = p.ensure(bytes, slots);
  if (st) return st;
  const bool stage = env::on(env::HOST_STAGE) && !pinned;
  if (stage && (st = p.ensure_stage(bytes, slots))) return st;
  const uint64_t out_bytes = rows[out.buf] * sb;
  uint64_t pend_s0[Pipeline::kMaxSlots] = {}, pend_cnt[Pipeline::kMaxSlots] = {};
  // staged: a slot's previous slice is waited for and its output copied out before the slot's
  // staging buffers take the next slice
  auto take_out = [&](int slot) {
    if (!pend_cnt[slot]) return;
    host_copy({{out.host + pend_s0[slot] * out.stride, out.stride, static_cast<const uint8_t *>(p.hst[slot][out.buf]),
                out_bytes, out_bytes, pend_cnt[slot]}});
    pend_cnt[slot] = 0;
  };
  auto slices = [&]() -> int {
    for (uint64_t s0 = 0, i = 0; s0 < n; s0 += S, i++) {
      const int slot = static_cast<int>(i % static_cast<uint64_t>(slots));
      const uint64_t cnt = std::min(S, n - s0);
      hipStream_t q = p.st[slot];
      if (inject_host_failure(i)) return fail(RS_ERR_DEVICE, "injected host-batch failure");
      if (stage) {  // the rows into the slot's staging, in the device layout
        HIP_TRY(hipStreamSynchronize(q));
        take_out(slot);
        std::vector<CopyJob> jobs;
        for (const In &r : in)
          jobs.push_back({static_cast<uint8_t *>(p.hst[slot][r.buf]) + r.first * sb, rows[r.buf] * sb,
                          r.host + s0 * r.stride + r.first * sb, r.stride, (r.last - r.first) * sb, cnt});
        host_copy(jobs);
      }
      for (const In &r : in) {  // one copy per run of rows
        const uint8_t *src = stage ? static_cast<const uint8_t *>(p.hst[slot][r.buf]) : r.host + s0 * r.stride;
        HIP_TRY(copy_rows(static_cast<uint8_t *>(p.buf[slot][r.buf]) + r.first * sb, rows[r.buf] * sb,
                          src + r.first * sb, stage ? rows[r.buf] * sb : r.stride, (r.last - r.first) * sb, cnt,
                          hipMemcpyHostToDevice, q));
      }
      const int rc = kernel(cnt, p.buf[slot], q);
      if (rc) return rc;
      if (stage) {
        HIP_TRY(copy_rows(p.hst[slot][out.buf], out_bytes, p.buf[slot][out.buf], out_bytes, out_bytes, cnt,
                          hipMemcpyDeviceToHost, q));
        pend_s0[slot] = s0;
        pend_cnt[slot] = cnt;
      } else {
        HIP_TRY(copy_rows(out.host + s0 * out.stride, out.stride, p.buf[slot][out.buf], out_bytes, out_bytes, cnt,
                          hipMemcpyDeviceToHost, q));
      }
    }
    return RS_OK;
  };
  // every slot stream is drained before the call returns, after an error and before an
  // exception leaves too: no copy into the caller's buffers (or out of them) outlives the call
  int rc;
  try {
    rc = slices();
  } catch (...) {
    (void)p.finish();
    throw;
  }
  const int fin = p.finish();
  if (stage && fin == RS_OK)
    for (int slot = 0; slot < slots; slot++) take_out(slot);  // slices that completed, also before an error
  return rc ? rc : fin;
}

}  // namespace

void rs::host::release_host_rings() {
  std::lock_guard<std::mutex> lk(g_pipe_mu);
  for (auto &kv : g_pipes) {
    Pipeline &p = *kv.second;
    std::lock_guard<std::mutex> pk(p.mu);
    int cur = 0;
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(kv.first);
    for (int i = 0; i < Pipeline::kMaxSlots; i++)
      for (int j = 0; j < 3; j++) {
        if (p.buf[i][j]) (void)hipFree(p.buf[i][j]);
        p.buf[i][j] = nullptr;
      }
    p.slots = 0;
    for (int j = 0; j < 3; j++) p.cap[j] = 0;
    for (int i = 0; i < Pipeline::kMaxSlots; i++)
      for (int j = 0; j < 3; j++) {
        if (p.hst[i][j]) (void)hipHostFree(p.hst[i][j]);
        p.hst[i][j] = nullptr;
      }
    p.hslots = 0;
    for (int j = 0; j < 3; j++) p.hcap[j] = 0;
    (void)hipSetDevice(cur);
  }
}

extern "C" {

int rs_encode_batch_host(uint64_t k, uint64_t m, size_t sb, uint64_t n, const void *h_orig, uint64_t orig_stride,
                         void *h_rec, uint64_t rec_stride, uint32_t flags) {
  TraceScope ts;
  return guarded([&]() -> int {
    if (k == 0) return fail(RS_ERR_TOO_FEW_ORIGINAL_SHARDS, "original_count == 0");
    int st = check_codec(k, m, sb);
    if (st) return st;
    if (n == 0) return RS_OK;
    if (!h_orig || !h_rec) return fail(RS_ERR_INVALID_ARGUMENT, "NULL host pointer");
    if (orig_stride == 0) orig_stride = k * sb;
    if (rec_stride == 0) rec_stride = m * sb;
    int dev;
    if ((st = current_device(&dev))) return st;
    const uint64_t S =
        std::max<uint64_t>(1, std::min<uint64_t>(n, host_slice_bytes(env::num(env::HOST_SLICE_MB)) / (k * sb)));
    return run_ring(dev, n, S, sb, {k, m, 0}, is_pinned(h_orig) && is_pinned(h_rec),
                    {{0, 0, k, static_cast<const uint8_t *>(h_orig), orig_stride}},
                    {1, static_cast<uint8_t *>(h_rec), rec_stride}, [&](uint64_t cnt, void *const *b, hipStream_t q) {
                      return rs_encode_batch_dev(k, m, sb, cnt, b[0], 0, b[1], 0, flags, q);
                    });
  });
}

int rs_reconstruct_batch_host(uint64_t k, uint64_t m, size_t sb, uint64_t n, const uint8_t *present,
                              const void *h_orig, uint64_t orig_stride, const void *h_rec, uint64_t rec_stride,
                              void *h_out, uint64_t out_stride, uint32_t flags) {
  TraceScope ts;
  return guarded([&]() -> int {
    if (!present) return fail(RS_ERR_INVALID_ARGUMENT, "present == NULL");
    int st = check_codec(k, m, sb);
    if (st) return st;
    uint64_t e = 0, have = 0;
    for (uint64_t i = 0; i < k; i++) e += present[i] ? 0 : 1;
    for (uint64_t i = 0; i < k + m; i++) have += present[i] ? 1 : 0;
    if (have < k) return fail(RS_ERR_NOT_ENOUGH_SHARDS, "fewer than original_count shards present");
    if (e == 0 || n == 0) return RS_OK;
    if (!h_orig || !h_rec || !h_out) return fail(RS_ERR_INVALID_ARGUMENT, "NULL host pointer");
    if (orig_stride == 0) orig_stride = k * sb;
    if (rec_stride == 0) rec_stride = m * sb;
    if (out_stride == 0) out_stride = e * sb;
    int dev;
    if ((st = current_device(&dev))) return st;
    // only the present shards cross PCIe
    std::vector<In> in;
    for (const auto &r : present_runs(present, k))
      in.push_back({0, r.first, r.second, static_cast<const uint8_t *>(h_orig), orig_stride});
    for (const auto &r : present_runs(present + k, m))
      in.push_back({1, r.first, r.second, static_cast<const uint8_t *>(h_rec), rec_stride});
    std::vector<std::pair<uint64_t, uint64_t>> runs;
    for (const In &r : in) runs.emplace_back(r.first, r.last);
    const uint64_t S = reconstruct_slice_stripes(n, k * sb, sb, runs, env::num(env::HOST_SLICE_MB));
    return run_ring(dev, n, S, sb, {k, m, e}, is_pinned(h_orig) && is_pinned(h_rec) && is_pinned(h_out), in,
                    {2, static_cast<uint8_t *>(h_out), out_stride}, [&](uint64_t cnt, void *const *b, hipStream_t q) {
                      return rs_reconstruct_batch_dev(k, m, sb, cnt, present, b[0], 0, b[1], 0, b[2], 0, flags, q);
                    });
  });
}

}  // extern "C"

namespace {
// One worker thread per device over contiguous stripe ranges (sharding.stripe_range's
// partition); each worker selects its device and calls the single-device host batch.
template <class F>
int run_multi(uint64_t n, const int *devices, int n_devices, F &&one) {
  std::vector<int> devs;
  if (devices) {
    if (n_devices <= 0) return fail(RS_ERR_INVALID_ARGUMENT, "n_devices <= 0");
    devs.assign(devices, devices + n_devices);
  } else {
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0) return fail(RS_ERR_NO_DEVICE, "no HIP device");
    for (int d = 0; d < cnt; d++) devs.push_back(d);
  }
  const uint64_t D = devs.size();
  std::vector<int> status(D, RS_OK);
  std::vector<std::string> msg(D);
  std::vector<std::thread> th;
  th.reserve(D);
  for (uint64_t i = 0; i < D; i++) {
    const uint64_t b = n * i / D, e = n * (i + 1) / D;
    th.emplace_back([&, i, b, e] {
      if (hipSetDevice(devs[i]) != hipSuccess) {
        status[i] = RS_ERR_NO_DEVICE;
        msg[i] = "hipSetDevice(" + std::to_string(devs[i]) + ") failed";
        return;
      }
      status[i] = e > b ? one(b, e - b) : RS_OK;
      if (status[i]) msg[i] = rs_last_error();
    });
  }
  for (auto &t : th) t.join();
  for (uint64_t i = 0; i < D; i++)
    if (status[i]) return fail(status[i], "device " + std::to_string(devs[i]) + ": " + msg[i]);
  return RS_OK;
}
}  // namespace

extern "C" {

int rs_encode_batch_host_multi(uint64_t k, uint64_t m, size_t sb, uint64_t n, const void *h_orig, uint64_t orig_stride,
                               void *h_rec, uint64_t rec_stride, uint32_t flags, const int *devices, int n_devices) {
  TraceScope ts;
  return guarded([&]() -> int {
    if (orig_stride == 0) orig_stride = k * sb;
    if (rec_stride == 0) rec_stride = m * sb;
    return run_multi(n, devices, n_devices, [&](uint64_t s0, uint64_t cnt) {
      return rs_encode_batch_host(k, m, sb, cnt, static_cast<const uint8_t *>(h_orig) + s0 * orig_stride,
                                  orig_stride, static_cast<uint8_t *>(h_rec) + s0 * rec_stride, rec_stride, flags);
    });
  });
}

int rs_reconstruct_batch_host_multi(uint64_t k, uint64_t m, size_t sb, uint64_t n, const uint8_t *present,
                                    const void *h_orig, uint64_t orig_stride, const void *h_rec, uint64_t rec_stride,
                                    void *h_out, uint64_t out_stride, uint32_t flags, const int *devices,
                                    int n_devices) {
  TraceScope ts;
  return guarded([&]() -> int {
    if (!present) return fail(RS_ERR_INVALID_ARGUMENT, "present == NULL");
    uint64_t e = 0;
    for (uint64_t i = 0; i < k; i++) e += present[i] ? 0 : 1;
    if (orig_stride == 0) orig_stride = k * sb;
    if (rec_stride == 0) rec_stride = m * sb;
    if (out_stride == 0) out_stride = e * sb;
    return run_multi(n, devices, n_devices, [&](uint64_t s0, uint64_t cnt) {
      return rs_reconstruct_batch_host(k, m, sb, cnt, present, static_cast<const uint8_t *>(h_orig) + s0 * orig_stride,
                                       orig_stride, static_cast<const uint8_t *>(h_rec) + s0 * rec_stride, rec_stride,
                                       static_cast<uint8_t *>(h_out) + s0 * out_stride, out_stride, flags);
    });
  });
}

}  // extern "C"
