"""No reconstruct path depends on, or writes, the bytes in the slots of missing shards
(include/reedsol.h): one case per reconstruct kernel family and entry point, through the
checker of tests/slot_contract.py. Every missing slot of d_original and d_recovery holds a
poison that differs from the truth in every byte (never zeros: an erased input XORed into an
output with any coefficient is invisible when it is zero); the call runs under two such
poisons, on strided buffers, into a guard-filled output. Restored slots must be the expected
bytes under both, the two outputs identical, the inputs unchanged and every output byte outside
the documented rows untouched. Each case also asserts the kernels it launched
(rs_last_kernels), so that it keeps testing the family it names.

Expected values: the erased data where the code decodes (flags 0 / 2); the oracle's literal
reconstruct of the clean shards under D1 and for D2-dropping codes; low-rate codes: the erased
data, parity from the GPU encode (checked against the oracle in tests/test_lowrate.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

from slot_contract import check_reconstruct

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import oracle as O  # noqa: E402
from rs_amd import reedsol_amd as R  # noqa: E402  (after torch: share its HIP runtime)

DEV = torch.device("cuda:0")
KNOBS = ("RS_AMD_DECODE", "RS_AMD_JIT", "RS_AMD_JIT_SYNC", "RS_AMD_FDEC", "RS_AMD_FFT", "RS_AMD_NET_SHARED",
         "RS_AMD_LOW_BLOCK", "RS_AMD_LOW_TRIM", "RS_AMD_PATTERNS", "RS_AMD_HOST_SLICE_MB", "RS_AMD_NV",
         "RS_AMD_NET_SMALL", "RS_AMD_NET_ASYNC_BLOCKS", "RS_AMD_PDEC", "RS_AMD_PDEC_AFTER", "RS_AMD_PDEC_MAX")


def set_knobs(monkeypatch, env):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    for name, val in env.items():
        monkeypatch.setenv(name, val)


@functools.lru_cache(maxsize=None)
def truth(k, m, sb, n, flags=0):
    """The true shards [n, k+m, sb] of a code and shape, computed once and read-only. High rate:
    parity from the oracle; low rate: from the GPU encode."""
    rng = np.random.default_rng(k * 1009 + m * 31 + sb + n + flags)
    data = rng.integers(0, 256, (n, k, sb), dtype=np.uint8)
    if R.use_high_rate(k, m):
        par = O.encode_batch(k, m, data, quirks=flags, threads=4)
    else:
        p = torch.zeros((n, m, sb), dtype=torch.uint8, device=DEV)
        R.encode_batch_dev(k, m, torch.from_numpy(data).to(DEV), p)
        torch.cuda.synchronize()
        par = p.cpu().numpy()
    shards = np.concatenate([data, par], axis=1)
    shards.setflags(write=False)
    return shards


def literal(k, m, flags):
    """The reference's decode as written, no decoder of the data: D1, or a code whose D2
    schedule drops the last full chunk (root.zig:151)."""
    c = 1 << (m - 1).bit_length()
    return bool(flags & 1) or bool(flags & 2 and k > c and k % c == 0)


def expected_rows(k, m, flags, present_row, stripe):
    """The restored shards of one stripe [k+m, sb] under one row of flags, ascending."""
    lost = [i for i in range(k) if not present_row[i]]
    if not lost:
        return stripe[:0]
    if literal(k, m, flags) and R.use_high_rate(k, m):
        return O.reconstruct_batch(k, m, present_row, stripe[None], quirks=flags)[0]
    return stripe[lost]


def dev_run(call, ran):
    """run() of check_reconstruct on the GPU: upload, call(orig, rec, out) on 2-D device tensors
    (row = stripe, row length = stride), note the kernels launched, synchronise, download."""
    def run(orig, rec, out):
        o, r, t = (torch.from_numpy(a).to(DEV) for a in (orig, rec, out))
        call(o, r, t)
        ran.append(R.last_kernels())
        torch.cuda.synchronize()
        return o.cpu().numpy(), r.cpu().numpy(), t.cpu().numpy()
    return run


def ptr(t):
    return C.c_void_p(t.data_ptr())


def launched(ran, want, forbid=()):
    """Every call launched a kernel of each wanted prefix and none of a forbidden one."""
    assert ran, "no call was made"
    for kernels in ran:
        for w in want:
            alts = w if isinstance(w, tuple) else (w,)
            assert any(x.startswith(alts) for x in kernels), (w, ran)
        for f in forbid:
            assert not any(x.startswith(f) for x in kernels), (f, ran)


# ------------------------------------------------------------ rs_reconstruct_batch_dev
def every(step, count, start=0):
    return list(range(start, start + step * count, step))


def case(id, k, m, sb, lost, lost_rec, want, env=None, n=3, flags=0, warm=False, forbid=(), pads=(256, 128, 64)):
    return pytest.param(dict(k=k, m=m, sb=sb, n=n, flags=flags, lost=sorted(lost), lost_rec=sorted(lost_rec),
                             want=want, forbid=forbid, env=env or {}, warm=warm, pads=pads), id=id)


SYN_TABLES = {"RS_AMD_DECODE": "syndrome", "RS_AMD_JIT": "0", "RS_AMD_FDEC": "0"}
FUSED = {"RS_AMD_FDEC": "1", "RS_AMD_DECODE": "syndrome"}
LOW_TAIL = sorted(set(range(100)) - {11, 50, 93})  # 97 of RS(100,600)'s originals lost
# Every pattern loses originals and recovery rows, the first recovery row and a row next to a used
# one among them. "= k": exactly k shards present.
BATCH_CASES = [
    case("decode_reg", 10, 4, 192, [1, 4], [0, 2], ["decode_reg_w16"], {"RS_AMD_DECODE": "fft"}),  # = k
    case("decode_matrix", 10, 4, 192, [0, 5, 9], [1], ["decode_matrix_e3"],
         {"RS_AMD_DECODE": "matrix", "RS_AMD_JIT": "0"}),  # = k
    case("decode_mtile", 70, 40, 1024, every(3, 20, 1), every(2, 20), ["decode_mtile16"],
         {"RS_AMD_DECODE": "matrix", "RS_AMD_JIT": "0"}),  # = k
    case("decode_generic", 100, 20, 192, [0, 31, 32, 63, 64, 95, 96, 99], [0, 2, 3, 7, 19], ["decode_generic"],
         {"RS_AMD_DECODE": "fft"}),
    case("net_reconstruct-4k", 10, 4, 4096, [1, 4], [0, 2], ["rs_net_reconstruct_i10_o2"],
         {"RS_AMD_DECODE": "net"}),  # = k
    case("net_reconstruct-1k-ragged", 10, 4, 1024, [0, 8, 9], [0], ["rs_net_reconstruct_i10_o3"],
         {"RS_AMD_DECODE": "net"}, n=5),  # = k; a wave unit spans 4 stripes: 5 is ragged
    case("net_shared", 16, 16, 8192, every(1, 12), [0, 2, 5, 15], ["rs_net_reconstruct_i16_o12"],
         {"RS_AMD_NET_SHARED": "1", "RS_AMD_JIT_SYNC": "1", "RS_AMD_FFT": "0"}),  # = k
    case("syndrome-tables-rs20_16", 20, 16, 1024, every(2, 10), [0, 2, 3, 9, 15], ["encode_", "decode_mtile16"],
         SYN_TABLES),
    case("syndrome-tables-rs70_33", 70, 33, 1024, every(3, 20, 2), every(2, 13), ["encode_", "decode_mtile16"],
         SYN_TABLES),  # = k
    # the syndromes run on the FFT kernel for shards of whole 4 KiB units; at 2 KiB the table
    # encode feeds the syndrome network's small-shard variant (two stripes per wave unit)
    case("syndrome-fft_encode+net_syndrome", 200, 55, 4096, every(6, 32, 3), [0, 2, 3, 30, 54],
         ["rs_fft_encode_k200_m55", "rs_net_syndrome_i32_o32"], {"RS_AMD_JIT_SYNC": "1", "RS_AMD_FDEC": "0"}),
    case("syndrome-table-encode+net_syndrome-2k", 200, 55, 2048, every(6, 32, 3), [0, 2, 3, 30, 54],
         ["encode_ws64", "rs_net_syndrome_i32_o32"], {"RS_AMD_JIT_SYNC": "1", "RS_AMD_FDEC": "0"}),
    case("fft_decode-rs33_17", 33, 17, 2048, [0, 31, 32], [0, 2, 16], ["rs_fft_decode_k33_m17"], FUSED),
    case("fft_decode-rs100_20", 100, 20, 2048, [5, 64, 96, 98, 99], [0, 1, 3, 19], ["rs_fft_decode_k100_m20"], FUSED),
    case("pattern-compiled-rs16_16", 16, 16, 4096, every(1, 12, 2), [0, 2, 5, 15],
         [("rs_fft_pdecode_k16_m16", "rs_net_reconstruct_i16", "rs_fft_inverse")], warm=True),  # = k
    case("pattern-compiled-rs33_17", 33, 17, 4096, every(2, 15, 4), [0, 2],
         [("rs_fft_pdecode_k33_m17", "rs_net_reconstruct_i33", "rs_fft_inverse")], warm=True),  # = k
    # without background networks the warmed pattern's steady state is the fused kernel with the
    # pattern compiled in (the two cases above settle on the pattern's direct network)
    case("pattern-compiled-fused-rs33_17", 33, 17, 4096, every(2, 14, 3) + [32], [0, 2], ["rs_fft_pdecode_k33_m17"],
         {"RS_AMD_NET_ASYNC_BLOCKS": "0"}, warm=True),  # = k
    case("fft_inverse", 32, 32, 1024, every(1, 32), [], ["rs_fft_inverse_k32_m32"]),  # = k; 3 stripes: ragged
    case("shard-tail", 10, 4, 70, [3, 9], [0, 2], ["k_tail_pack"], pads=(256, 128, 64)),  # = k
    case("literal-d1", 10, 4, 192, [1, 4], [0], ["decode_"], flags=1),
    case("literal-d1d2", 10, 4, 192, [0, 9], [0, 2], ["decode_"], flags=3),  # = k
    case("literal-d2-dropping", 8, 4, 192, [2, 7], [0], ["decode_"], flags=2),
    case("low-net_reconstruct_low", 3, 5, 4096, [0, 2], [0, 2, 3], ["rs_net_reconstruct_low_i3_o2"],
         {"RS_AMD_JIT_SYNC": "1"}),  # = k
    case("low-decode_reg", 3, 5, 4096, [0, 2], [0, 2, 3], ["decode_reg_w16"], {"RS_AMD_JIT": "0"}),  # = k
    case("low-decode_generic", 40, 100, 192, every(4, 10), every(1, 20) + [22, 99], ["decode_generic"],
         {"RS_AMD_JIT": "0"}),
    # RS(100,600), the loss shapes of test_low_rate_block_form: "tail" loses the first 500
    # recovery rows, "spread" the first 80, so the rows read are picked among the present ones
    case("low-blocks-tail", 100, 600, 2048, LOW_TAIL, every(1, 500), ["low_blocks"],
         {"RS_AMD_LOW_BLOCK": "1", "RS_AMD_JIT": "0"}),
    case("low-blocks-spread", 100, 600, 2048, LOW_TAIL, every(1, 80), ["low_blocks"],
         {"RS_AMD_LOW_BLOCK": "1", "RS_AMD_JIT": "0"}),
    case("low-blocks-off-tail", 100, 600, 2048, LOW_TAIL, every(1, 500), ["decode_generic"],
         {"RS_AMD_LOW_BLOCK": "0", "RS_AMD_JIT": "0"}, forbid=["low_blocks"]),
    case("low-blocks-off-spread", 100, 600, 2048, LOW_TAIL, every(1, 80), ["decode_generic"],
         {"RS_AMD_LOW_BLOCK": "0", "RS_AMD_JIT": "0"}, forbid=["low_blocks"]),
    case("low-trim-off-tail", 100, 600, 2048, LOW_TAIL, every(1, 500), ["decode_generic"],
         {"RS_AMD_LOW_TRIM": "0", "RS_AMD_JIT": "0"}, forbid=["low_blocks"]),
    case("low-trim-off-spread", 100, 600, 2048, LOW_TAIL, every(1, 80), ["decode_generic"],
         {"RS_AMD_LOW_TRIM": "0", "RS_AMD_JIT": "0"}, forbid=["low_blocks"]),
]


def batch_check(monkeypatch, c):
    set_knobs(monkeypatch, c["env"])
    k, m, sb, n, flags = c["k"], c["m"], c["sb"], c["n"], c["flags"]
    shards = truth(k, m, sb, n, flags)
    present = np.ones(k + m, np.uint8)
    present[c["lost"]] = 0
    present[np.array(c["lost_rec"], dtype=int) + k] = 0
    assert c["lost"] and int(present.sum()) >= k
    if literal(k, m, flags):
        expected = O.reconstruct_batch(k, m, present, shards, quirks=flags)
    else:
        expected = shards[:, c["lost"]]
    if c["warm"]:
        R.reconstruct_warm(k, m, sb, present, flags)
    ran = []

    def call(o, r, t):
        st = R.lib().rs_reconstruct_batch_dev(k, m, sb, n, C.c_void_p(present.ctypes.data), ptr(o), o.stride(0),
                                              ptr(r), r.stride(0), ptr(t), t.stride(0), flags, None)
        assert st == 0, R.lib().rs_last_error()

    try:
        check_reconstruct(dev_run(call, ran), k, m, shards, present, expected, pads=c["pads"])
    finally:
        print(f"\nFAMILY batch_dev {k},{m} sb {sb} flags {flags} {c['env']}: {ran}")
    launched(ran, c["want"], c["forbid"])


@pytest.mark.parametrize("c", BATCH_CASES)
def test_batch_dev(monkeypatch, c):
    batch_check(monkeypatch, c)


def test_syndrome_pattern_across_unit_sizes(monkeypatch):
    """One pattern of the syndrome path used with 4 KiB shards and then with 2 KiB shards, no
    e x e network (RS_AMD_NET_ASYNC_BLOCKS=0): the first runs the FFT syndromes and the generic
    solve, which need whole 4 KiB units; the second must get a plan of its own on the table
    kernels (the plan cache keys on the unit form), not the first one's."""
    env = {"RS_AMD_FDEC": "0", "RS_AMD_NET_ASYNC_BLOCKS": "0"}
    lost, lost_rec = every(6, 32, 2), [0, 2, 3, 30, 54]
    for sb, want in ((4096, ["rs_fft_encode_k200_m55", "rs_psyn_solve"]), (2048, ["encode_ws64", "decode_mtile16"])):
        batch_check(monkeypatch, case("", 200, 55, sb, lost, lost_rec, want, env).values[0])


# ------------------------------------------------------------ rs_reconstruct_batch_dev_patterns
def stripe_patterns(k, m, max_e):
    """present [7, k+m] and the expected status per stripe: nothing lost; more originals lost
    than max_e (14) where the code allows it; too few shards (2); two neighbours whose patterns
    are complements of each other on the first originals and recovery rows; exactly k present;
    one original and two recovery rows lost."""
    p = np.ones((7, k + m), np.uint8)
    status = [0] * 7
    if max_e + 1 <= min(k, m):  # e_s = max_e + 1 originals (the last ones), the first recovery row if spare
        p[1, k - (max_e + 1):k] = 0
        if m - (max_e + 1) >= 1:
            p[1, k] = 0
        status[1] = 14
    else:
        p[1, [0, k - 1]] = 0
        p[1, [k, k + m - 1]] = 0
    gone = [k] + list(range(k - 1, -1, -1)) + list(range(k + 1, k + m))  # NotEnoughShards: m + 1 shards lost
    p[2, gone[:m + 1]] = 0
    status[2] = 2
    span = min(4, k, 2 * max_e)
    even, odd = list(range(0, span, 2)), list(range(1, span, 2))
    p[3, even] = 0
    p[3, k + 1] = 0
    p[4, odd] = 0
    p[4, [k, k + 2]] = 0
    e5 = min(max_e, m, k)
    p[5, np.linspace(0, k - 1, e5).round().astype(int)] = 0
    e5 = int((p[5, :k] == 0).sum())
    p[5, k:k + m - e5] = 0  # exactly k present: the m - e5 leading recovery rows lost
    p[6, k - 1] = 0
    p[6, [k, k + 2]] = 0
    for s in range(7):
        have, e = int(p[s].sum()), int((p[s, :k] == 0).sum())
        assert status[s] == (2 if have < k else 14 if e > max_e else 0), (s, have, e)
    assert int(p[5].sum()) == k
    return p, status


def pcase(id, k, m, sb, max_e, path, want, env=None, flags=0):
    return pytest.param(dict(k=k, m=m, sb=sb, max_e=max_e, path=path, want=want, flags=flags,
                             env=dict({"RS_AMD_JIT_SYNC": "1"}, **(env or {}))), id=id)


PATTERN_CASES = [
    pcase("psyn_k10_m4", 10, 4, 4096, 2, "psyn_k10_m4", ["k_psyn_plan", "rs_psyn_reconstruct_k10_m4"]),
    pcase("fft_decode-rs16_16-max_e16", 16, 16, 4096, 16, "fft_decode", ["k_fdec_block", "rs_fft_decode_k16_m16"]),
    pcase("fft_decode-rs16_16-max_e12", 16, 16, 4096, 12, "fft_decode", ["k_fdec_block", "rs_fft_decode_k16_m16"]),
    pcase("fft_syndromes+psyn_solve", 200, 55, 8192, 8, "fft_syndromes+psyn_solve",
          ["k_wps_plan", "rs_fft_encode_k200_m55", "rs_psyn_solve"]),
    pcase("pattern_matrix", 5, 5, 320, 3, "pattern_matrix", ["k_pattern_images", "decode_matrix_e3"],
          {"RS_AMD_PATTERNS": "matrix"}),
    pcase("pattern_fft-d1", 10, 4, 192, 2, "pattern_fft", ["k_pattern_tables", "decode_reg_w16"], flags=1),
    pcase("pattern_fft-d2-dropping", 8, 4, 192, 2, "pattern_fft", ["k_pattern_tables", "decode_reg_w16"], flags=2),
    pcase("pattern_fft_low", 3, 5, 192, 2, "pattern_fft_low", ["k_pattern_tables", "decode_reg_w16"]),
]


@pytest.mark.parametrize("c", PATTERN_CASES)
def test_batch_dev_patterns(monkeypatch, c):
    set_knobs(monkeypatch, c["env"])
    k, m, sb, max_e, flags, n = c["k"], c["m"], c["sb"], c["max_e"], c["flags"], 7
    assert R.patterns_kernel_name(k, m, sb, max_e, flags) == c["path"]
    shards = truth(k, m, sb, n, flags)
    present, want_status = stripe_patterns(k, m, max_e)
    expected = [expected_rows(k, m, flags, present[s], shards[s])[:max_e] if want_status[s] != 2 else shards[s, :0]
                for s in range(n)]
    rows = np.random.default_rng(k + m).integers(1, 256, (n, k + m + 9), dtype=np.uint8)  # row stride > k + m,
    rows[:, :k + m] = present                                                            # the bytes past it nonzero
    d_present = torch.from_numpy(rows).to(DEV)
    ran, statuses = [], []

    def call(o, r, t):
        status = torch.full((n + 1,), -1, dtype=torch.int32, device=DEV)
        st = R.lib().rs_reconstruct_batch_dev_patterns(k, m, sb, n, ptr(d_present), d_present.stride(0), max_e, ptr(o),
                                                       o.stride(0), ptr(r), r.stride(0), ptr(t), t.stride(0),
                                                       ptr(status), flags, None)
        assert st == 0, R.lib().rs_last_error()
        statuses.append(status)

    try:
        check_reconstruct(dev_run(call, ran), k, m, shards, present, expected, max_e=max_e)
    finally:
        print(f"\nFAMILY patterns {k},{m} sb {sb} max_e {max_e} flags {flags} {c['path']}: {ran}")
    for status in statuses:
        assert status.cpu().tolist() == want_status + [-1]
    assert (d_present.cpu().numpy() == rows).all()
    launched(ran, c["want"])


# ------------------------------------------------------------ host batches
HOST = dict(k=10, m=4, sb=65536, n=9, lost=[2, 7], lost_rec=[0, 2])  # = k present


def host_run(fn, pinned, extra=()):
    """run() of check_reconstruct for the host-batch entry points: the arrays themselves
    (pageable) or pinned copies of them go in; what they hold afterwards comes back."""
    k, m, sb, n = HOST["k"], HOST["m"], HOST["sb"], HOST["n"]
    present = np.ones(k + m, np.uint8)
    present[HOST["lost"]] = 0
    present[[k + r for r in HOST["lost_rec"]]] = 0

    def run(orig, rec, out):
        o, r, t = (torch.from_numpy(a) for a in (orig, rec, out))
        if pinned:
            o, r, t = o.pin_memory(), r.pin_memory(), t.pin_memory()
        st = fn(k, m, sb, n, C.c_void_p(present.ctypes.data), ptr(o), o.stride(0), ptr(r), r.stride(0), ptr(t),
                t.stride(0), 0, *extra)
        assert st == 0, R.lib().rs_last_error()
        return o.numpy().copy(), r.numpy().copy(), t.numpy().copy()
    return present, run


@pytest.mark.parametrize("pinned", [True, False], ids=["pinned", "pageable"])
@pytest.mark.parametrize("entry", ["host", "host_multi"])
def test_batch_host(monkeypatch, entry, pinned):
    """The host ring copies only the runs of present rows; with 1 MiB slices (one stripe each)
    nine slices reuse both ring slots, whose device rows of missing shards hold what earlier
    slices and calls left there. The missing host rows are poisoned, differently per stripe, and
    the host inputs must come back unchanged."""
    set_knobs(monkeypatch, {"RS_AMD_HOST_SLICE_MB": "1"})
    k, m, sb, n = HOST["k"], HOST["m"], HOST["sb"], HOST["n"]
    shards = truth(k, m, sb, n)
    if entry == "host":
        present, run = host_run(R.lib().rs_reconstruct_batch_host, pinned)
    else:
        present, run = host_run(R.lib().rs_reconstruct_batch_host_multi, pinned, ((C.c_int * 2)(0, 0), 2))
    name = R.reconstruct_kernel_name(k, m, sb, present)  # launched on worker threads: the planned name
    assert name == "net_reconstruct_i10_o2", name
    check_reconstruct(run, k, m, shards, present, shards[:, HOST["lost"]], pads=(4096, 1024, 512))


# ------------------------------------------------------------ one-shot decode and Decoder
def c_decode(k, m, sb, orig, rec):
    """rs_decode through the C ABI: lists of bytes or None -> the k restored originals."""
    keep = [None if b is None else C.create_string_buffer(b, sb) for b in list(orig) + list(rec)]
    outs = [C.create_string_buffer(sb) for _ in range(k)]
    arr = lambda bufs: (C.c_void_p * len(bufs))(*[None if b is None else C.addressof(b) for b in bufs])  # noqa: E731
    st = R.lib().rs_decode(k, m, sb, arr(keep[:k]), arr(keep[k:]), arr(outs))
    assert st == 0, R.lib().rs_last_error()
    return [b.raw for b in outs]


@pytest.mark.parametrize("entry", ["rs_decode", "Decoder"])
@pytest.mark.parametrize("k,m", [(5, 5), (3, 5)], ids=["rs5_5", "rs3_5-low"])
def test_one_shot_after_decoys(entry, k, m):
    """rs_decode and the Decoder object leave the absent slots of their pooled staging
    unfilled. Every decodable mask that loses an original, each after two decodes of an
    unrelated stripe of the same size (one losing original 0, one original 1), after which every
    slot of the staging holds the decoy's bytes, not an earlier call's copy of the real shard."""
    sb = 64
    decode = (lambda o, r: c_decode(k, m, sb, o, r)) if entry == "rs_decode" else (lambda o, r: R.decode(k, m, o, r))
    rng = np.random.default_rng(k * 10 + m)
    orig = [rng.integers(0, 256, sb, dtype=np.uint8).tobytes() for _ in range(k)]
    decoy = [rng.integers(0, 256, sb, dtype=np.uint8).tobytes() for _ in range(k)]
    rec, decoy_rec = R.encode(k, m, orig), R.encode(k, m, decoy)
    kernels, done = set(), 0
    for mask in range(1 << (k + m)):
        if bin(mask).count("1") > m or not mask & ((1 << k) - 1):
            continue
        for lose in (0, 1):
            assert decode([None if i == lose else decoy[i] for i in range(k)], decoy_rec) == decoy, (mask, lose)
        o = [None if mask >> i & 1 else orig[i] for i in range(k)]
        r = [None if mask >> (k + i) & 1 else rec[i] for i in range(m)]
        assert decode(o, r) == orig, mask
        kernels.update(R.last_kernels())
        done += 1
    assert done == sum(1 for x in range(1 << (k + m)) if bin(x).count("1") <= m and x & ((1 << k) - 1))
    print(f"\nFAMILY one-shot {entry} {k},{m}: {sorted(kernels)}")
    assert kernels and all(x.startswith(("decode_", "k_tail_pack")) for x in kernels), kernels
