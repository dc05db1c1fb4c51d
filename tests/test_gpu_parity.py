"""GPU parity: the HIP kernels (through the C ABI) against the CPU oracle and
the reference's golden vectors. Bit-exact everywhere (integer/byte work).

Sizes: the oracle runs every small case in full; at BASELINE sizes
(RS(10,4) 1 MiB, RS(200,55) 256 KiB) parity is checked by size-independent
properties — encode -> erase -> reconstruct round trips — plus oracle
comparison on randomly sampled 64-byte columns (column independence,
SURVEY.md §A.6, itself pinned by tests/test_oracle_golden.py)."""
import os

import numpy as np
import pytest

from helpers import digest, iota_input, load, splitmix_bytes, survey_input

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from rs_amd import reedsol_amd as R  # noqa: E402  (after torch: share its HIP runtime)

DEV = torch.device("cuda:0")


def to_dev(a: np.ndarray):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def gpu_encode(k, m, data: np.ndarray, flags=0):
    """data [n, k, sb] -> parity [n, m, sb] through rs_encode_batch_dev."""
    d = to_dev(data)
    p = torch.zeros((data.shape[0], m, data.shape[2]), dtype=torch.uint8, device=DEV)
    R.encode_batch_dev(k, m, d, p, flags)
    torch.cuda.synchronize()
    return p.cpu().numpy()


def gpu_reconstruct(k, m, present, data: np.ndarray, parity: np.ndarray, flags=0):
    n, _, sb = data.shape
    e = int(k - np.sum(present[:k]))
    o = to_dev(data)
    r = to_dev(parity)
    out = torch.zeros((n, max(e, 1), sb), dtype=torch.uint8, device=DEV)
    R.reconstruct_batch_dev(k, m, present, o, r, out, flags)
    torch.cuda.synchronize()
    return out.cpu().numpy()[:, :e]


@pytest.fixture(params=["4", "2", "1"])
def nv(request, monkeypatch):
    monkeypatch.setenv("RS_AMD_NV", request.param)
    return int(request.param)


@pytest.fixture(params=["1", "0"])
def jit(request, monkeypatch):
    """RS_AMD_JIT: bit-sliced network kernels (hipRTC, rs_jit.hpp) on / off (table kernels)."""
    monkeypatch.setenv("RS_AMD_JIT", request.param)
    return request.param


@pytest.fixture(params=["fft", "matrix", "auto"])
def decode_mode(request, monkeypatch):
    """RS_AMD_DECODE: FFT kernels (root.zig:268-335 as written) or the e x k matrix kernel."""
    monkeypatch.setenv("RS_AMD_DECODE", request.param)
    return request.param


# ------------------------------------------------------------ golden vectors
@pytest.mark.parametrize("flags", [0, 3])
def test_mul_kats(flags):
    """Generic.zig:402-455 through the device mulScalar shim."""
    for c in load("engine_kats.json")["mul"]:
        buf = bytearray([c["lo"]] * 32 + [c["hi"]] * 32)
        R.engine_mul_scalar(buf, c["log_m"], flags)
        assert list(buf[:32]) == [c["expected_lo"]] * 32
        assert list(buf[32:]) == [c["expected_hi"]] * 32


def test_encode_golden_rs16_16():
    """tests.zig:104-129 + encode_data.zon, through the one-shot host API."""
    fx = load("rs16_16_encode.json")
    data = iota_input(16)
    rec = R.encode(16, 16, [bytes(r) for r in data])
    assert [list(r) for r in rec] == fx["parity"]


@pytest.mark.parametrize("km", ["4,2", "10,4", "16,16", "32,32", "200,55"])
@pytest.mark.parametrize("mode", ["corrected", "ref_literal"])
def test_parity_digests(km, mode):
    d = load("survey_digests.json")
    k, m = map(int, km.split(","))
    par = gpu_encode(k, m, survey_input(k)[None], 0 if mode == "corrected" else 3)
    assert digest(par[0].tobytes()) == d["parity"][km][mode]


def test_exhaustive_rs5_5_roundtrip():
    """tests.zig:61-102: all 2^10 presence masks, one-shot host API."""
    k = m = 5
    orig = [bytes(r) for r in iota_input(k)]
    rec = R.encode(k, m, orig)
    ok = 0
    for mask in range(1 << (k + m)):
        o = [None if mask >> i & 1 else orig[i] for i in range(k)]
        r = [None if mask >> (k + i) & 1 else rec[i] for i in range(m)]
        if bin(mask).count("1") <= k:
            assert R.decode(k, m, o, r) == orig, mask
            ok += 1
        else:
            with pytest.raises(R.NotEnoughShards):
                R.decode(k, m, o, r)
    assert ok == 638


# ------------------------------------------------------------ engine seam
@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("case", [
    # (shard_count, pos, size, trunc, skew_delta)
    (4, 0, 4, 4, 4), (4, 0, 4, 3, 8), (8, 4, 4, 2, 12), (16, 0, 16, 14, 0), (16, 0, 16, 16, 0),
    (8, 0, 8, 8, 0), (8, 0, 8, 5, 16), (2, 0, 2, 2, 2), (32, 0, 32, 20, 0), (64, 0, 64, 64, 64),
    (512, 0, 512, 456, 0), (6, 2, 4, 4, 300), (2, 0, 2, 1, 1000),
    # the phased column walk (rs_kernels.hip xform_ph): a lone radix-2 phase (128), two
    # and three phases, truncation inside and at the phase blocks, an offset window
    (128, 0, 128, 100, 0), (1024, 0, 1024, 1000, 5), (2048, 0, 2048, 2048, 0),
    (4096, 0, 4096, 3000, 0), (8192, 0, 8192, 5000, 7), (8192, 0, 8192, 64, 0), (260, 4, 256, 200, 3),
])
def test_engine_fft_ifft_vs_oracle(oracle, flags, case):
    count, pos, size, trunc, sd = case
    rng = np.random.default_rng(count * 31 + sd)
    for sb in (64, 192):
        shards = rng.integers(0, 256, (count, sb), dtype=np.uint8)
        for inverse in (False, True):
            g = bytearray(shards.tobytes())
            R.engine_fft(g, count, sb, pos, size, trunc, sd, flags, inverse)
            o = shards.copy()
            (oracle.ifft if inverse else oracle.fft)(o, pos, size, trunc, sd, flags)
            assert bytes(g) == o.tobytes(), (case, sb, inverse)


def test_engine_mul_scalar_random(oracle):
    rng = np.random.default_rng(5)
    x = rng.integers(0, 256, 64 * 33, dtype=np.uint8)
    for lm in (0, 1, 257, 0x7777, 0xABCD, 65534, 65535):
        for flags in (0, 1):
            g = bytearray(x.tobytes())
            R.engine_mul_scalar(g, lm, flags)
            o = x.copy()
            oracle.mul_scalar(o, lm, flags)
            assert bytes(g) == o.tobytes(), (lm, flags)


# ------------------------------------------------------------ codec vs oracle
KM_SMALL = [(1, 1), (2, 1), (4, 2), (3, 4), (5, 5), (10, 4), (8, 4), (12, 4), (6, 3), (9, 8), (16, 16),
            (17, 16), (20, 16), (16, 8), (30, 2), (64, 64), (100, 20), (200, 55), (33, 32), (65, 33), (70, 60)]


@pytest.mark.parametrize("k,m", KM_SMALL)
@pytest.mark.parametrize("flags", [0, 3])
@pytest.mark.parametrize("sb", [320, 4096])  # 4096: whole 4 KiB waves -> network / contiguous layout, ws64 path
def test_encode_vs_oracle(oracle, nv, jit, k, m, flags, sb):
    rng = np.random.default_rng(k * 7919 + m * 31 + flags)
    n = 3
    data = rng.integers(0, 256, (n, k, sb), dtype=np.uint8)
    par = gpu_encode(k, m, data, flags)
    for s in range(n):
        st, exp = oracle.encode(k, m, data[s], flags)
        assert st == 0
        assert (par[s] == exp).all(), (k, m, s, R.encode_kernel_name(k, m, sb))


@pytest.mark.parametrize("k,m", KM_SMALL)
@pytest.mark.parametrize("sb", [192, 2048])
def test_reconstruct_vs_oracle(oracle, nv, decode_mode, k, m, sb):
    rng = np.random.default_rng(k * 104729 + m)
    n = 2
    data = rng.integers(0, 256, (n, k, sb), dtype=np.uint8)
    par = oracle.encode_batch(k, m, data)
    for trial in range(3):
        lost = list(rng.choice(k + m, size=min(m, k), replace=False))
        if not any(i < k for i in lost):
            lost[0] = int(rng.integers(0, k))
        present = np.ones(k + m, np.uint8)
        present[lost] = 0
        missing = [i for i in range(k) if not present[i]]
        got = gpu_reconstruct(k, m, present, data, par)
        assert (got == data[:, missing]).all(), (k, m, trial, R.reconstruct_kernel_name(k, m, sb))
        # and the oracle agrees with itself through the same API
        exp = oracle.reconstruct_batch(k, m, present, np.concatenate([data, par], axis=1))
        assert (got == exp).all()


# ------------------------------------------------- bit-sliced network kernels
NET_KM = [(1, 1), (2, 1), (4, 2), (3, 4), (5, 5), (10, 4), (8, 4), (12, 4), (6, 3), (9, 8), (16, 16), (17, 16),
          (20, 16), (16, 8), (30, 2), (64, 4), (60, 8), (13, 7)]


@pytest.mark.parametrize("k,m", NET_KM)
@pytest.mark.parametrize("flags", [0, 1, 3])
def test_net_reconstruct_vs_oracle(oracle, monkeypatch, k, m, flags):
    """RS_AMD_DECODE=net: the e x k reconstruct map as a generated XOR network,
    against the oracle (both quirk modes: the D1 multiply is GF(2)-linear too)."""
    if not R.use_high_rate(k, m):
        pytest.skip("low rate")
    monkeypatch.setenv("RS_AMD_DECODE", "net")
    rng = np.random.default_rng(k * 131 + m * 7 + flags)
    sb, n = 8192, 2
    data = rng.integers(0, 256, (n, k, sb), dtype=np.uint8)
    par = oracle.encode_batch(k, m, data, quirks=flags)
    shards = np.concatenate([data, par], axis=1)
    for trial in range(2):
        e = int(rng.integers(1, min(k, m) + 1))
        lost = list(rng.choice(k, size=e, replace=False))
        extra = int(rng.integers(0, m - e + 1))  # also drop some recovery shards
        lost += [k + int(i) for i in rng.choice(m, size=extra, replace=False)]
        present = np.ones(k + m, np.uint8)
        present[lost] = 0
        missing = [i for i in range(k) if not present[i]]
        name = R.reconstruct_kernel_name(k, m, sb, present)
        got = gpu_reconstruct(k, m, present, data, par, flags)
        exp = oracle.reconstruct_batch(k, m, present, shards, quirks=flags)
        assert (got == exp).all(), (k, m, flags, lost, name)
        if flags & 1 == 0:
            assert (got == data[:, missing]).all()


@pytest.mark.parametrize("k,m,sb", [(10, 4, 4096), (10, 4, 12288), (16, 16, 4096), (4, 2, 65536), (30, 2, 8192)])
def test_net_matches_table_kernels(monkeypatch, k, m, sb):
    """Network kernels == table-driven kernels (JIT on/off), encode and reconstruct,
    on padded (strided) stripes."""
    rng = np.random.default_rng(sb + k)
    n = 3
    data = rng.integers(0, 256, (n, k, sb), dtype=np.uint8)
    present = np.ones(k + m, np.uint8)
    present[rng.choice(k, size=min(k, m), replace=False)] = 0
    missing = [i for i in range(k) if not present[i]]
    outs = {}
    for j in ("1", "0"):
        monkeypatch.setenv("RS_AMD_JIT", j)
        big = torch.zeros((n, k * sb + 4096), dtype=torch.uint8, device=DEV)  # stripe stride > k*sb
        big[:, :k * sb] = to_dev(data.reshape(n, -1))
        par = torch.zeros((n, m * sb + 1024), dtype=torch.uint8, device=DEV)
        assert R.lib().rs_encode_batch_dev(k, m, sb, n, big.data_ptr(), big.stride(0), par.data_ptr(),
                                           par.stride(0), 0, None) == 0, R.lib().rs_last_error()
        out = torch.zeros((n, len(missing), sb), dtype=torch.uint8, device=DEV)
        assert R.lib().rs_reconstruct_batch_dev(k, m, sb, n, present.ctypes.data, big.data_ptr(), big.stride(0),
                                                par.data_ptr(), par.stride(0), out.data_ptr(), out.stride(0),
                                                0, None) == 0, R.lib().rs_last_error()
        torch.cuda.synchronize()
        outs[j] = par[:, :m * sb].cpu().numpy()
        assert (out.cpu().numpy() == data[:, missing]).all(), j
    assert (outs["1"] == outs["0"]).all()


def test_reconstruct_not_enough_shards():
    data = np.zeros((1, 10, 64), np.uint8)
    par = np.zeros((1, 4, 64), np.uint8)
    present = np.ones(14, np.uint8)
    present[:5] = 0
    with pytest.raises(R.NotEnoughShards):
        gpu_reconstruct(10, 4, present, data, par)


def test_strided_and_unaligned_layouts(oracle):
    """Non-packed stripe strides and 4-byte-aligned (not 16) bases -> narrower lanes, same bytes."""
    rng = np.random.default_rng(9)
    k, m, sb, n = 10, 4, 1024, 5
    data = rng.integers(0, 256, (n, k, sb), dtype=np.uint8)
    exp = oracle.encode_batch(k, m, data)
    big = torch.zeros((n, k * sb + 4 + 64), dtype=torch.uint8, device=DEV)
    big[:, 4:4 + k * sb] = to_dev(data.reshape(n, -1))
    par = torch.zeros((n, m * sb + 8), dtype=torch.uint8, device=DEV)
    st = R.lib().rs_encode_batch_dev(k, m, sb, n, big.data_ptr() + 4, big.stride(0), par.data_ptr() + 4,
                                     par.stride(0), 0, None)
    assert st == 0, R.lib().rs_last_error()
    torch.cuda.synchronize()
    got = par[:, 4:4 + m * sb].cpu().numpy().reshape(n, m, sb)
    assert (got == exp).all()


# ------------------------------------------------------------ BASELINE sizes
def sample_columns(oracle, k, m, data, par, cols, flags=0):
    for s, c in cols:
        col = np.ascontiguousarray(data[s][:, 64 * c:64 * (c + 1)])
        st, exp = oracle.encode(k, m, col, flags)
        assert st == 0
        assert (par[s][:, 64 * c:64 * (c + 1)] == exp).all(), (s, c)


@pytest.mark.parametrize("decode_mode", ["fft", "auto"], indirect=True)
@pytest.mark.parametrize("k,m,sb,n,erase", [
    (10, 4, 1 << 20, 24, [0, 1, 2, 3]),       # configs[1]/[2] shape (fewer stripes)
    (4, 2, 64 << 10, 1, [1, 3]),              # configs[0]
    (200, 55, 256 << 10, 2, list(range(0, 110, 2))),  # configs[4]
])
def test_baseline_shapes_roundtrip(oracle, decode_mode, k, m, sb, n, erase):
    data = splitmix_bytes(0x5EED0000, n * k * sb).reshape(n, k, sb)
    par = gpu_encode(k, m, data)
    rng = np.random.default_rng(1)
    L = sb // 64
    cols = [(int(rng.integers(0, n)), int(c)) for c in rng.integers(0, L, 24)] + [(n - 1, L - 1), (0, 0)]
    sample_columns(oracle, k, m, data, par, cols)
    # every stripe in full against the oracle's batched (AVX2, threaded) encode
    exp = oracle.encode_batch(k, m, data, threads=16)
    assert (par == exp).all()
    present = np.ones(k + m, np.uint8)
    present[erase] = 0
    got = gpu_reconstruct(k, m, present, data, par)
    assert (got == data[:, erase]).all()
    # erase recovery shards too (any m of k+m)
    present = np.ones(k + m, np.uint8)
    lost = list(rng.choice(k, size=m // 2, replace=False)) + [k + i for i in range(m - m // 2)]
    present[lost] = 0
    missing = [i for i in range(k) if not present[i]]
    got = gpu_reconstruct(k, m, present, data, par)
    assert (got == data[:, missing]).all()


def test_linearity_full_size():
    """encode(a ^ b) == encode(a) ^ encode(b) at RS(10,4) 1 MiB (GF(2)-linearity)."""
    k, m, sb, n = 10, 4, 1 << 20, 4
    a = splitmix_bytes(11, n * k * sb).reshape(n, k, sb)
    b = splitmix_bytes(12, n * k * sb).reshape(n, k, sb)
    pa, pb, pab = gpu_encode(k, m, a), gpu_encode(k, m, b), gpu_encode(k, m, a ^ b)
    assert ((pa ^ pb) == pab).all()


@pytest.mark.parametrize("flags", [0, 3])
def test_reconstruct_matrix_ref_literal(oracle, monkeypatch, flags):
    """The matrix kernel reproduces the FFT reconstruct bit for bit in both quirk modes
    (the D1 multiply is GF(2)-linear, so its reconstruct is still a matrix of 16x16 maps)."""
    rng = np.random.default_rng(77)
    k, m, sb, n = 10, 4, 640, 3
    data = rng.integers(0, 256, (n, k, sb), dtype=np.uint8)
    par = oracle.encode_batch(k, m, data, quirks=flags)
    present = np.ones(k + m, np.uint8)
    present[[1, 4, 9]] = 0  # 3 originals lost, all 4 recovery present (one extra)
    outs = {}
    for mode in ("fft", "matrix"):
        monkeypatch.setenv("RS_AMD_DECODE", mode)
        outs[mode] = gpu_reconstruct(k, m, present, data, par, flags)
    assert (outs["fft"] == outs["matrix"]).all()
    exp = oracle.reconstruct_batch(k, m, present, np.concatenate([data, par], axis=1), quirks=flags)
    assert (outs["fft"] == exp).all()


def test_repeatable_and_nan_free_of_state():
    """Same inputs -> same bytes across calls and plan-cache hits."""
    k, m, sb = 10, 4, 1 << 16
    d = splitmix_bytes(3, 8 * k * sb).reshape(8, k, sb)
    assert (gpu_encode(k, m, d) == gpu_encode(k, m, d)).all()


@pytest.mark.parametrize("pinned,slice_mb,stage", [(True, None, None), (False, None, None), (False, "1", None),
                                                   (False, "2", None), (False, "1", "0")])
def test_host_batch_pipeline(oracle, monkeypatch, pinned, slice_mb, stage):
    """rs_encode_batch_host / rs_reconstruct_batch_host (H2D -> kernel -> D2H ring) == oracle,
    here with missing data and recovery rows (one copy per run of present rows). Pageable
    buffers go through the ring's pinned staging (RS_AMD_HOST_STAGE=0: the runtime's path),
    over many slices (RS_AMD_HOST_SLICE_MB) so both slots' staging is reused."""
    for name, val in (("RS_AMD_HOST_SLICE_MB", slice_mb), ("RS_AMD_HOST_STAGE", stage)):
        if val is not None:
            monkeypatch.setenv(name, val)
    k, m, sb, n = 10, 4, 1 << 16, 37  # several pipeline slices at 256 MiB / (k*sb) = 409 stripes? -> force small
    data = torch.from_numpy(splitmix_bytes(77, n * k * sb).reshape(n, k, sb))
    if pinned:
        data = data.pin_memory()
    par = torch.zeros((n, m, sb), dtype=torch.uint8)
    if pinned:
        par = par.pin_memory()
    R.encode_batch_host(k, m, data, par)
    exp = oracle.encode_batch(k, m, data.numpy(), threads=4)
    assert (par.numpy() == exp).all()
    for present in ([0, 1, 0, 1, 1, 1, 1, 0, 1, 1] + [1, 1, 1, 1], [0, 1, 0, 1, 1, 1, 1, 0, 1, 1] + [1, 0, 1, 1]):
        missing = [i for i in range(k) if not present[i]]
        out = torch.zeros((n, len(missing), sb), dtype=torch.uint8)
        R.reconstruct_batch_host(k, m, present, data, par, out)
        assert (out.numpy() == data.numpy()[:, missing]).all()


@pytest.mark.parametrize("devices", [None, [0, 0], [0, 0, 0]])
def test_host_batch_multi_device(oracle, devices):
    """rs_*_batch_host_multi: contiguous stripe ranges, one worker thread + staging
    ring per listed device (here the box's one GPU listed several times, so the
    workers share its ring and run concurrently through the C ABI) == oracle."""
    k, m, sb, n = 10, 4, 1 << 16, 11
    data = torch.from_numpy(splitmix_bytes(5, n * k * sb).reshape(n, k, sb)).pin_memory()
    par = torch.zeros((n, m, sb), dtype=torch.uint8).pin_memory()
    R.encode_batch_host_multi(k, m, data, par, devices)
    exp = oracle.encode_batch(k, m, data.numpy(), threads=4)
    assert (par.numpy() == exp).all()
    present = [1, 0, 1, 1, 0, 1, 1, 1, 1, 0] + [1, 1, 1, 1]
    missing = [i for i in range(k) if not present[i]]
    out = torch.zeros((n, len(missing), sb), dtype=torch.uint8).pin_memory()
    R.reconstruct_batch_host_multi(k, m, present, data, par, out, devices)
    assert (out.numpy() == data.numpy()[:, missing]).all()


@pytest.mark.parametrize("pinned", [True, False])
@pytest.mark.parametrize("op", ["encode", "reconstruct"])
def test_host_batch_error_drains_slices(oracle, monkeypatch, op, pinned):
    """A host batch whose 4th slice fails (fault injection, RS_AMD_INJECT_HOST_FAIL):
    the call returns the error only after the earlier slices' copies have landed
    (every slot stream drained; pageable: copied out of the staging), and no later slice is
    written."""
    k, m, sb, n = 10, 4, 1 << 16, 9
    monkeypatch.setenv("RS_AMD_HOST_SLICE_MB", "1")  # 1 MiB / 640 KiB -> 1 stripe per slice
    monkeypatch.setenv("RS_AMD_INJECT_HOST_FAIL", "3")

    def mem(t):
        return t.pin_memory() if pinned else t

    data = mem(torch.from_numpy(splitmix_bytes(91, n * k * sb).reshape(n, k, sb)))
    exp = oracle.encode_batch(k, m, data.numpy(), threads=4)
    if op == "encode":
        out = mem(torch.zeros((n, m, sb), dtype=torch.uint8))
        st = R.lib().rs_encode_batch_host(k, m, sb, n, data.data_ptr(), 0, out.data_ptr(), 0, 0)
        want = exp
    else:
        present = np.array([0, 1, 0, 1, 1, 1, 1, 0, 1, 1] + [1, 1, 1, 1], np.uint8)
        missing = [i for i in range(k) if not present[i]]
        par = mem(torch.from_numpy(exp))
        out = mem(torch.zeros((n, len(missing), sb), dtype=torch.uint8))
        st = R.lib().rs_reconstruct_batch_host(k, m, sb, n, present.ctypes.data, data.data_ptr(), 0, par.data_ptr(), 0,
                                               out.data_ptr(), 0, 0)
        want = data.numpy()[:, missing]
    assert st == 15  # RS_ERR_DEVICE (include/reedsol.h)
    got = out.numpy()
    assert (got[:3] == want[:3]).all()  # slices 0..2 complete when the call returned
    assert not got[3:].any()            # nothing from the failed slice on


@pytest.mark.parametrize("k,m,sb", [(10, 4, 4096), (5, 5, 320), (4, 2, 2048), (16, 16, 1024), (20, 16, 512),
                                    (200, 55, 512), (4, 2, 8192), (3, 3, 4096), (64, 4, 4096), (7, 1, 4096)])
@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("path", ["auto", "matrix", "fft"])
def test_reconstruct_per_stripe_patterns(oracle, monkeypatch, k, m, sb, flags, path):
    """rs_reconstruct_batch_dev_patterns: the syndrome network (auto: corrected, k <= 64,
    m <= 4, 4 KiB units; rs_psyn.hpp), else per-stripe matrices built on the GPU + the
    matrix kernel (matrix: corrected, W <= 32, max_e <= 8), or the FFT reconstruct kernels
    with the erasure locator evaluated per stripe (fft; the fallback of the others)."""
    monkeypatch.setenv("RS_AMD_PATTERNS", path)
    n = 9
    rng = np.random.default_rng(k * 31 + m + flags)
    data = rng.integers(0, 256, (n, k, sb), dtype=np.uint8)
    par = oracle.encode_batch(k, m, data, quirks=flags)
    present = np.ones((n, k + m), np.uint8)
    for s in range(n):
        lost = rng.choice(k + m, size=int(rng.integers(0, m + 1)), replace=False)
        present[s, lost] = 0
    present[n - 1, :] = 1
    present[n - 1, :m + 1] = 0  # not enough shards
    max_e = m
    out = torch.full((n, max_e, sb), 0xAB, dtype=torch.uint8, device=DEV)
    status = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    R.reconstruct_batch_dev_patterns(k, m, to_dev(present), to_dev(data), to_dev(par), out, status, flags)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    status = status.cpu().numpy()
    assert status[n - 1] == 2
    for s in range(n - 1):
        assert status[s] == 0, s
        missing = [i for i in range(k) if not present[s, i]]
        assert (out[s, len(missing):] == 0xAB).all(), s  # slots >= e_s are not written
        if not missing:
            continue
        exp = oracle.reconstruct_batch(k, m, present[s], np.concatenate([data[s:s + 1], par[s:s + 1]], axis=1),
                                       quirks=flags)
        assert (out[s, :len(missing)] == exp[0]).all(), (s, missing)
        if flags == 0:
            assert (out[s, :len(missing)] == data[s, missing]).all()


@pytest.mark.parametrize("flags", [0, 2])
@pytest.mark.parametrize("max_e", [1, 2, 4])
def test_per_stripe_syndrome_network(oracle, flags, max_e):
    """RS(10,4) 64 KiB, 4 random losses per stripe (the per-stripe benchmark's shape): the
    syndrome network against the oracle, D2 schedule too; stripes losing more originals
    than max_e restore the first max_e and report RS_ERR_INVALID_ARGUMENT (14)."""
    k, m, sb, n = 10, 4, 65536, 37
    assert R.patterns_kernel_name(k, m, sb, max_e, flags) == "psyn_k10_m4"
    rng = np.random.default_rng(1004 + flags + max_e)
    data = rng.integers(0, 256, (n, k, sb), dtype=np.uint8)
    par = oracle.encode_batch(k, m, data, quirks=flags, threads=8)
    present = np.ones((n, k + m), np.uint8)
    for s in range(n):
        present[s, rng.choice(k + m, size=4, replace=False)] = 0
    out = torch.full((n, max_e, sb), 0xAB, dtype=torch.uint8, device=DEV)
    status = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    R.reconstruct_batch_dev_patterns(k, m, to_dev(present), to_dev(data), to_dev(par), out, status, flags)
    torch.cuda.synchronize()
    out, status = out.cpu().numpy(), status.cpu().numpy()
    for s in range(n):
        missing = [i for i in range(k) if not present[s, i]]
        assert status[s] == (14 if len(missing) > max_e else 0), s
        got = missing[:max_e]
        assert (out[s, :len(got)] == data[s, got]).all(), (s, missing)
        assert (out[s, len(got):] == 0xAB).all(), s


@pytest.mark.parametrize("k,m,sb,n", [(200, 55, 8192, 13), (100, 20, 4096, 9), (33, 17, 4096, 7), (64, 64, 4096, 5),
                                      (40, 50, 8192, 6)])
@pytest.mark.parametrize("flags", [0, 2])
@pytest.mark.parametrize("max_e", [8, 20, 64])
def test_per_stripe_wide_codes(oracle, k, m, sb, n, flags, max_e):
    """Wide codes, per-stripe patterns: syndromes on the FFT kernel with per-stripe masks,
    then the generic e x e solve (rs_psyn.hpp) in output groups of 8 (max_e > 8: the
    plan's Gauss-Jordan runs one wave per stripe, k_wps_plan_wave). Stripes lose
    0..max_e + 4 originals (at most m, plus some recovery shards); more than max_e restore
    the first max_e and report 14; too few present report 2 and write nothing."""
    rng = np.random.default_rng(k * 7 + m + flags + max_e)
    assert R.patterns_kernel_name(k, m, sb, max_e, flags) in ("fft_decode", "fft_syndromes+psyn_solve")
    data = rng.integers(0, 256, (n, k, sb), dtype=np.uint8)
    par = oracle.encode_batch(k, m, data, quirks=flags, threads=8)
    present = np.ones((n, k + m), np.uint8)
    for s in range(n - 1):
        e = int(rng.integers(0, min(max_e + 4, m, k) + 1))
        present[s, rng.choice(k, size=e, replace=False)] = 0
        present[s, k + rng.choice(m, size=int(rng.integers(0, m - e + 1)), replace=False)] = 0
    present[n - 1, :] = 1
    present[n - 1, : m + 1] = 0  # not enough shards
    out = torch.full((n, max_e, sb), 0xAB, dtype=torch.uint8, device=DEV)
    status = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    R.reconstruct_batch_dev_patterns(k, m, to_dev(present), to_dev(data), to_dev(par), out, status, flags)
    torch.cuda.synchronize()
    out, status = out.cpu().numpy(), status.cpu().numpy()
    assert status[n - 1] == 2 and (out[n - 1] == 0xAB).all()
    for s in range(n - 1):
        missing = [i for i in range(k) if not present[s, i]]
        assert status[s] == (14 if len(missing) > max_e else 0), s
        got = missing[:max_e]
        assert (out[s, :len(got)] == data[s, got]).all(), (s, missing)
        assert (out[s, len(got):] == 0xAB).all(), s


@pytest.mark.parametrize("k,m,sb,n", [(100, 4, 8192, 7), (32, 8, 4096, 9), (64, 8, 8192, 5), (5, 5, 4096, 9),
                                      (256, 5, 4096, 3), (40, 12, 8192, 6), (16, 16, 4096, 9), (64, 16, 4096, 5),
                                      (9, 9, 4096, 7), (100, 10, 4096, 4)])
@pytest.mark.parametrize("flags", [0, 2])
@pytest.mark.parametrize("max_e", [4, 8, 16])
def test_per_stripe_mid_band(oracle, monkeypatch, k, m, sb, n, flags, max_e):
    """Mid-band codes on the per-stripe pattern path (round 3): the fused syndrome network
    for k <= 256, m <= 8 (rs_psyn.hpp; m > 4 solves one output at a time) and chunk-16
    FFT syndromes + the generic solve for 9 <= m <= 16. Stripes lose 0..max_e + 2
    originals and random recovery shards; more than max_e restore the first max_e (14)."""
    monkeypatch.setenv("RS_AMD_JIT_SYNC", "1")  # the pattern kernels, not a pending compile's fallback
    max_e = min(max_e, m)
    path = R.patterns_kernel_name(k, m, sb, max_e, flags)
    c = 1 << (m - 1).bit_length()
    if flags & 2 and k > c and k % c == 0:  # D2 drops the last chunk: not MDS, the reference decode as written
        assert path == "pattern_fft"
        pytest.skip("D2-dropping code: covered against the oracle by test_per_stripe_patterns_d2_dropping")
    assert path in (f"psyn_k{k}_m{m}", "fft_decode", "fft_syndromes+psyn_solve"), path
    rng = np.random.default_rng(k * 11 + m + flags + max_e)
    data = rng.integers(0, 256, (n, k, sb), dtype=np.uint8)
    par = oracle.encode_batch(k, m, data, quirks=flags, threads=8)
    present = np.ones((n, k + m), np.uint8)
    for s in range(n - 1):
        e = int(rng.integers(0, min(max_e + 2, m, k) + 1))
        present[s, rng.choice(k, size=e, replace=False)] = 0
        present[s, k + rng.choice(m, size=int(rng.integers(0, m - e + 1)), replace=False)] = 0
    present[n - 1, :] = 1
    present[n - 1, : m + 1] = 0  # not enough shards
    out = torch.full((n, max_e, sb), 0xAB, dtype=torch.uint8, device=DEV)
    status = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    R.reconstruct_batch_dev_patterns(k, m, to_dev(present), to_dev(data), to_dev(par), out, status, flags)
    torch.cuda.synchronize()
    out, status = out.cpu().numpy(), status.cpu().numpy()
    assert status[n - 1] == 2 and (out[n - 1] == 0xAB).all()
    for s in range(n - 1):
        missing = [i for i in range(k) if not present[s, i]]
        assert status[s] == (14 if len(missing) > max_e else 0), s
        got = missing[:max_e]
        assert (out[s, :len(got)] == data[s, got]).all(), (s, missing)
        assert (out[s, len(got):] == 0xAB).all(), s


@pytest.mark.parametrize("k,m,sb", [(8, 4, 4096), (100, 4, 4096), (32, 8, 8192), (4, 2, 2048), (64, 16, 4096),
                                    (128, 32, 2048)])
@pytest.mark.parametrize("flags", [2, 3])
def test_per_stripe_patterns_d2_dropping(oracle, k, m, sb, flags):
    """Codes whose D2 schedule drops the last full chunk (root.zig:151: k > chunk, k % chunk
    == 0): the parity ignores those shards, so the literal reconstruct (root.zig:268-335)
    is no decoder and its output depends on every present shard. Per-stripe patterns on
    such codes must reproduce it exactly: against oracle.reconstruct_batch(quirks=flags)
    stripe by stripe, with surplus recovery shards present in most stripes."""
    n = 7
    rng = np.random.default_rng(k * 17 + m + flags)
    data = rng.integers(0, 256, (n, k, sb), dtype=np.uint8)
    par = oracle.encode_batch(k, m, data, quirks=flags, threads=8)
    present = np.ones((n, k + m), np.uint8)
    for s in range(n):
        e = int(rng.integers(1, m + 1)) if s else m  # stripe 0: exactly k present
        present[s, rng.choice(k, size=e, replace=False)] = 0
        extra = m - e if s == 0 else int(rng.integers(0, m - e + 1))
        present[s, k + rng.choice(m, size=extra, replace=False)] = 0
    max_e = m
    out = torch.full((n, max_e, sb), 0xAB, dtype=torch.uint8, device=DEV)
    status = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    R.reconstruct_batch_dev_patterns(k, m, to_dev(present), to_dev(data), to_dev(par), out, status, flags)
    torch.cuda.synchronize()
    out, status = out.cpu().numpy(), status.cpu().numpy()
    for s in range(n):
        assert status[s] == 0, s
        missing = [i for i in range(k) if not present[s, i]]
        exp = oracle.reconstruct_batch(k, m, present[s], np.concatenate([data[s:s + 1], par[s:s + 1]], axis=1),
                                       quirks=flags)
        assert (out[s, :len(missing)] == exp[0]).all(), (s, missing)
        assert (out[s, len(missing):] == 0xAB).all(), s


@pytest.mark.parametrize("k,m", [(8, 4), (100, 4), (32, 8), (128, 32)])
def test_batch_reconstruct_d2_dropping(oracle, k, m):
    """The same for one pattern per batch under D2 alone (flags 2: the corrected multiply,
    so every path but the literal map would otherwise be eligible), surplus shards present."""
    sb, n = 4096, 3
    rng = np.random.default_rng(k * 5 + m)
    data = rng.integers(0, 256, (n, k, sb), dtype=np.uint8)
    par = oracle.encode_batch(k, m, data, quirks=2)
    shards = np.concatenate([data, par], axis=1)
    for trial in range(3):
        e = int(rng.integers(1, m + 1))
        present = np.ones(k + m, np.uint8)
        present[rng.choice(k, size=e, replace=False)] = 0
        present[k + rng.choice(m, size=int(rng.integers(0, m - e + 1)), replace=False)] = 0
        got = gpu_reconstruct(k, m, present, data, par, 2)
        exp = oracle.reconstruct_batch(k, m, present, shards, quirks=2)
        assert (got == exp).all(), (k, m, trial, R.reconstruct_kernel_name(k, m, sb, present))


@pytest.mark.parametrize("sb", [2, 6, 66, 70, 1000, 4102])
@pytest.mark.parametrize("k,m", [(10, 4), (5, 5), (200, 55)])
def test_shard_tails_vs_oracle(oracle, k, m, sb):
    """shard_bytes % 64 != 0 (the reference panics): tail chunk layout of root.zig:338-348."""
    rng = np.random.default_rng(sb * 7 + k)
    n = 3
    data = rng.integers(0, 256, (n, k, sb), dtype=np.uint8)
    par = gpu_encode(k, m, data)
    exp = oracle.encode_batch(k, m, data)
    assert (par == exp).all()
    present = np.ones(k + m, np.uint8)
    lost = rng.choice(k, size=min(m, k), replace=False)
    present[lost] = 0
    got = gpu_reconstruct(k, m, present, data, par)
    assert (got == data[:, sorted(lost)]).all()


@pytest.mark.parametrize("sb", [70, 1000, 4102])
@pytest.mark.parametrize("k,m", [(10, 4), (5, 5), (200, 55)])
def test_per_stripe_patterns_shard_tails(oracle, k, m, sb):
    """Per-stripe patterns with shard_bytes % 64 != 0 (root.zig:338-348 tail layout, as the
    other entry points): every stripe restores its lost originals; restored slots past a
    stripe's own e are left untouched."""
    rng = np.random.default_rng(sb + k * 13)
    n = 5
    data = rng.integers(0, 256, (n, k, sb), dtype=np.uint8)
    par = gpu_encode(k, m, data)
    assert (par == oracle.encode_batch(k, m, data)).all()
    present = np.ones((n, k + m), np.uint8)
    for s in range(n):
        e = int(rng.integers(0, min(k, m) + 1))
        present[s, rng.choice(k, size=e, replace=False)] = 0
        present[s, k + rng.choice(m, size=int(rng.integers(0, m - e + 1)), replace=False)] = 0
    max_e = min(k, m)
    out = torch.full((n, max_e, sb), 0x5A, dtype=torch.uint8, device=DEV)
    status = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    R.reconstruct_batch_dev_patterns(k, m, to_dev(present), to_dev(data), to_dev(par), out, status)
    torch.cuda.synchronize()
    out, status = out.cpu().numpy(), status.cpu().numpy()
    for s in range(n):
        assert status[s] == 0, s
        missing = [i for i in range(k) if not present[s, i]]
        assert (out[s, :len(missing)] == data[s, missing]).all(), (s, missing)
        assert (out[s, len(missing):] == 0x5A).all(), s


def test_more_than_65535_stripes(oracle):
    """Launch splitting at 65535 stripes (grid y): network encode + reconstruct over
    65,540 stripes; the stripes either side of the split are checked against the oracle."""
    k, m, sb, n = 4, 2, 4096, 65540
    g = torch.Generator(device=DEV)
    g.manual_seed(65540)
    d = torch.randint(0, 256, (n, k, sb), dtype=torch.uint8, device=DEV, generator=g)
    p = torch.zeros((n, m, sb), dtype=torch.uint8, device=DEV)
    R.encode_batch_dev(k, m, d, p)
    present = [0, 1, 1, 0, 1, 1]
    out = torch.zeros((n, 2, sb), dtype=torch.uint8, device=DEV)
    R.reconstruct_batch_dev(k, m, present, d, p, out)
    torch.cuda.synchronize()
    assert torch.equal(out, d[:, [0, 3]])
    idx = [0, 65533, 65534, 65535, 65536, n - 1]
    sample = d[idx].cpu().numpy()
    assert (p[idx].cpu().numpy() == oracle.encode_batch(k, m, sample)).all()


@pytest.mark.parametrize("k,m", [(16, 16), (32, 8), (12, 12)])
def test_net_tile_widths_agree(oracle, monkeypatch, k, m):
    """8-output (default) and 4-output network tiles, encode and reconstruct of
    multi-tile maps: identical bytes, equal to the oracle."""
    rng = np.random.default_rng(k * 31 + m)
    sb, n = 8192, 2
    data = rng.integers(0, 256, (n, k, sb), dtype=np.uint8)
    exp = oracle.encode_batch(k, m, data)
    lost = sorted(int(i) for i in rng.choice(k, size=min(k, m), replace=False))
    present = np.ones(k + m, np.uint8)
    present[lost] = 0
    for tile in ("8", "4"):
        monkeypatch.setenv("RS_AMD_NET_TILE", tile)
        d = to_dev(data)
        p = torch.zeros((n, m, sb), dtype=torch.uint8, device=DEV)
        R.encode_batch_dev(k, m, d, p)
        out = torch.zeros((n, len(lost), sb), dtype=torch.uint8, device=DEV)
        R.reconstruct_batch_dev(k, m, present, d, p, out)
        torch.cuda.synchronize()
        assert (p.cpu().numpy() == exp).all(), tile
        assert (out.cpu().numpy() == data[:, lost]).all(), tile


@pytest.mark.parametrize("k,m", [(100, 20), (30, 30), (40, 17), (33, 32)])
def test_chunk32_register_encode_vs_oracle(oracle, monkeypatch, k, m):
    """Chunk 32 (17 <= m <= 32) on the table path: the register kernel
    k_encode_reg<32,1> (and the syndrome reconstruct built on it), bit-exact."""
    monkeypatch.setenv("RS_AMD_JIT", "0")
    assert R.encode_kernel_name(k, m, 4096) == "encode_reg_w32_nv1"
    rng = np.random.default_rng(k * 7 + m)
    sb, n = 4096, 2
    data = rng.integers(0, 256, (n, k, sb), dtype=np.uint8)
    exp = oracle.encode_batch(k, m, data)
    d = to_dev(data)
    p = torch.zeros((n, m, sb), dtype=torch.uint8, device=DEV)
    R.encode_batch_dev(k, m, d, p)
    torch.cuda.synchronize()
    assert (p.cpu().numpy() == exp).all()
    lost = sorted(int(i) for i in rng.choice(k, size=m, replace=False))
    present = np.ones(k + m, np.uint8)
    present[lost] = 0
    out = torch.zeros((n, m, sb), dtype=torch.uint8, device=DEV)
    R.reconstruct_batch_dev(k, m, present, d, p, out)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == data[:, lost]).all(), R.reconstruct_kernel_name(k, m, sb, present)


@pytest.mark.parametrize("k,m,sb,n_lost", [(1000, 300, 128, 300), (4096, 4096, 64, 2000), (32768, 32768, 64, 4000),
                                           (65535, 1, 64, 1)])
def test_maximum_shard_counts_vs_oracle(oracle, k, m, sb, n_lost):
    """Shard counts up to the codec's limits (root.zig:397-415: chunk + k <= 65536,
    up to 32768 + 32768 and 65535 + 1): the generic work-buffer kernels with
    transforms of up to 65,536 points. Encode bit-exact vs the oracle; the
    reconstruct restores every erased original."""
    rng = np.random.default_rng(k + m)
    data = rng.integers(0, 256, (1, k, sb), dtype=np.uint8)
    par = gpu_encode(k, m, data)
    np.testing.assert_array_equal(par, oracle.encode_batch(k, m, data))
    lost = sorted(int(i) for i in rng.choice(k, size=n_lost, replace=False))
    present = np.ones(k + m, np.uint8)
    present[lost] = 0
    rest = gpu_reconstruct(k, m, present, data, par)
    np.testing.assert_array_equal(rest[0], data[0, lost])


@pytest.mark.parametrize("sb", [1024, 2048])
@pytest.mark.parametrize("k,m,n", [(10, 4, 5), (4, 2, 7), (16, 16, 3), (32, 8, 9), (6, 3, 1)])
def test_small_shard_networks_vs_oracle(oracle, monkeypatch, sb, k, m, n):
    """1 / 2 KiB shards on the network kernels (wave units span 4 / 2 stripes; for stripe
    counts that are no multiple of that, pieces past the batch are clamped to the last
    stripe of their wave unit and rewrite identical bytes, so nothing past row n is
    touched — the guard row checks it): encode (forced on, RS_AMD_NET_SMALL_ENCODE=1;
    encodes of small shards default to the table kernels) bit-exact vs the oracle,
    reconstruct restores the erased originals, and both equal the table kernels'
    (RS_AMD_NET_SMALL=0)."""
    monkeypatch.setenv("RS_AMD_NET_SMALL_ENCODE", "1")
    assert R.encode_kernel_name(k, m, sb).startswith("net_encode"), R.encode_kernel_name(k, m, sb)
    rng = np.random.default_rng(k * 131 + m + sb)
    data = rng.integers(0, 256, (n, k, sb), dtype=np.uint8)
    exp = oracle.encode_batch(k, m, data)
    d = to_dev(data)
    guard = 0xA5
    p = torch.full((n + 1, m, sb), guard, dtype=torch.uint8, device=DEV)  # row n: must stay untouched
    R.encode_batch_dev(k, m, d, p[:n])
    torch.cuda.synchronize()
    np.testing.assert_array_equal(p[:n].cpu().numpy(), exp)
    assert (p[n].cpu().numpy() == guard).all()
    lost = sorted(int(i) for i in rng.choice(k, size=min(m, k), replace=False))
    present = np.ones(k + m, np.uint8)
    present[lost] = 0
    assert R.reconstruct_kernel_name(k, m, sb, present).startswith("net_reconstruct")
    out = torch.full((n + 1, len(lost), sb), guard, dtype=torch.uint8, device=DEV)
    R.reconstruct_batch_dev(k, m, present, d, p[:n], out[:n])
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out[:n].cpu().numpy(), data[:, lost])
    assert (out[n].cpu().numpy() == guard).all()
    monkeypatch.setenv("RS_AMD_NET_SMALL", "0")
    assert not R.encode_kernel_name(k, m, sb).startswith("net_")
    p2 = torch.zeros((n, m, sb), dtype=torch.uint8, device=DEV)
    R.encode_batch_dev(k, m, d, p2)
    torch.cuda.synchronize()
    assert torch.equal(p2, p[:n])


@pytest.mark.parametrize("sb", [1024, 2048])
@pytest.mark.parametrize("n", [5, 7])
def test_small_shard_syndrome_network(oracle, monkeypatch, sb, n):
    """RS(200,55) losing 32 data shards at 1 / 2 KiB shards: the syndrome path's e x e
    map on its small-shard network variant (inputs rec ^ scratch per 1 KiB piece),
    compiled synchronously; ragged stripe counts with a guard row; == table kernels."""
    monkeypatch.setenv("RS_AMD_JIT_SYNC", "1")
    monkeypatch.setenv("RS_AMD_FDEC", "0")  # the syndrome path's forms (fused: test_gpu_fdec.py)
    k, m = 200, 55
    rng = np.random.default_rng(sb + n)
    data = rng.integers(0, 256, (n, k, sb), dtype=np.uint8)
    par = oracle.encode_batch(k, m, data, threads=8)
    lost = sorted(int(i) for i in rng.choice(k, size=32, replace=False))
    present = np.ones(k + m, np.uint8)
    present[lost] = 0
    name = R.reconstruct_kernel_name(k, m, sb, present)
    assert "net_syndrome" in name, name
    guard = 0x5A
    out = torch.full((n + 1, 32, sb), guard, dtype=torch.uint8, device=DEV)
    R.reconstruct_batch_dev(k, m, present, to_dev(data), to_dev(par), out[:n])
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out[:n].cpu().numpy(), data[:, lost])
    assert (out[n].cpu().numpy() == guard).all()
    monkeypatch.setenv("RS_AMD_NET_SMALL", "0")
    assert gpu_reconstruct(k, m, present, data, par).tobytes() == out[:n].cpu().numpy().tobytes()


@pytest.mark.parametrize("sb", [1024, 2048])
@pytest.mark.parametrize("k,m,n", [(16, 64, 5), (10, 20, 7)])
def test_small_shard_lowrate_networks(oracle, monkeypatch, sb, k, m, n):
    """Low-rate maps (up to 64 outputs, several 8-output tiles) on the small-shard network
    variants, JIT on and compiled synchronously: encode == oracle restatement (parity
    unpinned: the reference has no low-rate codec), reconstruct restores the data,
    both equal the table kernels (RS_AMD_NET_SMALL=0)."""
    monkeypatch.setenv("RS_AMD_JIT_SYNC", "1")
    monkeypatch.setenv("RS_AMD_NET_SMALL_ENCODE", "1")
    rng = np.random.default_rng(k * 7 + m + sb)
    data = rng.integers(0, 256, (n, k, sb), dtype=np.uint8)
    exp = oracle.encode_low_batch(k, m, data) if hasattr(oracle, "encode_low_batch") else None
    p = gpu_encode(k, m, data)
    if exp is not None:
        np.testing.assert_array_equal(p, exp)
    else:
        for s in range(n):
            st, e = oracle.encode_low(k, m, data[s])
            assert st == 0
            np.testing.assert_array_equal(p[s], e)
    lost = sorted(int(i) for i in rng.choice(k, size=min(k, m) // 2 + 1, replace=False))
    present = np.ones(k + m, np.uint8)
    present[lost] = 0
    got = gpu_reconstruct(k, m, present, data, p)
    np.testing.assert_array_equal(got, data[:, lost])
    monkeypatch.setenv("RS_AMD_NET_SMALL", "0")
    assert (gpu_encode(k, m, data) == p).all()
    assert (gpu_reconstruct(k, m, present, data, p) == got).all()
