"""Verify (scrub) on the GPU: rs_verify_batch_dev's flags against the oracle,
expected = (stored != oracle.encode_batch(k, m, data, quirks=flags)).any(axis=2), over the
encode's kernel families (networks, FFT kernels, table kernels, small shards, tails, low rate),
the compare kernel's three load widths, strides, slicing and allocation failures. Low-rate
parity is unpinned, so those cases take the library's own encode as the clean parity."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import oracle as O  # noqa: E402
from helpers import splitmix_bytes  # noqa: E402
from rs_amd import reedsol_amd as R  # noqa: E402

DEV = torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def clean(k, m, sb, n, flags=0):
    """(data [n, k, sb], its oracle parity [n, m, sb]): computed once per shape, never modified."""
    data = splitmix_bytes(k * 1000 + m * 10 + flags + sb, n * k * sb).reshape(n, k, sb)
    par = O.encode_batch(k, m, data, quirks=flags)
    data.setflags(write=False)
    par.setflags(write=False)
    return data, par


def expected(stored, par):
    return (stored != par).any(axis=2).astype(np.uint8)


def verify(k, m, data, stored, flags=0):
    """-> (bad [n, m], count, the kernels the call launched)"""
    d, p = torch.from_numpy(np.array(data)).to(DEV), torch.from_numpy(np.array(stored)).to(DEV)
    count = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    bad = R.verify_batch_dev(k, m, d, p, count=count, flags=flags)
    kernels = ";".join(R.last_kernels())
    torch.cuda.synchronize()
    assert bad.dtype == torch.uint8 and tuple(bad.shape) == (data.shape[0], m)
    return bad.cpu().numpy(), int(count.item()), kernels


def corrupt(par, s, r, off, bit=0x40):
    stored = par.copy()
    stored[s, r, off] ^= bit
    return stored


# ------------------------------------------------- whole 4 KiB units, aligned
@pytest.mark.parametrize("n", [1, 3, 9])
@pytest.mark.parametrize("sb", [4096, 8192, 20480])
@pytest.mark.parametrize("flags", [0, 3])
def test_rs10_4_whole_units(flags, sb, n):
    k, m = 10, 4
    data, par = clean(k, m, sb, n, flags)
    bad, count, kernels = verify(k, m, data, par, flags)
    assert not bad.any() and count == 0
    assert "rs_net_encode_" in kernels and "verify_compare" in kernels and "verify_count" in kernels, kernels
    last = sb - 4096  # the shard's last 4 KiB unit
    cases = [(0, 0, 0),  # the first byte of recovery 0 in stripe 0
             (n - 1, m - 1, sb - 1),  # the last byte of the last recovery shard in the last stripe
             (n // 2, 1, last + 5 * 64 + 7),  # the low half of a 64-byte chunk of the last unit
             (n // 2, 2, last + 9 * 64 + 40)]  # the high half
    assert cases[2][2] % 64 < 32 <= cases[3][2] % 64
    for s, r, off in cases:
        stored = corrupt(par, s, r, off)
        exp = expected(stored, par)
        assert exp.sum() == 1 and exp[s, r] == 1
        bad, count, kernels = verify(k, m, data, stored, flags)
        assert (bad == exp).all(), (s, r, off, bad)
        assert count == 1


def test_corrupt_original_sets_every_flag():
    k, m, sb, n = 10, 4, 8192, 3
    data, par = clean(k, m, sb, n)
    broken = data.copy()
    broken[1, 7, 4321] ^= 0x04
    exp = expected(par, O.encode_batch(k, m, broken))
    assert exp[1].all() and exp.sum() == m  # every encode block is a multiplication by a nonzero element
    bad, count, kernels = verify(k, m, broken, par)
    assert (bad == exp).all(), bad
    assert count == m


@pytest.mark.parametrize("k,m", [(32, 8), (6, 3)])
def test_other_network_codes(k, m):
    sb, n = 4096, 2
    data, par = clean(k, m, sb, n)
    stored = corrupt(par, 0, m - 1, 2049)
    stored[1, 0, 4095] ^= 0x01
    exp = expected(stored, par)
    assert exp.sum() == 2
    bad, count, kernels = verify(k, m, data, stored)
    assert (bad == exp).all(), bad
    assert count == 2
    assert f"rs_net_encode_i{k}_o{m}_" in kernels and "verify_compare" in kernels, kernels


@pytest.mark.parametrize("jit", ["1", "0"])
def test_strides_and_guards(monkeypatch, jit):
    """Strided inputs, a flag row stride above m: the bytes between the rows stay untouched, and
    the inputs are not written."""
    monkeypatch.setenv("RS_AMD_JIT", jit)
    k, m, sb, n = 10, 4, 4096, 3
    data, par = clean(k, m, sb, n)
    stored = corrupt(par, 2, 3, 1000)
    stored[0, 1, 77] ^= 0x80
    exp = expected(stored, par)
    orig_t = torch.from_numpy(splitmix_bytes(5, n * (k + 3) * sb).reshape(n, k + 3, sb)).to(DEV)
    rec_t = torch.from_numpy(splitmix_bytes(6, n * (m + 2) * sb).reshape(n, m + 2, sb)).to(DEV)
    orig_t[:, :k] = torch.from_numpy(data.copy()).to(DEV)
    rec_t[:, :m] = torch.from_numpy(stored).to(DEV)
    orig0, rec0 = orig_t.clone(), rec_t.clone()
    bad_t = torch.full((n, m + 5), 7, dtype=torch.uint8, device=DEV)
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    out = R.verify_batch_dev(k, m, orig_t[:, :k], rec_t[:, :m], bad=bad_t[:, :m], count=count)
    kernels = ";".join(R.last_kernels())
    torch.cuda.synchronize()
    assert ("rs_net_encode_" in kernels) == (jit == "1") and "verify_compare" in kernels, kernels
    assert out.data_ptr() == bad_t.data_ptr()
    got = bad_t.cpu().numpy()
    assert (got[:, m:] == 7).all()
    assert (got[:, :m] == exp).all(), got
    assert int(count.item()) == 2
    assert torch.equal(orig_t, orig0) and torch.equal(rec_t, rec0)


# ------------------------------------------------------- the other encode forms
def check_one_byte(k, m, sb, n, flags=0, low=False):
    """One corrupted recovery byte in the last stripe (+ a clean stripe where n > 1)."""
    if low:  # unpinned parity: the library's own encode is the clean parity
        data = splitmix_bytes(k + m + sb, n * k * sb).reshape(n, k, sb)
        p = torch.zeros((n, m, sb), dtype=torch.uint8, device=DEV)
        R.encode_batch_dev(k, m, torch.from_numpy(data).to(DEV), p, flags)
        torch.cuda.synchronize()
        par = p.cpu().numpy()
    else:
        data, par = clean(k, m, sb, n, flags)
    stored = corrupt(par, n - 1, m // 2, sb - 3)
    exp = expected(stored, par)
    assert exp.sum() == 1
    bad, count, kernels = verify(k, m, data, stored, flags)
    assert (bad == exp).all(), (bad, kernels)
    assert count == 1
    assert "verify_compare" in kernels, kernels
    return kernels


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("sb", [1024, 2048])
def test_small_shards(sb, n):
    check_one_byte(10, 4, sb, n)  # odd batches of the small-piece form


@pytest.mark.parametrize("sb", [4096 + 34, 130])
def test_tails(sb):
    check_one_byte(10, 4, sb, 2)  # tails: shard starts are 2-byte aligned


def test_unaligned_recovery():
    """The recovery tensor offset by 4 bytes: the compare's dword path."""
    k, m, sb, n = 10, 4, 4096, 2
    data, par = clean(k, m, sb, n)
    stored = corrupt(par, 1, 0, 4092)
    exp = expected(stored, par)
    flat = torch.zeros(n * m * sb + 16, dtype=torch.uint8, device=DEV)
    rec = flat[4:4 + n * m * sb].view(n, m, sb)
    rec.copy_(torch.from_numpy(stored).to(DEV))
    assert rec.data_ptr() % 16 == 4
    bad = R.verify_batch_dev(k, m, torch.from_numpy(data.copy()).to(DEV), rec)
    kernels = ";".join(R.last_kernels())
    torch.cuda.synchronize()
    assert (bad.cpu().numpy() == exp).all()
    assert "verify_compare" in kernels, kernels


@pytest.mark.parametrize("k,m,n", [(200, 55, 2), (16, 16, 2)])
def test_wide_codes(k, m, n):
    check_one_byte(k, m, 4096, n)


def test_low_rate():
    check_one_byte(3, 10, 4096, 2, low=True)


def test_without_jit(monkeypatch):
    monkeypatch.setenv("RS_AMD_JIT", "0")
    check_one_byte(10, 4, 4096, 2)


def test_slices(monkeypatch):
    """2.25 MiB of parity under a 1 MiB scratch cap: at least 3 slices."""
    monkeypatch.setenv("RS_AMD_JIT", "0")
    monkeypatch.setenv("RS_AMD_SCRATCH_CAP_MB", "1")
    k, m, sb, n = 10, 4, 65536, 9
    data, par = clean(k, m, sb, n)
    stored = par.copy()
    for s, r, off in [(0, 0, 17), (4, 3, 65535), (8, 1, 30000)]:
        stored[s, r, off] ^= 0x10
    exp = expected(stored, par)
    assert exp.sum() == 3
    bad, count, kernels = verify(k, m, data, stored)
    assert (bad == exp).all(), bad
    assert count == 3
    assert "verify_compare" in kernels


def test_network_and_table_encodes_agree(monkeypatch):
    k, m, sb, n = 10, 4, 8192, 9
    data, par = clean(k, m, sb, n)
    rng = np.random.default_rng(20251)
    stored = par.copy()
    for _ in range(5):
        stored[rng.integers(n), rng.integers(m), rng.integers(sb)] ^= np.uint8(1 << rng.integers(8))
    exp = expected(stored, par)
    net, c1, k1 = verify(k, m, data, stored)
    monkeypatch.setenv("RS_AMD_JIT", "0")
    plain, c2, k2 = verify(k, m, data, stored)
    assert "rs_net_encode_" in k1 and "rs_net_encode_" not in k2 and "verify_compare" in k1 and "verify_compare" in k2
    assert (net == plain).all() and (net == exp).all()
    assert c1 == c2 == int(exp.sum())


def test_every_allocation_fails_cleanly(monkeypatch):
    """Every allocation of a cold call fails in turn: each call returns OutOfMemory,
    and the library works once disarmed (tests/test_gpu_alloc_fail.py's protocol)."""
    monkeypatch.setenv("RS_AMD_JIT", "0")
    k, m, sb, n = 10, 4, 4096, 2
    data, par = clean(k, m, sb, n)
    stored = corrupt(par, 0, 2, 5)
    exp = expected(stored, par)
    d, p = torch.from_numpy(data.copy()).to(DEV), torch.from_numpy(stored).to(DEV)
    bad = torch.zeros((n, m), dtype=torch.uint8, device=DEV)
    count = torch.zeros(1, dtype=torch.int64, device=DEV)

    def call():
        R.verify_batch_dev(k, m, d, p, bad=bad, count=count)
        torch.cuda.synchronize()

    call()  # kernels loaded
    R.net_wait()
    R.debug_release_caches()
    R.debug_fail_alloc(-1)
    call()  # a cold call: count its allocations
    n_alloc = R.debug_fail_alloc(-1)
    assert n_alloc >= 1, n_alloc
    R.debug_release_caches()
    try:
        for i in range(n_alloc):
            R.debug_fail_alloc(i)
            with pytest.raises(R.OutOfMemory):
                call()
            R.debug_fail_alloc(-1)
            R.debug_release_caches()
    finally:
        R.debug_fail_alloc(-1)
    bad.fill_(9)
    call()
    assert (bad.cpu().numpy() == exp).all()
    assert int(count.item()) == 1
