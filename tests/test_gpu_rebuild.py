"""Rebuild on the GPU: rs_rebuild_batch_dev puts back every lost shard of a stripe, recovery shards
included. The expected originals are the data; the expected parity is oracle.encode_batch of it,
except for low-rate codes (unpinned parity), where it is the library's own encode. Every case
fills the missing slots with poison, pre-fills the output with a canary (slots a stripe does not
restore must keep it) and asserts that no input is written. Covers the fast form (the rebuild
variant of the syndrome network, both solve shapes), the general form (tables only, tails, a wide
and a low-rate code, slicing), their agreement, the scrub -> locate -> rebuild flow and
allocation failures."""
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
CANARY, POISON = 0xC3, 0x5E


@functools.lru_cache(maxsize=None)
def clean(k, m, sb, n):
    """(data [n, k, sb], its parity [n, m, sb]): computed once per shape, never modified."""
    data = splitmix_bytes(k * 1000 + m * 10 + sb + 3, n * k * sb).reshape(n, k, sb)
    if R.use_high_rate(k, m):
        par = O.encode_batch(k, m, data)
    else:  # unpinned parity: the library's own encode is the expected parity
        p = torch.zeros((n, m, sb), dtype=torch.uint8, device=DEV)
        R.encode_batch_dev(k, m, torch.from_numpy(data).to(DEV), p)
        torch.cuda.synchronize()
        par = p.cpu().numpy()
    data.setflags(write=False)
    par.setflags(write=False)
    return data, par


def device_rows(a, pad_rows=0, offset=0, fill=0x99):
    """CUDA tensor [n, rows, sb] holding `a`, inside [n, rows + pad_rows, sb] (a padded stripe stride)
    and `offset` bytes past a 16-byte boundary; the bytes around it hold `fill`."""
    n, rows, sb = a.shape
    flat = torch.full((n * (rows + pad_rows) * sb + 16,), fill, dtype=torch.uint8, device=DEV)
    whole = flat[offset:offset + n * (rows + pad_rows) * sb].view(n, rows + pad_rows, sb)
    t = whole[:, :rows]
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(DEV))
    assert t.data_ptr() % 16 == offset
    return t, flat


def rebuild(k, m, sb, patterns, max_e, pad_rows=0, offset=0, calls=1, wait=False):
    """One stripe per pattern (the list of its missing shards, originals [0, k), recovery [k, k + m)).
    -> (rebuilt [n, max_e + 1, sb] as numpy: the row past max_e must keep the canary, status, kernels
    of the last call)."""
    n = len(patterns)
    data, par = clean(k, m, sb, n)
    present = np.ones((n, k + m), np.uint8)
    d, p = np.array(data), np.array(par)
    for s, miss in enumerate(patterns):
        for i in miss:
            present[s, i] = 0
            (d[s, i] if i < k else p[s, i - k])[:] = splitmix_bytes(s * 100 + i, sb) | 1 if s % 2 else POISON
    dt, dflat = device_rows(d, pad_rows, offset)
    pt, pflat = device_rows(p, pad_rows, offset)
    pr = torch.from_numpy(present).to(DEV)
    d0, p0, pr0 = dflat.clone(), pflat.clone(), pr.clone()
    for c in range(calls):
        if c and wait:
            R.net_wait()
        out, oflat = device_rows(np.full((n, max_e + 1, sb), CANARY, np.uint8), pad_rows, offset, fill=CANARY)
        status = torch.full((n,), -1, dtype=torch.int32, device=DEV)
        ret = R.rebuild_batch_dev(k, m, pr, dt, pt, out[:, :max_e], status=status)
        kernels = ";".join(R.last_kernels())
        torch.cuda.synchronize()
        assert ret.data_ptr() == status.data_ptr()
        assert torch.equal(dflat, d0) and torch.equal(pflat, p0) and torch.equal(pr, pr0)  # inputs unwritten
        assert (oflat[:offset] == CANARY).all() and (oflat[offset + out.numel() + n * pad_rows * sb:] == CANARY).all()
        if pad_rows:
            assert (oflat[offset:offset + n * (max_e + 1 + pad_rows) * sb].view(n, -1, sb)[:, max_e + 1:] == CANARY).all()
    return out.cpu().numpy(), status.cpu().tolist(), kernels


def expected(k, m, sb, patterns, max_e):
    """(rebuilt [n, max_e + 1, sb], status) per the contract"""
    n = len(patterns)
    data, par = clean(k, m, sb, n)
    want = np.full((n, max_e + 1, sb), CANARY, np.uint8)
    status = []
    for s, miss in enumerate(patterns):
        order = sorted(miss)  # originals ascending, then recovery shards ascending
        if len(order) > m:
            status.append(2)
            continue
        status.append(14 if len(order) > max_e else 0)
        for slot, i in enumerate(order[:max_e]):
            want[s, slot] = data[s, i] if i < k else par[s, i - k]
    return want, status


def check(k, m, sb, patterns, max_e, **kw):
    got, status, kernels = rebuild(k, m, sb, patterns, max_e, **kw)
    want, want_status = expected(k, m, sb, patterns, max_e)
    assert status == want_status, (status, want_status, kernels)
    bad = np.argwhere((got != want).any(axis=2))
    assert bad.size == 0, (bad.tolist(), kernels)
    return kernels


# RS(10, 4): each single shard, originals only, recovery only up to all 4, mixed 1+1, 2+2, 3+1 and
# 1+3, a clean stripe, 5 missing (status 2, no byte written)
RS10_4 = ([[i] for i in range(14)] + [[0, 9], [1, 4, 7], [0, 1, 2, 3], [6, 9, 3, 5]] +
          [[10, 13], [11, 12], [10, 11, 12], [11, 12, 13], [10, 11, 12, 13]] +
          [[3, 11], [0, 9, 10, 13], [2, 5, 8, 12], [6, 10, 11, 13]] + [[]] + [[0, 1, 2, 10, 11], [4, 10, 11, 12, 13]])
# max_e = 2 beside e_s = 3: status 14, the first two slots in the contract's order, an intact third
RS10_4_MAX2 = [[1, 5, 12], [4, 10, 11], [10, 11, 12], [0, 1, 2], [7], [13], [2, 12], [], [0, 1, 2, 3, 4]]


# ------------------------------------------------------------------------ fast form
@pytest.mark.parametrize("sb,pad_rows", [(4096, 0), (8192, 3)], ids=["4k", "8k_padded_stride"])
def test_fast_rs10_4(sb, pad_rows):
    k, m = 10, 4
    assert R.rebuild_kernel_name(k, m, sb, 4) == "psyn_rebuild_k10_m4"
    kernels = check(k, m, sb, RS10_4, 4, pad_rows=pad_rows, calls=2, wait=True)
    assert "k_psyn_rebuild_plan" in kernels and "rs_psyn_rebuild_k10_m4_" in kernels, kernels
    assert "k_rebuild_gather" not in kernels, kernels
    kernels = check(k, m, sb, RS10_4_MAX2, 2, pad_rows=pad_rows)
    assert "rs_psyn_rebuild_k10_m4_" in kernels, kernels


def test_fast_max_e_1():
    """max_e = 1: a stripe's first missing shard only, an original before a recovery shard"""
    kernels = check(10, 4, 4096, [[3], [12], [3, 12], [11, 12], []], 1)
    assert "rs_psyn_rebuild_" in kernels, kernels


def test_fast_rs4_4():
    """m = 4 beside k < 8: the rebuild variant takes the one-output-at-a-time solve; k = m, so every
    original can be lost"""
    pats = [[0, 1, 2, 3], [4, 5, 6, 7], [0, 3, 5, 6], [2], [7], [1, 4], [], [0, 1, 2, 4, 5]]
    kernels = check(4, 4, 4096, pats, 4, calls=2, wait=True)
    assert "rs_psyn_rebuild_k4_m4_" in kernels, kernels


RS33_5 = [[0, 32, 33], [5, 37], [33, 34, 35, 36, 37], [1, 2, 3, 4, 31], [7, 20, 34, 35, 36], [32], [36], [],
          [0, 1, 2, 33, 34, 35], [31, 32, 33, 37]]


def test_fast_rs33_5():
    """two erased-mask words, and the one-output-at-a-time solve; the kernel compiles in the background,
    so the first call takes the general form"""
    k, m, sb = 33, 5, 4096
    kernels = check(k, m, sb, RS33_5, 5, calls=2, wait=True)
    assert "rs_psyn_rebuild_k33_m5_" in kernels, kernels
    kernels = check(k, m, sb, RS33_5, 3)
    assert "rs_psyn_rebuild_k33_m5_" in kernels, kernels


# --------------------------------------------------------------------- general form
def test_general_no_jit(monkeypatch):
    monkeypatch.setenv("RS_AMD_JIT", "0")
    kernels = check(10, 4, 4096, RS10_4, 4)
    assert "psyn" not in kernels, kernels
    for name in ("k_rebuild_prepare", "k_rebuild_gather_x16", "k_rebuild_pick_x16"):
        assert name in kernels, kernels
    check(10, 4, 4096, RS10_4_MAX2, 2)


def test_general_tail_offset():
    """sb = 100 (one whole chunk and a tail) on buffers 4 bytes past a 16-byte boundary"""
    kernels = check(10, 4, 100, RS10_4, 4, offset=4)
    assert "k_rebuild_gather_x4" in kernels and "k_rebuild_pick_x4" in kernels, kernels
    check(10, 4, 100, RS10_4_MAX2, 2, offset=4)
    kernels = check(10, 4, 4096 + 34, RS10_4[10:], 4, offset=2)  # no multiple of 4: bytes
    assert "k_rebuild_gather_x1" in kernels, kernels


def test_general_unaligned_whole_units():
    """a psyn shape on 4-byte-aligned buffers: the general form, dword copies"""
    kernels = check(10, 4, 4096, RS10_4[8:24], 4, offset=4)
    assert "psyn_rebuild" not in kernels and "k_rebuild_gather_x4" in kernels, kernels


def test_general_wide():
    """RS(200, 55): up to 20 missing, mixed; a stripe beyond max_e and an undecodable one"""
    k, m, sb = 200, 55, 2048
    pats = [list(range(0, 200, 17)) + [200 + r for r in range(0, 55, 7)],  # 12 + 8
            [200 + r for r in range(20)],  # recovery only
            [199, 0, 100, 254, 200],
            list(range(10, 31)) + [210],  # 22 > max_e: status 14, the first 20 are originals
            ]
    assert len(pats[0]) == 20 and len(pats[3]) == 22
    kernels = check(k, m, sb, pats, 20)
    assert "k_rebuild_gather" in kernels and "k_rebuild_pick" in kernels, kernels
    check(k, m, sb, [list(range(56)), [3, 250], []], 2)  # 56 missing: status 2


def test_general_low_rate():
    k, m, sb = 3, 9, 4096
    pats = [[0], [3], [11], [0, 1, 5, 6, 7, 8, 9, 10, 11], [3, 4, 5, 6, 7, 8], [2, 4], [], [1, 2, 3, 4, 5, 6, 7, 8, 9, 10]]
    check(k, m, sb, pats, 9)
    check(k, m, sb, pats, 2)


def test_general_low_rate_small_m():
    """RS(3, 5) and RS(2, 4): low-rate codes that the syndrome network's shape test (k <= 256, m <= 8,
    whole 4 KiB units) would take, but whose parity comes from the low-rate construction: the general
    form, and the library's own encode as the expected parity"""
    for k, m, pats in [(3, 5, [[0], [3], [7], [0, 4], [1, 2, 3, 5, 6], [3, 4, 5, 6, 7], [0, 1, 2], [], [0, 1, 2, 3, 4, 5]]),
                       (2, 4, [[1], [5], [0, 1, 2, 3], [2, 3, 4, 5], [0, 3], []])]:
        assert not R.use_high_rate(k, m)
        kernels = check(k, m, 4096, pats, m, calls=2, wait=True)
        assert "psyn_rebuild" not in kernels and "k_rebuild_gather_x16" in kernels, kernels
        check(k, m, 4096, pats, 2)


def test_general_slices(monkeypatch):
    """RS(200, 55), sb = 64: 16 KB of scratch per stripe, 150 stripes under a 1 MiB cap: 3 slices"""
    monkeypatch.setenv("RS_AMD_SCRATCH_CAP_MB", "1")
    k, m, sb, n = 200, 55, 64, 150
    pats = [[(s * 7) % k, k + s % m] if s % 3 else ([k + (s * 5) % m] if s % 2 else [(s * 11) % k]) for s in range(n)]
    pats[70] = list(range(56))  # undecodable, in the middle slice
    pats[71] = []
    kernels = check(k, m, sb, pats, 2)
    assert kernels.count("k_rebuild_pick") >= 3, kernels


def test_slices_fast_shape(monkeypatch):
    """one stripe per slice at the least: RS(10, 4), 64 KiB shards (896 KiB a stripe) under a 1 MiB cap"""
    monkeypatch.setenv("RS_AMD_SCRATCH_CAP_MB", "1")
    monkeypatch.setenv("RS_AMD_JIT", "0")
    kernels = check(10, 4, 1 << 16, [[0, 10], [13], [5]], 2)
    assert kernels.count("k_rebuild_pick") == 3, kernels


# ------------------------------------------------------------------------ agreement
def test_forms_agree(monkeypatch):
    k, m, sb = 10, 4, 8192
    pats = RS10_4 + RS10_4_MAX2
    fast = rebuild(k, m, sb, pats, 3)
    assert "rs_psyn_rebuild_" in fast[2], fast[2]
    monkeypatch.setenv("RS_AMD_JIT", "0")
    general = rebuild(k, m, sb, pats, 3)
    assert "k_rebuild_gather" in general[2] and "psyn" not in general[2], general[2]
    assert fast[1] == general[1]
    assert (fast[0] == general[0]).all()
    assert fast[1] == expected(k, m, sb, pats, 3)[1]


# ----------------------------------------------------------------------------- flow
def test_scrub_locate_rebuild():
    """One corrupt original, one corrupt recovery shard, two corrupt recovery shards: locate's present
    rows go to rebuild as they are, max_e = m - 1, and writing the rebuilt shards back heals all."""
    k, m, sb, n = 10, 4, 4096, 5
    data, par = clean(k, m, sb, n)
    d, p = torch.from_numpy(np.array(data)).to(DEV), torch.from_numpy(np.array(par)).to(DEV)
    d[1, 6, 100] ^= 0x10
    p[2, 3, 4000] ^= 0x01
    p[4, 0, 0] ^= 0x80
    p[4, 2, 77] ^= 0x08
    present = torch.full((n, k + m), 9, dtype=torch.uint8, device=DEV)
    located = R.locate_batch_dev(k, m, d, p, present=present)
    rebuilt = torch.full((n, m - 1, sb), CANARY, dtype=torch.uint8, device=DEV)
    status = R.rebuild_batch_dev(k, m, present, d, p, rebuilt)
    torch.cuda.synchronize()
    assert located.cpu().tolist() == [R.LOCATE_CLEAN, 6, k + 3, R.LOCATE_CLEAN, R.LOCATE_RECOVERY_SET]
    assert status.cpu().tolist() == [0] * n
    pres, rb = present.cpu().numpy(), rebuilt.cpu().numpy()
    for s in range(n):  # the caller's write-back: slot order = originals, then recovery shards
        missing = [i for i in range(k + m) if not pres[s, i]]
        for slot, i in enumerate(missing):
            (d[s, i] if i < k else p[s, i - k]).copy_(rebuilt[s, slot])
        assert (rb[s, len(missing):] == CANARY).all()
    assert [len([i for i in range(k + m) if not pres[s, i]]) for s in range(n)] == [0, 1, 1, 0, 2]
    torch.cuda.synchronize()
    assert (d.cpu().numpy() == data).all() and (p.cpu().numpy() == par).all()
    assert R.verify_batch_dev(k, m, d, p).sum().item() == 0


# -------------------------------------------------------------- allocation failures
@pytest.mark.parametrize("jit", ["1", "0"], ids=["fast", "general"])
def test_every_allocation_fails_cleanly(monkeypatch, jit):
    """Every allocation of a cold call fails in turn: each call returns OutOfMemory, and the library
    works once disarmed (tests/test_gpu_verify.py's protocol)."""
    monkeypatch.setenv("RS_AMD_JIT", jit)
    k, m, sb = 10, 4, 4096
    pats = [[2, 11], [], [13], [0, 1, 2, 3]]
    n = len(pats)
    data, par = clean(k, m, sb, n)
    present = np.ones((n, k + m), np.uint8)
    for s, miss in enumerate(pats):
        present[s, miss] = 0
    d, p = torch.from_numpy(np.array(data)).to(DEV), torch.from_numpy(np.array(par)).to(DEV)
    pr = torch.from_numpy(present).to(DEV)
    out = torch.full((n, m + 1, sb), CANARY, dtype=torch.uint8, device=DEV)
    status = torch.zeros((n,), dtype=torch.int32, device=DEV)

    def call():
        R.rebuild_batch_dev(k, m, pr, d, p, out[:, :m], status=status)
        torch.cuda.synchronize()

    call()  # kernels loaded
    R.net_wait()
    R.debug_release_caches()
    R.debug_fail_alloc(-1)
    call()  # a cold call: count its allocations
    n_alloc = R.debug_fail_alloc(-1)
    assert n_alloc >= 3, n_alloc  # a plan, the device tables, the scratch
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
    out.fill_(CANARY)
    status.fill_(77)
    call()
    want, want_status = expected(k, m, sb, pats, m)
    assert status.cpu().tolist() == want_status
    assert (out.cpu().numpy() == want).all()
