"""Locate on the GPU: rs_locate_batch_dev names the shard each test corrupts. The expected answer
is known by construction; the clean parity is oracle.encode_batch, except for low-rate codes
(unpinned parity), where it is the library's own encode. Covers the compare's and the confirm's
three load widths, tails, every outcome, strides, slicing, the heal through
rs_reconstruct_batch_dev_patterns and allocation failures."""
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
CLEAN, RECOVERY_SET, UNLOCATED = R.LOCATE_CLEAN, R.LOCATE_RECOVERY_SET, R.LOCATE_UNLOCATED


@functools.lru_cache(maxsize=None)
def clean(k, m, sb, n):
    """(data [n, k, sb], its clean parity [n, m, sb]): computed once per shape, never modified."""
    data = splitmix_bytes(k * 1000 + m * 10 + sb, n * k * sb).reshape(n, k, sb)
    if R.use_high_rate(k, m):
        par = O.encode_batch(k, m, data)
    else:  # unpinned parity: the library's own encode is the clean parity
        p = torch.zeros((n, m, sb), dtype=torch.uint8, device=DEV)
        R.encode_batch_dev(k, m, torch.from_numpy(data).to(DEV), p)
        torch.cuda.synchronize()
        par = p.cpu().numpy()
    data.setflags(write=False)
    par.setflags(write=False)
    return data, par


def locate(k, m, data, stored, rec_offset=0):
    """-> (located [n], present [n, k + m], counts [4], the kernels the call launched).
    rec_offset: the recovery tensor starts that many bytes past a 16-byte boundary."""
    n, _, sb = data.shape
    d = torch.from_numpy(np.array(data)).to(DEV)
    if rec_offset:
        flat = torch.zeros(n * m * sb + 16, dtype=torch.uint8, device=DEV)
        p = flat[rec_offset:rec_offset + n * m * sb].view(n, m, sb)
        p.copy_(torch.from_numpy(np.array(stored)).to(DEV))
        assert p.data_ptr() % 16 == rec_offset
    else:
        p = torch.from_numpy(np.array(stored)).to(DEV)
    d0, p0 = d.clone(), p.clone()
    located = torch.full((n,), 77, dtype=torch.int32, device=DEV)
    present = torch.full((n, k + m), 9, dtype=torch.uint8, device=DEV)
    counts = torch.full((4,), -1, dtype=torch.int64, device=DEV)
    out = R.locate_batch_dev(k, m, d, p, located=located, present=present, counts=counts)
    kernels = ";".join(R.last_kernels())
    torch.cuda.synchronize()
    assert out.data_ptr() == located.data_ptr() and out.dtype == torch.int32
    assert torch.equal(d, d0) and torch.equal(p, p0)  # neither input is written
    return located.cpu().numpy(), present.cpu().numpy(), counts.cpu().tolist(), kernels


def expected_present(k, m, located, bad_recovery=()):
    """The rows the located answers imply; bad_recovery: (stripe, r) cleared in RECOVERY_SET stripes."""
    pres = np.ones((len(located), k + m), np.uint8)
    for s, loc in enumerate(located):
        if loc >= 0:
            pres[s, loc] = 0
    for s, r in bad_recovery:
        pres[s, k + r] = 0
    return pres


def expected_counts(located):
    loc = np.asarray(located)
    return [int((loc == CLEAN).sum()), int((loc >= 0).sum()), int((loc == RECOVERY_SET).sum()),
            int((loc == UNLOCATED).sum())]


def check(k, m, data, stored, want, bad_recovery=(), rec_offset=0):
    located, present, counts, kernels = locate(k, m, data, stored, rec_offset)
    assert located.tolist() == list(want), (located, want, kernels)
    assert (present == expected_present(k, m, want, bad_recovery)).all(), present
    assert counts == expected_counts(want), counts
    return kernels


def one_shard_cases(sb):
    """(name, offsets and masks) of the corruptions of one shard"""
    whole = sb - sb % 64
    last = whole - 64  # a whole chunk of the last segment
    cases = [("first symbol", [(0, 0x01)]), ("last symbol", [(sb - 1, 0x80)]),
             ("low half", [(last + 7, 0x20)]), ("high half", [(last + 40, 0x04)])]
    assert (last + 7) % 64 < 32 <= (last + 40) % 64
    return cases


# ------------------------------------------------------------- one corrupt shard
@pytest.mark.parametrize("n", [1, 3, 9])
@pytest.mark.parametrize("sb", [64, 4096, 20480, 130, 4096 + 34])
def test_rs10_4_one_corrupt_shard(sb, n):
    k, m = 10, 4
    data, par = clean(k, m, sb, n)
    kernels = check(k, m, data, par, [CLEAN] * n)
    assert "verify_compare" in kernels and "k_locate_classify" in kernels and "k_locate_finish" in kernels, kernels
    other = splitmix_bytes(99 + sb, sb)
    for ci, (name, edits) in enumerate(one_shard_cases(sb) + [("whole shard", None)]):
        for j in (0, k - 1):
            s = (ci + j) % n
            broken = data.copy()
            if edits is None:
                broken[s, j] = other  # a whole shard replaced by other bytes
            else:
                for off, mask in edits:
                    broken[s, j, off] ^= mask
            want = [CLEAN] * n
            want[s] = j
            check(k, m, broken, par, want)
    for ci, (name, edits) in enumerate(one_shard_cases(sb)):
        s, r = ci % n, ci % m
        stored = par.copy()
        for off, mask in edits:
            stored[s, r, off] ^= mask
        want = [CLEAN] * n
        want[s] = k + r
        check(k, m, data, stored, want)


@pytest.mark.parametrize("k,m", [(5, 2), (3, 1), (16, 16), (200, 55), (3, 10)])
def test_other_codes(k, m):
    sb, n = 4096, 2
    data, par = clean(k, m, sb, n)
    check(k, m, data, par, [CLEAN, CLEAN])
    for j, off in [(0, 0), (k - 1, sb - 1)]:
        broken = data.copy()
        broken[1, j, off] ^= 0x10
        check(k, m, broken, par, [CLEAN, j if m >= 2 else UNLOCATED])
    for r in {0, m - 1}:
        stored = par.copy()
        stored[0, r, 2049] ^= 0x02
        check(k, m, data, stored, [k + r if m >= 2 else UNLOCATED, CLEAN])


def test_recovery_set():
    k, m, sb, n = 10, 4, 4096, 3
    data, par = clean(k, m, sb, n)
    stored = par.copy()
    stored[1, 0, 100] ^= 0x01
    stored[1, 3, 4000] ^= 0x40
    check(k, m, data, stored, [CLEAN, RECOVERY_SET, CLEAN], bad_recovery=[(1, 0), (1, 3)])


@pytest.mark.parametrize("what", ["two originals, different positions", "two originals, same position",
                                  "original and recovery 2", "original and recovery 0", "all recovery"])
def test_unlocated(what):
    k, m, sb, n = 10, 4, 20480, 3
    data, par = clean(k, m, sb, n)
    broken, stored = data.copy(), par.copy()
    if what.startswith("two originals"):
        broken[1, 2, 17000] ^= 0x08
        broken[1, 7, 17000 if "same" in what else 300] ^= 0x30
    elif what.startswith("original and recovery"):
        broken[1, 4, 555] ^= 0x01
        stored[1, int(what[-1]), 19000] ^= 0x80
    else:
        for r in range(m):
            stored[1, r, 64 * r + 3] ^= 0x02
    check(k, m, broken, stored, [CLEAN, UNLOCATED, CLEAN])


def test_rs3_1_is_unlocated():
    k, m, sb, n = 3, 1, 4096, 2
    data, par = clean(k, m, sb, n)
    broken = data.copy()
    broken[0, 1, 9] ^= 0x01
    stored = par.copy()
    stored[1, 0, 4095] ^= 0x01
    kernels = check(k, m, broken, stored, [UNLOCATED, UNLOCATED])
    assert "k_locate_confirm" not in kernels, kernels  # no ratio to confirm with one recovery shard


# --------------------------------------------------------- every outcome at once
def mixed(k, m, sb):
    """9 stripes of RS(10, 4)-like codes (m >= 4) holding every outcome -> (data, stored, want, bad_recovery)"""
    n = 9
    data, par = clean(k, m, sb, n)
    broken, stored = data.copy(), par.copy()
    want = [CLEAN] * n
    broken[1, 0, sb // 2 + 1] ^= 0x01
    want[1] = 0
    stored[2, 2, sb - 1] ^= 0x10
    want[2] = k + 2
    stored[3, 1, 5] ^= 0x02
    stored[3, 3, sb - 7] ^= 0x04
    want[3] = RECOVERY_SET
    broken[4, 3, 11] ^= 0x20
    broken[4, 8, sb - 11] ^= 0x40
    want[4] = UNLOCATED
    broken[5, k - 1] = splitmix_bytes(4242 + sb, sb)
    want[5] = k - 1
    for r in range(m):
        stored[6, r, 32 * r] ^= 0x08
    want[6] = UNLOCATED
    broken[7, 5, 1] ^= 0x80
    stored[7, 2, sb - 2] ^= 0x01
    want[7] = UNLOCATED
    return broken, stored, want, [(3, 1), (3, 3)]


@pytest.mark.parametrize("sb", [20480, 4096 + 34])
def test_mixed_batch_with_strides(sb):
    """Every outcome in one batch, strided inputs, a present row stride above k + m: the bytes
    between the rows keep their sentinel and the inputs are not written."""
    k, m, n = 10, 4, 9
    broken, stored, want, bad_recovery = mixed(k, m, sb)
    orig_t = torch.from_numpy(splitmix_bytes(5, n * (k + 3) * sb).reshape(n, k + 3, sb)).to(DEV)
    rec_t = torch.from_numpy(splitmix_bytes(6, n * (m + 2) * sb).reshape(n, m + 2, sb)).to(DEV)
    orig_t[:, :k] = torch.from_numpy(broken).to(DEV)
    rec_t[:, :m] = torch.from_numpy(stored).to(DEV)
    orig0, rec0 = orig_t.clone(), rec_t.clone()
    pres_t = torch.full((n, k + m + 5), 7, dtype=torch.uint8, device=DEV)
    counts = torch.zeros(4, dtype=torch.int64, device=DEV)
    located = R.locate_batch_dev(k, m, orig_t[:, :k], rec_t[:, :m], present=pres_t[:, :k + m], counts=counts)
    kernels = ";".join(R.last_kernels())
    torch.cuda.synchronize()
    assert located.cpu().tolist() == want, (located, kernels)
    got = pres_t.cpu().numpy()
    assert (got[:, k + m:] == 7).all()
    assert (got[:, :k + m] == expected_present(k, m, want, bad_recovery)).all(), got
    assert counts.cpu().tolist() == expected_counts(want) == [2, 3, 1, 3]
    assert torch.equal(orig_t, orig0) and torch.equal(rec_t, rec0)
    for name in ("verify_compare", "k_locate_classify", "k_locate_confirm", "k_locate_finish"):
        assert name in kernels, kernels
    assert kernels.index("verify_compare") < kernels.index("k_locate_classify") < \
        kernels.index("k_locate_confirm") < kernels.index("k_locate_finish")


def test_network_and_table_encodes_agree(monkeypatch):
    k, m, sb = 10, 4, 8192
    broken, stored, want, bad_recovery = mixed(k, m, sb)
    k1 = check(k, m, broken, stored, want, bad_recovery)
    monkeypatch.setenv("RS_AMD_JIT", "0")
    k0 = check(k, m, broken, stored, want, bad_recovery)
    assert "rs_net_encode_" in k1 and "rs_net_encode_" not in k0 and "k_locate_confirm" in k0, (k1, k0)


# ------------------------------------------------------------------------ heal
@pytest.mark.parametrize("k,m,sb", [(10, 4, 8192), (200, 55, 4096)])
def test_heal(k, m, sb):
    """scrub -> locate -> reconstruct: the present rows go to rs_reconstruct_batch_dev_patterns
    as they are (max_e = 1) and slot 0 of a stripe with a corrupt original is the clean shard."""
    n = 4
    data, par = clean(k, m, sb, n)
    broken, stored = data.copy(), par.copy()
    hurt = {0: 0, 2: k - 1, 3: k // 2}  # stripe -> corrupt original
    broken[0, 0, 1] ^= 0x01
    broken[2, k - 1] = splitmix_bytes(31 + k, sb)
    broken[3, k // 2, sb - 1] ^= 0x80
    stored[1, m - 1, 123] ^= 0x04  # a recovery shard: e_s = 0, healed by encoding again
    want = [0, k + m - 1, k - 1, k // 2]
    d, p = torch.from_numpy(broken).to(DEV), torch.from_numpy(stored).to(DEV)
    present = torch.zeros((n, k + m), dtype=torch.uint8, device=DEV)
    located = R.locate_batch_dev(k, m, d, p, present=present)
    restored = torch.zeros((n, 1, sb), dtype=torch.uint8, device=DEV)
    status = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    R.reconstruct_batch_dev_patterns(k, m, present, d, p, restored, status=status)
    torch.cuda.synchronize()
    assert located.cpu().tolist() == want
    assert status.cpu().tolist() == [0] * n
    got = restored.cpu().numpy()
    for s, j in hurt.items():
        assert (got[s, 0] == data[s, j]).all(), (s, j)


# ------------------------------------------------------- layouts and slicing
@pytest.mark.parametrize("sb,offset", [(4096, 4), (20480, 4), (130, 2), (4096 + 34, 2)])
def test_unaligned_recovery(sb, offset):
    """The recovery tensor 4 bytes (tails: 2 bytes) past a 16-byte boundary: the dword and byte paths."""
    k, m = 10, 4
    broken, stored, want, bad_recovery = mixed(k, m, sb)
    check(k, m, broken, stored, want, bad_recovery, rec_offset=offset)


def test_slices(monkeypatch):
    """2.25 MiB of parity under a 1 MiB scratch cap: at least 3 slices."""
    monkeypatch.setenv("RS_AMD_JIT", "0")
    monkeypatch.setenv("RS_AMD_SCRATCH_CAP_MB", "1")
    k, m, sb, n = 10, 4, 65536, 9
    data, par = clean(k, m, sb, n)
    broken, stored = data.copy(), par.copy()
    broken[0, 3, 17] ^= 0x10
    stored[4, 1, 65535] ^= 0x10
    broken[8, 9, 30000] ^= 0x10
    want = [3, CLEAN, CLEAN, CLEAN, k + 1, CLEAN, CLEAN, CLEAN, 9]
    kernels = check(k, m, broken, stored, want)
    assert kernels.count("k_locate_finish") >= 3, kernels  # one per slice (only repeats in a row collapse)


def test_flags_are_rejected():
    k, m, sb, n = 10, 4, 4096, 2
    data, par = clean(k, m, sb, n)
    d, p = torch.from_numpy(data.copy()).to(DEV), torch.from_numpy(par.copy()).to(DEV)
    located = torch.full((n,), 77, dtype=torch.int32, device=DEV)
    with pytest.raises(R.InvalidArgument):
        R.locate_batch_dev(k, m, d, p, located=located, flags=3)
    torch.cuda.synchronize()
    assert located.cpu().tolist() == [77, 77]
    assert R.last_kernels() == []


def test_every_allocation_fails_cleanly(monkeypatch):
    """Every allocation of a cold call fails in turn: each call returns OutOfMemory,
    and the library works once disarmed (tests/test_gpu_verify.py's protocol)."""
    monkeypatch.setenv("RS_AMD_JIT", "0")
    k, m, sb, n = 10, 4, 4096, 3
    data, par = clean(k, m, sb, n)
    broken, stored = data.copy(), par.copy()
    broken[0, 6, 5] ^= 0x01
    stored[2, 2, 5] ^= 0x01
    want = [6, CLEAN, k + 2]
    d, p = torch.from_numpy(broken).to(DEV), torch.from_numpy(stored).to(DEV)
    located = torch.zeros((n,), dtype=torch.int32, device=DEV)
    present = torch.zeros((n, k + m), dtype=torch.uint8, device=DEV)
    counts = torch.zeros(4, dtype=torch.int64, device=DEV)

    def call():
        R.locate_batch_dev(k, m, d, p, located=located, present=present, counts=counts)
        torch.cuda.synchronize()

    call()  # kernels loaded
    R.net_wait()
    R.debug_release_caches()
    R.debug_fail_alloc(-1)
    call()  # a cold call: count its allocations
    n_alloc = R.debug_fail_alloc(-1)
    assert n_alloc >= 4, n_alloc  # the encode's plan, the locate plan, the device tables, the scratch
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
    located.fill_(77)
    present.fill_(9)
    call()
    assert located.cpu().tolist() == want
    assert (present.cpu().numpy() == expected_present(k, m, want)).all()
    assert counts.cpu().tolist() == expected_counts(want)
