"""Multi-shard locate on the GPU: rs_locate_multi_batch_dev names the set of shards each test
corrupts. The expected answer is known by construction; the clean parity is oracle.encode_batch,
except for low-rate codes (unpinned parity), where it is the library's own encode. Covers the
check's three load widths, tails, segment boundaries, every set shape, rank-deficient and
over-rank stripes, strides, slicing, the heal through rs_rebuild_batch_dev, agreement with
rs_locate_batch_dev and allocation failures. Every stripe of every batch is compared."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import oracle as O  # noqa: E402
from helpers import splitmix_bytes  # noqa: E402
from locate_model import symbol_bytes  # noqa: E402
from rs_amd import reedsol_amd as R  # noqa: E402

DEV = torch.device("cuda:0")
UNLOCATED = R.LOCATE_UNLOCATED


@functools.lru_cache(maxsize=None)
def clean(k, m, sb, n):
    """(data [n, k, sb], its clean parity [n, m, sb]): computed once per shape, never modified."""
    data = splitmix_bytes(k * 1000 + m * 10 + sb + 1, n * k * sb).reshape(n, k, sb)
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


def shard(k, broken, stored, s, i):
    """the bytes of shard i in [0, k + m) of stripe s"""
    return broken[s, i] if i < k else stored[s, i - k]


def xor_symbol(row, q, err):
    lo, hi = symbol_bytes(row.shape[0], q)
    row[lo] ^= err & 0xFF
    row[hi] ^= err >> 8


def locate(k, m, max_t, data, stored, rec_offset=0):
    """-> (count [n], located [n, max_t], present [n, k + m], counts [max_t + 2], the kernels the
    call launched). rec_offset: the recovery tensor starts that many bytes past a 16-byte boundary."""
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
    count = torch.full((n,), 77, dtype=torch.int32, device=DEV)
    located = torch.full((n, max_t), 55, dtype=torch.int32, device=DEV)
    present = torch.full((n, k + m), 9, dtype=torch.uint8, device=DEV)
    counts = torch.full((max_t + 2,), -1, dtype=torch.int64, device=DEV)
    out = R.locate_multi_batch_dev(k, m, d, p, max_t, count=count, located=located, present=present, counts=counts)
    kernels = ";".join(R.last_kernels())
    torch.cuda.synchronize()
    assert out.data_ptr() == count.data_ptr() and out.dtype == torch.int32
    assert torch.equal(d, d0) and torch.equal(p, p0)  # no input is written
    return count.cpu().numpy(), located.cpu().numpy(), present.cpu().numpy(), counts.cpu().tolist(), kernels


def expected(k, m, max_t, sets):
    """sets: per stripe the corrupt shards (any order) or None for an unlocated stripe ->
    (count, located rows, present rows, counts)"""
    n = len(sets)
    count = np.array([UNLOCATED if T is None else len(T) for T in sets], np.int32)
    located = np.full((n, max_t), -1, np.int32)
    present = np.ones((n, k + m), np.uint8)
    counts = [0] * (max_t + 2)
    for s, T in enumerate(sets):
        counts[max_t + 1 if T is None else len(T)] += 1
        for q, i in enumerate(sorted(T or [])):
            located[s, q] = i
            present[s, i] = 0
    return count, located, present, counts


def check(k, m, max_t, data, stored, sets, rec_offset=0):
    count, located, present, counts, kernels = locate(k, m, max_t, data, stored, rec_offset)
    want = expected(k, m, max_t, sets)
    assert count.tolist() == want[0].tolist(), (count, sets, kernels)
    assert (located == want[1]).all(), (located, sets)
    assert (present == want[2]).all(), present
    assert counts == want[3], counts
    return kernels


def one_shard_cases(sb):
    """(name, offsets and masks) of the corruptions of one shard"""
    whole = sb - sb % 64
    last = whole - 64  # a whole chunk of the last segment
    cases = [("first symbol", [(0, 0x01)]), ("last symbol", [(sb - 1, 0x80)]),
             ("low half", [(last + 7, 0x20)]), ("high half", [(last + 40, 0x04)])]
    assert (last + 7) % 64 < 32 <= (last + 40) % 64
    return cases


def width(sb, rec_offset=0):
    """the check kernel the alignment of an otherwise 16-byte-aligned call selects"""
    al = sb | rec_offset
    return "k_mloc_check_x16" if al % 16 == 0 else "k_mloc_check_x4" if al % 4 == 0 else "k_mloc_check_x1"


# ------------------------------------------------------------- RS(10, 4), max_t 2
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("sb", [64, 4096, 20480, 130, 4096 + 34])
def test_rs10_4_up_to_two_corrupt_shards(sb, n):
    k, m, max_t = 10, 4, 2
    data, par = clean(k, m, sb, n)
    kernels = check(k, m, max_t, data, par, [[]] * n)
    order = ["k_verify_compare"] + [width(sb), "k_mloc_extend"] * (max_t + 1) + ["k_mloc_match", "k_mloc_finish"]
    assert kernels.endswith(";".join(order)), kernels  # max_t + 1 rounds, whatever the batch holds
    cases = one_shard_cases(sb)
    # t = 1: an original, a recovery shard
    for ci, (name, edits) in enumerate(cases):
        for i in (0, k - 1, k + ci % m):
            s = (ci + i) % n
            broken, stored = data.copy(), par.copy()
            for off, mask in edits:
                shard(k, broken, stored, s, i)[off] ^= mask
            sets = [[]] * n
            sets[s] = [i]
            check(k, m, max_t, broken, stored, sets)
    # t = 2 over {original, original}, {original, recovery}, {recovery, recovery}
    for pi, (a, b) in enumerate([(2, 7), (k - 1, k + 1), (k, k + m - 1)]):
        s = pi % n
        sets = [[]] * n
        sets[s] = [a, b]
        # both wrong at the same four symbols: a with the cases' masks, b with the same mask at the
        # first symbol and another one elsewhere, so the two error rows are not proportional
        broken, stored = data.copy(), par.copy()
        for ci, (name, edits) in enumerate(cases):
            for off, mask in edits:
                shard(k, broken, stored, s, a)[off] ^= mask
                shard(k, broken, stored, s, b)[off] ^= mask if ci == 0 else mask ^ 0xFF
        check(k, m, max_t, broken, stored, sets)
        # different symbols only: a at the first symbol, b in the last chunk and at the last symbol
        # (at 20480: a in segment 0, b in segment 1, so the second pivot is found a round later)
        broken, stored = data.copy(), par.copy()
        for ci, (name, edits) in enumerate(cases):
            for off, mask in edits:
                shard(k, broken, stored, s, a if ci == 0 else b)[off] ^= mask
        if sb == 20480:
            assert cases[0][1][0][0] < 16384 <= min(off for _, e in cases[1:] for off, _ in e)
        check(k, m, max_t, broken, stored, sets)
    # a whole shard replaced, and one bit flipped in another
    s = n - 1
    broken, stored = data.copy(), par.copy()
    broken[s, 4] = splitmix_bytes(99 + sb, sb)
    stored[s, 2, sb // 2] ^= 0x10
    sets = [[]] * n
    sets[s] = [4, k + 2]
    check(k, m, max_t, broken, stored, sets)


# ------------------------------------------------------- unlocated, deterministic
def test_rank_above_max_t_is_unlocated():
    """three corrupt shards, each with its single flipped symbol at a different position: rank 3"""
    k, m, sb, n, max_t = 10, 4, 20480, 3, 2
    data, par = clean(k, m, sb, n)
    broken, stored = data.copy(), par.copy()
    broken[1, 2, 300] ^= 0x08
    broken[1, 7, 17000] ^= 0x30
    stored[1, 3, 9000] ^= 0x01
    check(k, m, max_t, broken, stored, [[], None, []])


@pytest.mark.parametrize("a,b", [(1, 8), (3, 10 + 2), (10, 10 + 3)])
def test_rank_deficient_pair_is_unlocated(a, b):
    """err_b(p) = alpha * err_a(p) at every symbol p: rank 1, and no single shard explains it"""
    k, m, sb, n, max_t = 10, 4, 4096 + 34, 2, 2
    data, par = clean(k, m, sb, n)
    broken, stored = data.copy(), par.copy()
    alpha_log = 12345
    for q, e in [(0, 0x0001), (700, 0xBEEF), (sb // 2 - 1, 0x8000), (2048 + 3, 0x0100)]:  # whole chunks and the tail
        xor_symbol(shard(k, broken, stored, 0, a), q, e)
        xor_symbol(shard(k, broken, stored, 0, b), q, O.mul16(e, alpha_log))
    check(k, m, max_t, broken, stored, [None, []])


# ------------------------------------------------------------------ other codes
def spread(k, broken, stored, s, T, seed):
    """shard T[i] alone is wrong at a symbol of its own (so the errors have rank len(T)), and each
    is wrong at random other symbols"""
    rng = np.random.default_rng(seed)
    P = broken.shape[2] // 2
    own = rng.permutation(P)[:len(T)]
    free = np.setdiff1d(np.arange(P), own)
    for i, sh in enumerate(T):
        row = shard(k, broken, stored, s, sh)
        xor_symbol(row, int(own[i]), int(rng.integers(1, 65536)))
        for q in rng.choice(free, 20, replace=False):
            xor_symbol(row, int(q), int(rng.integers(1, 65536)))


@pytest.mark.parametrize("k,m,max_t,sets", [
    (5, 2, 1, [[3], [5 + 1]]),
    (16, 16, 8, [[0, 3, 15, 16, 17, 20, 30, 31], [5, 16 + 9, 16 + 15]]),
    (200, 55, 3, [[0, 199, 200 + 54], [77, 200]]),
    (3, 10, 5, [[0, 2, 3, 3 + 4, 3 + 9], [1]]),
])
def test_other_codes(k, m, max_t, sets):
    sb, n = 4096, 2
    data, par = clean(k, m, sb, n)
    check(k, m, max_t, data, par, [[], []])
    broken, stored = data.copy(), par.copy()
    for s, T in enumerate(sets):
        spread(k, broken, stored, s, T, seed=k + s)
    check(k, m, max_t, broken, stored, sets)
    if len(sets[0]) > 1:  # one shard fewer than the rank allowed: unlocated, the other stripe unchanged
        count, located, _, _, _ = locate(k, m, len(sets[0]) - 1, broken, stored)
        assert count[0] == UNLOCATED and (located[0] == -1).all()
        assert count[1] == (len(sets[1]) if len(sets[1]) < len(sets[0]) else UNLOCATED)


# ------------------------------------------------------------------ load widths
def mixed(k, m, sb):
    """6 stripes of an RS(10, 4)-like code holding clean, t = 1, t = 2 and unlocated stripes
    -> (data, stored, sets)"""
    n = 6
    data, par = clean(k, m, sb, n)
    broken, stored = data.copy(), par.copy()
    sets = [[] for _ in range(n)]
    broken[1, 0, sb // 2 + 1] ^= 0x01
    sets[1] = [0]
    stored[2, 1, 5] ^= 0x02
    stored[2, 3, sb - 7] ^= 0x04
    sets[2] = [k + 1, k + 3]
    broken[3, 3, 11] ^= 0x20
    broken[3, 8, sb - 11] ^= 0x40
    sets[3] = [3, 8]
    for r in range(3):  # three shards, three symbols: rank 3
        stored[4, r, 64 * r + 3] ^= 0x08
    sets[4] = None
    broken[5, k - 1] = splitmix_bytes(4242 + sb, sb)
    stored[5, 0, sb - 2] ^= 0x01
    sets[5] = [k - 1, k]
    return broken, stored, sets


@pytest.mark.parametrize("offset", [4, 8])
@pytest.mark.parametrize("sb", [4096, 4096 + 34])
def test_unaligned_recovery(sb, offset):
    """The recovery tensor 4 and 8 bytes past a 16-byte boundary: the dword and the byte loads."""
    k, m, max_t = 10, 4, 2
    broken, stored, sets = mixed(k, m, sb)
    kernels = check(k, m, max_t, broken, stored, sets, rec_offset=offset)
    assert width(sb, offset) in kernels and width(sb, offset) != "k_mloc_check_x16", kernels
    for name in ("verify_compare", "k_mloc_extend", "k_mloc_match", "k_mloc_finish"):
        assert name in kernels, kernels


# ---------------------------------------------------------------------- strides
@pytest.mark.parametrize("sb", [20480, 4096 + 34])
def test_mixed_batch_with_strides(sb):
    """Clean, t = 1, t = 2 and unlocated stripes in one batch, strided inputs, located and present
    rows with strides above max_t and k + m: the words and bytes between the rows keep their
    sentinel and the inputs are not written."""
    k, m, max_t = 10, 4, 2
    broken, stored, sets = mixed(k, m, sb)
    n = len(sets)
    orig_t = torch.from_numpy(splitmix_bytes(5, n * (k + 3) * sb).reshape(n, k + 3, sb)).to(DEV)
    rec_t = torch.from_numpy(splitmix_bytes(6, n * (m + 2) * sb).reshape(n, m + 2, sb)).to(DEV)
    orig_t[:, :k] = torch.from_numpy(broken).to(DEV)
    rec_t[:, :m] = torch.from_numpy(stored).to(DEV)
    orig0, rec0 = orig_t.clone(), rec_t.clone()
    loc_t = torch.full((n, max_t + 3), 1234, dtype=torch.int32, device=DEV)
    pres_t = torch.full((n, k + m + 5), 7, dtype=torch.uint8, device=DEV)
    counts = torch.full((max_t + 2,), -1, dtype=torch.int64, device=DEV)
    count = R.locate_multi_batch_dev(k, m, orig_t[:, :k], rec_t[:, :m], max_t, located=loc_t[:, :max_t],
                                     present=pres_t[:, :k + m], counts=counts)
    torch.cuda.synchronize()
    want = expected(k, m, max_t, sets)
    assert count.cpu().tolist() == want[0].tolist()
    loc, pres = loc_t.cpu().numpy(), pres_t.cpu().numpy()
    assert (loc[:, max_t:] == 1234).all() and (pres[:, k + m:] == 7).all()
    assert (loc[:, :max_t] == want[1]).all(), loc
    assert (pres[:, :k + m] == want[2]).all(), pres
    assert counts.cpu().tolist() == want[3] == [1, 1, 3, 1]
    assert torch.equal(orig_t, orig0) and torch.equal(rec_t, rec0)


def test_count_alone():
    """d_located, d_present and d_counts are optional"""
    k, m, sb, max_t = 10, 4, 4096, 2
    broken, stored, sets = mixed(k, m, sb)
    count = R.locate_multi_batch_dev(k, m, torch.from_numpy(broken).to(DEV), torch.from_numpy(stored).to(DEV), max_t)
    torch.cuda.synchronize()
    assert count.cpu().tolist() == expected(k, m, max_t, sets)[0].tolist()


# ---------------------------------------------------------------------- slicing
@pytest.mark.parametrize("sb,slices", [(20480, 1), (65536, 3)])
def test_slices(monkeypatch, sb, slices):
    """9 stripes under a 1 MiB scratch cap: at 64 KiB shards at least 3 slices (at 20 KiB the batch
    still fits one). The answers equal those of the uncapped call."""
    monkeypatch.setenv("RS_AMD_JIT", "0")
    k, m, n, max_t = 10, 4, 9, 2
    data, par = clean(k, m, sb, n)
    broken, stored = data.copy(), par.copy()
    sets = [[] for _ in range(n)]
    broken[0, 3, 17] ^= 0x10
    sets[0] = [3]
    stored[4, 1, sb - 1] ^= 0x10
    broken[4, 0, 16384 + 5] ^= 0x01
    sets[4] = [0, k + 1]
    for j in (1, 2, 3):
        broken[6, j, 64 * j] ^= 0x02
    sets[6] = None
    broken[8, 9, sb // 2] ^= 0x10
    broken[8, 8, 3] ^= 0x10
    sets[8] = [8, 9]
    whole = locate(k, m, max_t, broken, stored)
    monkeypatch.setenv("RS_AMD_SCRATCH_CAP_MB", "1")
    kernels = check(k, m, max_t, broken, stored, sets)
    capped = locate(k, m, max_t, broken, stored)
    for x, y in zip(whole[:3], capped[:3]):
        assert (x == y).all()
    assert whole[3] == capped[3]
    assert kernels.count("k_mloc_finish") >= slices, kernels  # one per slice (only repeats in a row collapse)
    assert whole[4].count("k_mloc_finish") == 1, whole[4]


# ------------------------------------------------------------------------- heal
@pytest.mark.parametrize("k,m,sb,max_t", [(10, 4, 8192, 2), (200, 55, 4096, 3)])
def test_heal(k, m, sb, max_t):
    """scrub -> locate -> rebuild: the present rows go to rs_rebuild_batch_dev as they are
    (max_e = max_t) and the rebuilt slots are the clean shards, originals first."""
    n = 4
    data, par = clean(k, m, sb, n)
    broken, stored = data.copy(), par.copy()
    sets = [[0, k - 1], [k + m - 1], [], sorted([k // 2, k, k + 1][:max_t])]
    for s, T in enumerate(sets):
        spread(k, broken, stored, s, T, seed=100 + s)
    d, p = torch.from_numpy(broken).to(DEV), torch.from_numpy(stored).to(DEV)
    present = torch.zeros((n, k + m), dtype=torch.uint8, device=DEV)
    count = R.locate_multi_batch_dev(k, m, d, p, max_t, present=present)
    rebuilt = torch.zeros((n, max_t, sb), dtype=torch.uint8, device=DEV)
    status = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    R.rebuild_batch_dev(k, m, present, d, p, rebuilt, status=status)
    torch.cuda.synchronize()
    assert count.cpu().tolist() == [len(T) for T in sets]
    assert status.cpu().tolist() == [0] * n
    got = rebuilt.cpu().numpy()
    for s, T in enumerate(sets):
        for slot, i in enumerate(T):
            assert (got[s, slot] == (data[s, i] if i < k else par[s, i - k])).all(), (s, i)
        assert (got[s, len(T):] == 0).all()  # the other slots are not written


# ---------------------------------------------------------- agreement with locate
@pytest.mark.parametrize("sb", [4096, 20480 + 2])
def test_agrees_with_locate(sb):
    """<= 1 corrupt shard per stripe: rs_locate_batch_dev names the same shard. A stripe with two
    bad recovery shards: the multi form names the rows whose present flag locate cleared."""
    k, m, n, max_t = 10, 4, 6, 2
    data, par = clean(k, m, sb, n)
    broken, stored = data.copy(), par.copy()
    broken[0, 6, 5] ^= 0x01
    stored[2, 2, sb - 1] ^= 0x40
    broken[3, 0] = splitmix_bytes(17 + sb, sb)
    stored[4, 0, 100] ^= 0x01
    stored[4, 3, sb - 100] ^= 0x40
    broken[5, k - 1, sb // 2] ^= 0x80
    sets = [[6], [], [k + 2], [0], [k, k + 3], [k - 1]]
    d, p = torch.from_numpy(broken).to(DEV), torch.from_numpy(stored).to(DEV)
    pres1 = torch.zeros((n, k + m), dtype=torch.uint8, device=DEV)
    pres2 = torch.zeros((n, k + m), dtype=torch.uint8, device=DEV)
    loc2 = torch.zeros((n, max_t), dtype=torch.int32, device=DEV)
    loc1 = R.locate_batch_dev(k, m, d, p, present=pres1)
    count = R.locate_multi_batch_dev(k, m, d, p, max_t, located=loc2, present=pres2)
    torch.cuda.synchronize()
    assert loc1.cpu().tolist() == [6, R.LOCATE_CLEAN, k + 2, 0, R.LOCATE_RECOVERY_SET, k - 1]
    want = expected(k, m, max_t, sets)
    assert count.cpu().tolist() == want[0].tolist() and (loc2.cpu().numpy() == want[1]).all()
    assert torch.equal(pres1, pres2) and (pres2.cpu().numpy() == want[2]).all()
    for s, one in enumerate(loc1.cpu().tolist()):
        if one >= 0:
            assert loc2[s].cpu().tolist() == [one, -1]


# ---------------------------------------------------------- allocation failures
def test_every_allocation_fails_cleanly(monkeypatch):
    """Every allocation of a cold call fails in turn: each call returns OutOfMemory,
    and the library works once disarmed (tests/test_gpu_verify.py's protocol)."""
    monkeypatch.setenv("RS_AMD_JIT", "0")
    k, m, sb, max_t = 10, 4, 4096, 2
    broken, stored, sets = mixed(k, m, sb)
    n = len(sets)
    d, p = torch.from_numpy(broken).to(DEV), torch.from_numpy(stored).to(DEV)
    count = torch.zeros((n,), dtype=torch.int32, device=DEV)
    located = torch.zeros((n, max_t), dtype=torch.int32, device=DEV)
    present = torch.zeros((n, k + m), dtype=torch.uint8, device=DEV)
    counts = torch.zeros(max_t + 2, dtype=torch.int64, device=DEV)

    def call():
        R.locate_multi_batch_dev(k, m, d, p, max_t, count=count, located=located, present=present, counts=counts)
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
    count.fill_(77)
    located.fill_(55)
    present.fill_(9)
    call()
    want = expected(k, m, max_t, sets)
    assert count.cpu().tolist() == want[0].tolist()
    assert (located.cpu().numpy() == want[1]).all()
    assert (present.cpu().numpy() == want[2]).all()
    assert counts.cpu().tolist() == want[3]
