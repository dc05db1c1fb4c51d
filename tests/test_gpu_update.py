"""Update on the GPU: rs_update_batch_dev patches stored parity in place when originals change.
The expected parity is oracle.encode_batch of the new originals, except for low-rate codes
(unpinned parity), where it is the library's own encode of them. Every case also asserts that
index, old and new are not written. Covers the apply kernel's three access widths, tails, both
forms (old + new, delta), rows with empty slots, more than one tile, per-stripe status, strides,
slicing, the rejections and allocation failures."""
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
NONE = R.UPDATE_NONE


def encode(k, m, data):
    """The parity the update must reproduce for `data` [n, k, sb]"""
    if R.use_high_rate(k, m):
        return O.encode_batch(k, m, data)
    p = torch.zeros((data.shape[0], m, data.shape[2]), dtype=torch.uint8, device=DEV)
    R.encode_batch_dev(k, m, torch.from_numpy(np.ascontiguousarray(data)).to(DEV), p)
    torch.cuda.synchronize()
    return p.cpu().numpy()


@functools.lru_cache(maxsize=None)
def clean(k, m, sb, n):
    """(data [n, k, sb], its parity [n, m, sb]): computed once per shape, never modified."""
    data = splitmix_bytes(k * 1000 + m * 10 + sb + 7, n * k * sb).reshape(n, k, sb)
    par = encode(k, m, data)
    data.setflags(write=False)
    par.setflags(write=False)
    return data, par


def index_tensor(rows):
    return torch.from_numpy(np.array(rows, dtype=np.uint32).view(np.int32)).to(DEV)


def offset_copy(a, offset):
    """a CUDA copy of numpy array `a` that starts `offset` bytes past a 16-byte boundary"""
    if not offset:
        return torch.from_numpy(np.array(a)).to(DEV)
    flat = torch.zeros(a.size + 16, dtype=torch.uint8, device=DEV)
    t = flat[offset:offset + a.size].view(a.shape)
    t.copy_(torch.from_numpy(np.array(a)).to(DEV))
    assert t.data_ptr() % 16 == offset
    return t


def change(k, m, sb, rows, seed=0):
    """rows [n][max_u] of valid indices or NONE -> (old [n, max_u, sb], new, new data [n, k, sb]); the
    shards of empty slots hold bytes that must not matter."""
    n, max_u = len(rows), len(rows[0])
    data, _ = clean(k, m, sb, n)
    new_data = data.copy()
    old = splitmix_bytes(seed + 11, n * max_u * sb).reshape(n, max_u, sb)
    new = splitmix_bytes(seed + 12, n * max_u * sb).reshape(n, max_u, sb)
    for s, row in enumerate(rows):
        for i, j in enumerate(row):
            if j != NONE and j < k:
                old[s, i] = data[s, j]
                new_data[s, j] = new[s, i]
    return old, new, new_data


def update(k, m, sb, rows, delta=False, offset=0, seed=0):
    """Run one update of the clean parity -> (parity after [n, m, sb], status [n], kernels)."""
    n = len(rows)
    old, new, _ = change(k, m, sb, rows, seed)
    _, par = clean(k, m, sb, n)
    idx = index_tensor(rows)
    p = offset_copy(par, offset)
    if delta:
        nw, od = offset_copy(old ^ new, offset), None
    else:
        nw, od = offset_copy(new, offset), offset_copy(old, offset)
    idx0, nw0, od0 = idx.clone(), nw.clone(), None if od is None else od.clone()
    status = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    out = R.update_batch_dev(k, m, idx, nw, p, old=od, status=status)
    kernels = ";".join(R.last_kernels())
    torch.cuda.synchronize()
    assert out.data_ptr() == status.data_ptr()
    assert torch.equal(idx, idx0) and torch.equal(nw, nw0) and (od is None or torch.equal(od, od0))  # inputs unwritten
    return p.cpu().numpy(), status.cpu().tolist(), kernels


def check(k, m, sb, rows, delta=False, offset=0, seed=0):
    """Every row valid: the parity after the update is the encode of the new originals."""
    got, status, kernels = update(k, m, sb, rows, delta, offset, seed)
    want = encode(k, m, change(k, m, sb, rows, seed)[2])
    assert status == [0] * len(rows), (status, kernels)
    bad = np.argwhere((got != want).any(axis=2))
    assert bad.size == 0, (bad.tolist(), kernels)
    return kernels


# ------------------------------------------------------------ load widths and tails
@pytest.mark.parametrize("delta", [False, True], ids=["old_new", "delta"])
@pytest.mark.parametrize("n", [1, 3, 9])
@pytest.mark.parametrize("sb", [64, 4096, 20480, 130, 4096 + 34])
def test_rs10_4_one_original(sb, n, delta):
    k, m = 10, 4
    js = [0, k - 1, 3, 7, 1, 8, 5, 2, 6]  # a different original per stripe, the first and the last among them
    kernels = check(k, m, sb, [[js[s]] for s in range(n)], delta, seed=sb + n)
    assert "k_update_prepare" in kernels and kernels.index("k_update_prepare") < kernels.index("k_update_apply")
    assert ("k_update_apply_x16_t1" if sb % 64 == 0 else "k_update_apply_x1_t1") in kernels, kernels
    if n == 1:
        check(k, m, sb, [[k - 1]], delta, seed=1)


@pytest.mark.parametrize("k,m", [(5, 2), (3, 1), (16, 16), (200, 55), (3, 10)])
def test_other_codes(k, m):
    sb = 4096
    check(k, m, sb, [[0], [k - 1]])
    check(k, m, sb, [[k // 2], [NONE]], delta=True)


# ----------------------------------------------------------------------------- rows
@pytest.mark.parametrize("sb", [4096, 130])
def test_rows_with_empty_slots(sb):
    """max_u = 3 holding 0, 1, 2 and 3 live slots, NONE in first, middle and last position"""
    k, m = 10, 4
    rows = [[NONE, NONE, NONE], [4, NONE, NONE], [NONE, 9, NONE], [NONE, NONE, 0], [2, 7, NONE], [6, NONE, 1],
            [NONE, 3, 8], [5, 0, 9]]
    got, status, kernels = update(k, m, sb, rows)
    assert (got[0] == clean(k, m, sb, len(rows))[1][0]).all()  # the all-NONE stripe is untouched
    assert "_t4" in check(k, m, sb, rows)
    check(k, m, sb, rows, delta=True)


@pytest.mark.parametrize("sb", [4096, 4096 + 34])
def test_second_tile(sb):
    """max_u = 6: rows of 5 and 6 live slots take a second tile of 1 and 2; max_u = k: every original"""
    k, m = 10, 4
    rows = [[1, 3, 5, 7, 9, NONE], [9, 8, 7, 6, 5, 4], [NONE, NONE, 2, NONE, NONE, NONE], [0, NONE, 1, 2, 3, 4],
            [0, 1, 2, 3, NONE, NONE]]
    check(k, m, sb, rows)
    check(k, m, sb, rows, delta=True)
    everything = [list(range(k)), list(range(k - 1, -1, -1))]
    check(k, m, sb, everything)


def test_two_slots_tile():
    k, m, sb = 10, 4, 4096
    assert "_t2" in check(k, m, sb, [[3, 8], [NONE, 0], [9, NONE], [NONE, NONE]])


# ---------------------------------------------------------------- per-stripe status
@pytest.mark.parametrize("sb", [4096, 130])
def test_per_stripe_status(sb):
    k, m = 10, 4
    rows = [[1, NONE, 2], [k, NONE, NONE], [3, 4, 5], [0, k + m, 1], [NONE, 0xFFFFFFFE, NONE], [6, NONE, 6],
            [7, 7, k], [NONE, NONE, 9]]
    want_status = [0, 7, 0, 7, 7, 8, 7, 0]  # stripe 6 has both faults: the invalid index is reported
    got, status, kernels = update(k, m, sb, rows)
    assert status == want_status, (status, kernels)
    _, par = clean(k, m, sb, len(rows))
    want = encode(k, m, change(k, m, sb, rows)[2])
    for s, st in enumerate(want_status):
        assert (got[s] == (want[s] if st == 0 else par[s])).all(), s  # a rejected stripe: no parity byte written
        assert st != 0 or (got[s] != par[s]).any()


# -------------------------------------------------------------------------- strides
@pytest.mark.parametrize("sb", [4096, 4096 + 34])
def test_strides(sb):
    """Parity in [n, m + 2, sb], change buffers in [n, max_u + 1, sb], index rows wider than max_u,
    all filled with a sentinel: every byte outside the addressed rows keeps it."""
    k, m, max_u = 10, 4, 3
    rows = [[2, NONE, 9], [NONE, NONE, NONE], [0, 1, 2], [NONE, 5, NONE]]
    n = len(rows)
    old, new, new_data = change(k, m, sb, rows)
    par = clean(k, m, sb, n)[1]
    par_t = torch.full((n + 1, m + 2, sb), 0xA5, dtype=torch.uint8, device=DEV)
    par_t[:n, :m] = torch.from_numpy(np.array(par)).to(DEV)
    old_t = torch.full((n, max_u + 1, sb), 0x5A, dtype=torch.uint8, device=DEV)
    new_t = torch.full((n, max_u + 1, sb), 0x3C, dtype=torch.uint8, device=DEV)
    old_t[:, :max_u] = torch.from_numpy(old).to(DEV)
    new_t[:, :max_u] = torch.from_numpy(new).to(DEV)
    idx_t = torch.full((n, max_u + 5), 0, dtype=torch.int32, device=DEV)  # 0 past the row: a duplicate if read
    idx_t[:, :max_u] = index_tensor(rows)
    old0, new0, idx0 = old_t.clone(), new_t.clone(), idx_t.clone()
    status = R.update_batch_dev(k, m, idx_t[:, :max_u], new_t[:, :max_u], par_t[:n, :m], old=old_t[:, :max_u])
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * n
    got = par_t.cpu().numpy()
    assert (got[:n, :m] == encode(k, m, new_data)).all()
    assert (got[:n, m:] == 0xA5).all() and (got[n] == 0xA5).all()  # stride padding, the row past the batch
    assert torch.equal(old_t, old0) and torch.equal(new_t, new0) and torch.equal(idx_t, idx0)


# ------------------------------------------------------------------------ alignment
@pytest.mark.parametrize("delta", [False, True], ids=["old_new", "delta"])
@pytest.mark.parametrize("sb,offset,variant", [(4096, 4, "_x4_"), (20480, 4, "_x4_"), (130, 2, "_x1_"),
                                               (4096 + 34, 2, "_x1_")])
def test_unaligned_buffers(sb, offset, variant, delta):
    """Parity, old and new 4 bytes (tails: 2 bytes) past a 16-byte boundary: the dword and byte variants."""
    k, m = 10, 4
    rows = [[3, NONE, 0], [9, 1, 5], [NONE, NONE, NONE], [NONE, 7, NONE], [2, 4, 6]]
    kernels = check(k, m, sb, rows, delta, offset=offset)
    assert "k_update_apply" + variant in kernels, kernels


def test_dword_tail():
    """shard_bytes % 4 == 0 with a tail: whole chunks by dwords, the tail by bytes"""
    assert "_x4_" in check(10, 4, 4096 + 36, [[8, 1], [NONE, 4]])


# ---------------------------------------------------------------------- composition
def test_verify_flags_then_clears():
    """Encode, change originals: verify flags all m rows of the changed stripes; after the update none."""
    k, m, sb = 10, 4, 4096
    rows = [[2, NONE], [NONE, NONE], [9, 0]]
    n = len(rows)
    old, new, new_data = change(k, m, sb, rows)
    data, _ = clean(k, m, sb, n)
    d = torch.from_numpy(np.array(data)).to(DEV)
    p = torch.zeros((n, m, sb), dtype=torch.uint8, device=DEV)
    R.encode_batch_dev(k, m, d, p)
    d.copy_(torch.from_numpy(new_data).to(DEV))
    bad = R.verify_batch_dev(k, m, d, p)
    torch.cuda.synchronize()
    assert bad.cpu().tolist() == [[1] * m, [0] * m, [1] * m]
    R.update_batch_dev(k, m, index_tensor(rows), torch.from_numpy(new).to(DEV), p, old=torch.from_numpy(old).to(DEV))
    bad = R.verify_batch_dev(k, m, d, p)
    torch.cuda.synchronize()
    assert bad.cpu().tolist() == [[0] * m] * n


# --------------------------------------------------------------------------- slices
def test_slices(monkeypatch):
    """RS(200, 55), max_u 4: 21 KB of scratch per stripe, 120 stripes under a 1 MiB cap: 3 slices."""
    monkeypatch.setenv("RS_AMD_SCRATCH_CAP_MB", "1")
    k, m, sb, n = 200, 55, 64, 120
    rows = [[(s * 7) % k, NONE, (s * 7 + 50) % k if s % 3 else NONE, (s * 7 + 100) % k if s % 5 == 0 else NONE]
            for s in range(n)]
    rows[60] = [5, 5, NONE, NONE]  # a rejected stripe in the middle slice
    got, status, kernels = update(k, m, sb, rows)
    assert kernels.count("k_update_apply") >= 3, kernels  # one per slice (prepare in between)
    assert status == [8 if s == 60 else 0 for s in range(n)]
    want = encode(k, m, change(k, m, sb, rows)[2])
    want[60] = clean(k, m, sb, n)[1][60]
    assert (got == want).all(), np.argwhere((got != want).any(axis=2)).tolist()


# ----------------------------------------------------------------------- rejections
def test_rejections():
    k, m, sb, n = 10, 4, 4096, 2
    rows = [[1], [2]]
    old, new, _ = change(k, m, sb, rows)
    par = clean(k, m, sb, n)[1]
    idx, nw, od = index_tensor(rows), torch.from_numpy(new).to(DEV), torch.from_numpy(old).to(DEV)
    p = torch.from_numpy(np.array(par)).to(DEV)
    status = torch.full((n,), 77, dtype=torch.int32, device=DEV)
    for flags in (1, 2, 3):
        with pytest.raises(R.InvalidArgument):
            R.update_batch_dev(k, m, idx, nw, p, old=od, status=status, flags=flags)
        assert R.last_kernels() == []
    # new inside the parity's range: the update would read what it writes
    both = torch.zeros((n, m + 1, sb), dtype=torch.uint8, device=DEV)
    both[:, :m] = p
    both0 = both.clone()
    with pytest.raises(R.InvalidArgument):
        R.update_batch_dev(k, m, idx, both[:, m:], both[:, :m], status=status)
    assert R.last_kernels() == []
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [77, 77]  # nothing written
    assert (p.cpu().numpy() == par).all() and torch.equal(both, both0)


# -------------------------------------------------------------- allocation failures
def test_every_allocation_fails_cleanly():
    """Every allocation of a cold call fails in turn: each call returns OutOfMemory,
    and the library works once disarmed (tests/test_gpu_verify.py's protocol)."""
    k, m, sb = 10, 4, 4096
    rows = [[6, NONE], [NONE, NONE], [0, 9]]
    n = len(rows)
    old, new, new_data = change(k, m, sb, rows)
    par = clean(k, m, sb, n)[1]
    idx, nw, od = index_tensor(rows), torch.from_numpy(new).to(DEV), torch.from_numpy(old).to(DEV)
    p = torch.from_numpy(np.array(par)).to(DEV)
    status = torch.zeros((n,), dtype=torch.int32, device=DEV)

    def call():
        R.update_batch_dev(k, m, idx, nw, p, old=od, status=status)
        torch.cuda.synchronize()

    call()  # kernels loaded
    R.net_wait()
    R.debug_release_caches()
    R.debug_fail_alloc(-1)
    call()  # a cold call: count its allocations
    n_alloc = R.debug_fail_alloc(-1)
    assert n_alloc >= 3, n_alloc  # the plan, the device tables, the scratch
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
    p.copy_(torch.from_numpy(np.array(par)).to(DEV))  # the two successful calls above cancelled each other
    status.fill_(77)
    call()
    assert status.cpu().tolist() == [0] * n
    assert (p.cpu().numpy() == encode(k, m, new_data)).all()
