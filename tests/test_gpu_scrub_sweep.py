"""Position sweeps of the detectors on the GPU (tests/scrub_sweep.py; the CPU side of the same
checker is tests/test_scrub_sweep_model.py): rs_verify_batch_dev and rs_locate_batch_dev see a
flipped bit in every 16-byte slot of a shard, in a recovery shard and in an original, and the
locate's confirm rejects a candidate that is inconsistent in one such slot only. One stripe per
probe, one upload and one library call per sweep and entry point.

Also here, because they share the work-item decomposition (stripe, group of up to 16 rows, 16 KiB
segment): the update at the row-group edges m = 17 and m = 18, compared in full with the oracle,
and every scrub-family kernel past its grid cap of 2^20 work items."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import oracle as O  # noqa: E402
import scrub_sweep as W  # noqa: E402
from helpers import splitmix_bytes  # noqa: E402
from rs_amd import reedsol_amd as R  # noqa: E402

DEV = torch.device("cuda:0")
CLEAN, UNLOCATED, NONE = R.LOCATE_CLEAN, R.LOCATE_UNLOCATED, R.UPDATE_NONE
LOCATE_KERNELS = ("k_verify_compare", "k_locate_classify", "k_locate_confirm", "k_locate_finish")


def upload(a, offset=0):
    """a CUDA copy of numpy array `a` that starts `offset` bytes past a 16-byte boundary"""
    if not offset:
        return torch.from_numpy(np.array(a)).to(DEV)
    flat = torch.zeros(a.size + 16, dtype=torch.uint8, device=DEV)
    t = flat[offset:offset + a.size].view(a.shape)
    t.copy_(torch.from_numpy(np.array(a)).to(DEV))
    assert t.data_ptr() % 16 == offset
    return t


class OnDevice:
    """A sweep uploaded once; verify and locate are the back ends scrub_sweep's checker takes."""

    def __init__(self, sweep, rec_offset=0):
        self.sweep = sweep
        self.d, self.p = upload(sweep.data), upload(sweep.stored, rec_offset)
        self.d0, self.p0 = self.d.clone(), self.p.clone()
        self.kernels = {}

    def unchanged(self):
        return torch.equal(self.d, self.d0) and torch.equal(self.p, self.p0)

    def verify(self, k, m, data, stored):
        assert data is self.sweep.data and stored is self.sweep.stored
        count = torch.full((1,), -1, dtype=torch.int64, device=DEV)
        bad = R.verify_batch_dev(k, m, self.d, self.p, count=count)
        self.kernels["verify"] = ";".join(R.last_kernels())
        torch.cuda.synchronize()
        return bad.cpu().numpy(), int(count.item()), self.unchanged()

    def locate(self, k, m, data, stored):
        assert data is self.sweep.data and stored is self.sweep.stored
        n = data.shape[0]
        located = torch.full((n,), 77, dtype=torch.int32, device=DEV)
        present = torch.full((n, k + m), 9, dtype=torch.uint8, device=DEV)
        counts = torch.full((4,), -1, dtype=torch.int64, device=DEV)
        R.locate_batch_dev(k, m, self.d, self.p, located=located, present=present, counts=counts)
        self.kernels["locate"] = ";".join(R.last_kernels())
        torch.cuda.synchronize()
        return located.cpu().numpy(), present.cpu().numpy(), counts.cpu().tolist(), self.unchanged()

    def locate_multi(self, k, m, data, stored):
        """rs_locate_multi_batch_dev at max_t = 1, for scrub_sweep.multi_as_locate"""
        assert data is self.sweep.data and stored is self.sweep.stored
        n = data.shape[0]
        count = torch.full((n,), 77, dtype=torch.int32, device=DEV)
        located = torch.full((n, 1), 55, dtype=torch.int32, device=DEV)
        present = torch.full((n, k + m), 9, dtype=torch.uint8, device=DEV)
        counts = torch.full((3,), -1, dtype=torch.int64, device=DEV)
        R.locate_multi_batch_dev(k, m, self.d, self.p, 1, count=count, located=located, present=present, counts=counts)
        self.kernels["locate_multi"] = ";".join(R.last_kernels())
        torch.cuda.synchronize()
        return count.cpu().numpy(), located.cpu().numpy(), present.cpu().numpy(), counts.cpu().tolist(), self.unchanged()


def run(sweep, rec_offset=0, verify=True):
    """verify (unless the sweep is locate's alone), locate and the multi-shard locate at max_t = 1
    on one upload of the sweep"""
    dev = OnDevice(sweep, rec_offset)
    if verify:
        W.check_verify(sweep, dev.verify)
        assert "k_verify_compare" in dev.kernels["verify"] and "k_verify_count" in dev.kernels["verify"], dev.kernels
    W.check_locate(sweep, dev.locate)
    for name in LOCATE_KERNELS:
        assert name in dev.kernels["locate"], dev.kernels
    W.check_locate(sweep, W.multi_as_locate(dev.locate_multi), reference=W.MultiCode)
    al = sweep.sb | rec_offset
    check = "k_mloc_check_x16" if al % 16 == 0 else "k_mloc_check_x4" if al % 4 == 0 else "k_mloc_check_x1"
    order = ["k_verify_compare"] + [check, "k_mloc_extend"] * 2 + ["k_mloc_match", "k_mloc_finish"]
    assert dev.kernels["locate_multi"].endswith(";".join(order)), dev.kernels  # max_t + 1 rounds
    return dev


# ------------------------------------------------------------ RS(3, 2): every slot
@functools.lru_cache(maxsize=2)
def rs3_2(sb):
    return W.Batch(3, 2, sb, W.positions(sb))


# name -> (shard bytes, bytes the recovery tensor starts past a 16-byte boundary):
#   aligned  16-byte loads, one whole and one partial segment (16384 + 4096)
#   dword    the same shards, the compare's, classify's and confirm's dword paths
#   bytes    16384 + 4096 + 34: byte loads, a partial last segment, a 17-symbol tail
#   sb2 / sb66 / sb130: tail only, one and two chunks; every byte a probe
SHAPES = {"aligned": (20480, 0), "dword": (20480, 4), "bytes": (20514, 0), "sb2": (2, 0), "sb66": (66, 0),
          "sb130": (130, 0)}


@pytest.mark.parametrize("sweep", ["recovery", "original", "reject"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_rs3_2_every_slot(shape, sweep):
    """recovery / original: every 16-byte slot (and each byte lane and bit) is flipped once in a
    recovery shard and once in an original, for verify and for locate. reject: every slot is once
    the only place where a located candidate is inconsistent."""
    sb, offset = SHAPES[shape]
    batch = rs3_2(sb)
    assert batch.n == len(W.positions(sb)) + 3
    if sweep == "reject":
        run(W.reject_sweep(batch), offset, verify=False)
    else:
        run((W.recovery_sweep if sweep == "recovery" else W.original_sweep)(batch), offset)


# ------------------------------------------------------- wide codes: the row groups
@pytest.mark.parametrize("k,m,sb,rows", [(33, 18, 20480, list(range(1, 18))),
                                         (200, 55, 4096, [1, 16, 17, 32, 33, 48, 49, 54])],
                         ids=["rs33_18", "rs200_55"])
def test_reject_in_every_row_group(k, m, sb, rows):
    """k_locate_confirm walks rows 1.. in groups of 16. m = 18: the full first group and a second
    group of the single row 17; RS(200, 55): both edges of the groups 1-16, 17-32, 33-48, 49-54.
    One probe per (row, segment, 4096-byte pass of the segment)."""
    assert O.use_high_rate(k, m) == 1
    coarse = W.coarse_positions(sb)
    assert len(coarse) == -(-sb // 4096)
    batch = W.Batch(k, m, sb, coarse * len(rows))
    sweep = W.reject_sweep(batch, [r for r in rows for _ in coarse])
    assert sorted({p.shard - k for p in sweep.stripes if p}) == rows
    run(sweep, verify=False)


@pytest.mark.parametrize("sb,offset", [(640, 0), (640, 4), (640 + 34, 0)], ids=["aligned", "dword", "bytes"])
def test_rs200_55_high_byte_first(sb, offset):
    """classify's candidate from a high byte of S_0, whole chunks and tail, in a code where pairing
    a symbol's bytes wrongly changes the answer (scrub_sweep.highbyte_sweep)."""
    k, m = 200, 55
    batch = W.Batch(k, m, sb, W.positions(sb))
    sweep = W.highbyte_sweep(batch)
    assert {p.shard for p in sweep.stripes if p} == set(range(192, 200))
    run(sweep, offset, verify=False)


# -------------------------------------------------------- update at the group edges
@pytest.mark.parametrize("delta", [False, True], ids=["old_new", "delta"])
@pytest.mark.parametrize("u", [1, 3])
@pytest.mark.parametrize("sb", [20480, 20514])
@pytest.mark.parametrize("m", [17, 18])
def test_update_row_group_edges(m, sb, u, delta):
    """k_update_apply walks the recovery rows in groups of 16, B rows in flight: m = 17 leaves a
    last group of one row (every prefetch slot on that row), m = 18 one of two. u = 1: B = 4;
    u = 3: tiles of 3 and of 2 slots, B = 2 and 4. The parity lies in a sentinel-framed allocation
    and is compared in full with the oracle's encode of the new originals."""
    k, n = 33, 3
    assert O.use_high_rate(k, m) == 1
    rows = [[0], [32], [16]] if u == 1 else [[0, 32, 7], [31, NONE, 16], [5, 9, 20]]
    data = splitmix_bytes(m * 100 + sb + u, n * k * sb).reshape(n, k, sb)
    new = splitmix_bytes(m * 100 + sb + u + 1, n * u * sb).reshape(n, u, sb)
    old = splitmix_bytes(m * 100 + sb + u + 2, n * u * sb).reshape(n, u, sb)  # empty slots: bytes that must not matter
    new_data = data.copy()
    for s, row in enumerate(rows):
        for i, j in enumerate(row):
            if j != NONE:
                old[s, i] = data[s, j]
                new_data[s, j] = new[s, i]
    par_t = torch.full((n + 1, m + 2, sb), 0xA5, dtype=torch.uint8, device=DEV)
    par_t[:n, :m] = upload(O.encode_batch(k, m, data))
    idx = torch.from_numpy(np.array(rows, dtype=np.uint32).view(np.int32)).to(DEV)
    nw, od = (upload(old ^ new), None) if delta else (upload(new), upload(old))
    idx0, nw0, od0 = idx.clone(), nw.clone(), None if od is None else od.clone()
    status = R.update_batch_dev(k, m, idx, nw, par_t[:n, :m], old=od)
    kernels = ";".join(R.last_kernels())
    torch.cuda.synchronize()
    assert f"k_update_apply_{'x16' if sb % 16 == 0 else 'x1'}_t{1 if u == 1 else 4}" in kernels, kernels
    assert status.cpu().tolist() == [0] * n
    got, want = par_t.cpu().numpy(), O.encode_batch(k, m, new_data)
    bad = np.argwhere(got[:n, :m] != want)
    assert bad.size == 0, (f"{len(bad)} bytes, first (stripe, row, offset) {bad[0].tolist()}", kernels)
    assert (got[:n, m:] == 0xA5).all() and (got[n] == 0xA5).all()  # stride padding, the row past the batch
    assert torch.equal(idx, idx0) and torch.equal(nw, nw0) and (od is None or torch.equal(od, od0))


# ----------------------------------------------------------------- past the grid cap
N_BIG = (1 << 20) + 5  # every scrub-family launch caps its grid at 2^20 work items


def encode_columns(data):
    """The parity of RS(2, 2) stripes [n, 2, 64] by one oracle encode of the stripes laid side by
    side as columns ([2, n * 64]): 64-byte chunks are independent (tests/test_oracle_golden.py)."""
    n = data.shape[0]
    st, rec = O.encode(2, 2, np.ascontiguousarray(data.transpose(1, 0, 2)).reshape(2, n * 64))
    assert st == 0
    return np.ascontiguousarray(rec.reshape(2, n, 64).transpose(1, 0, 2))


@functools.lru_cache(maxsize=1)
def big():
    data = splitmix_bytes(2264, N_BIG * 2 * 64).reshape(N_BIG, 2, 64)
    par = encode_columns(data)
    for s0 in (0, N_BIG - 1000):
        assert (par[s0:s0 + 1000] == O.encode_batch(2, 2, data[s0:s0 + 1000])).all()
    data.setflags(write=False)
    par.setflags(write=False)
    return data, par


def test_past_the_grid_cap_verify_and_locate():
    """RS(2, 2), 64-byte shards, 2^20 + 5 stripes: k_verify_compare (2 n work items), k_verify_count
    (n m > 2^18 threads), k_locate_classify and k_locate_confirm (n work items each; the two
    corrupt originals lie in stripes 2^20 and 2^20 + 1, which only the second trip reaches) all go
    round their grid-stride loops again. k_locate_finish would need n (k + m) > 2^24 elements with a
    present row: out of scope at this size."""
    k, m, n = 2, 2, N_BIG
    data, par = big()
    broken, stored = data.copy(), par.copy()
    flags = np.zeros((n, m), np.uint8)
    located = np.full(n, CLEAN, np.int32)
    for i, s in enumerate((0, 1 << 19, (1 << 20) - 1, (1 << 20) + 4)):
        r = i % m
        stored[s, r, (i * 21 + 5) % 64] ^= 1 << i
        flags[s, r], located[s] = 1, k + r
    for i, s in enumerate((1 << 20, (1 << 20) + 1)):
        broken[s, i, 40 - 33 * i] ^= 0x10 << i
        flags[s], located[s] = 1, i
    d, p = upload(broken), upload(stored)
    d0, p0 = d.clone(), p.clone()
    count = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    bad = R.verify_batch_dev(k, m, d, p, count=count)
    kernels = ";".join(R.last_kernels())
    assert "k_verify_compare" in kernels and "k_verify_count" in kernels, kernels
    got = bad.cpu().numpy()
    assert np.array_equal(got, flags), np.argwhere(got != flags)[:8].tolist()
    assert int(count.item()) == int(flags.sum()) == 4 + 2 * m

    loc_t = torch.full((n,), 77, dtype=torch.int32, device=DEV)
    present = torch.full((n, k + m), 9, dtype=torch.uint8, device=DEV)
    counts = torch.full((4,), -1, dtype=torch.int64, device=DEV)
    R.locate_batch_dev(k, m, d, p, located=loc_t, present=present, counts=counts)
    kernels = ";".join(R.last_kernels())
    for name in LOCATE_KERNELS:
        assert name in kernels, kernels
    got = loc_t.cpu().numpy()
    assert np.array_equal(got, located), [(int(s), int(got[s]), int(located[s])) for s in np.flatnonzero(got != located)[:8]]
    want_present = np.ones((n, k + m), np.uint8)
    want_present[np.flatnonzero(located >= 0), located[located >= 0]] = 0
    assert np.array_equal(present.cpu().numpy(), want_present)
    assert counts.cpu().tolist() == W.class_counts(located) == [n - 6, 6, 0, 0]
    assert torch.equal(d, d0) and torch.equal(p, p0)


def test_past_the_grid_cap_update():
    """u = 1 on all 2^20 + 5 stripes, the index rotating over the two originals: k_update_prepare and
    k_update_apply (n work items each) take a second trip; the parity equals the oracle's of the
    new data on every stripe."""
    k, m, n = 2, 2, N_BIG
    data, par = big()
    which = (np.arange(n) % 2).astype(np.uint32)
    new = splitmix_bytes(2265, n * 64).reshape(n, 1, 64)
    old = np.ascontiguousarray(data[np.arange(n), which])[:, None, :]
    new_data = data.copy()
    new_data[np.arange(n), which] = new[:, 0]
    p, want = upload(par), upload(encode_columns(new_data))
    idx, nw, od = torch.from_numpy(which.view(np.int32).reshape(n, 1)).to(DEV), upload(new), upload(old)
    idx0, nw0, od0 = idx.clone(), nw.clone(), od.clone()
    status = R.update_batch_dev(k, m, idx, nw, p, old=od)
    kernels = ";".join(R.last_kernels())
    assert "k_update_prepare" in kernels and "k_update_apply_x16_t1" in kernels, kernels
    assert not status.any().item()
    differ = (p != want).flatten(1).any(dim=1)
    assert not differ.any().item(), differ.nonzero().flatten()[:8].tolist()
    assert torch.equal(idx, idx0) and torch.equal(nw, nw0) and torch.equal(od, od0)
