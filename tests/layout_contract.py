"""The layout contract of the device entry points (include/reedsol.h): whole-chunk shards need
4-byte-aligned pointers and stripe strides, 16-byte alignment is only what the fastest kernels
need, and a narrower layout computes the same bytes on the table kernels without touching
anything outside the documented rows. Next to slot_contract.py, whose check_reconstruct the
reconstruct cases go through; this module adds

  * the layout classes: per buffer a byte offset of the base and a residue (mod 16) of the
    stripe stride, and the widest lane (`max_nv` dword pairs) the class still allows;
  * place(): an array laid into a guard-framed flat device allocation at such an offset, so
    that a write before the first or past the last row is seen;
  * check_encode(): the encode's counterpart of check_reconstruct, array-agnostic
    (tests/test_layout_contract_model.py runs it on the oracle and proves that it rejects wrong
    backends; tests/test_gpu_layouts.py runs it on the GPU).

An encode backend is a callable run(orig, par_init) -> (orig_after, par_after) over numpy uint8
arrays with one row per stripe, the row length being the stripe stride:
  orig [n, k * sb + pad], par_init [n + 1, m * sb + pad]
(par_init's last row is a guard stripe past the batch)."""
import collections
import re

import numpy as np

from slot_contract import GUARD, _strided, _where

FRAME = 0x3C        # fills the 32 bytes around a placed array
FRAME_BYTES = 32
BUFFERS = ("original", "recovery", "restored")  # an encode has the first two: its parity is d_recovery
HIPRTC = ("rs_net_", "rs_fft_", "rs_psyn")       # kernels that need 16-byte alignment throughout

# offsets / residues: one per buffer of BUFFERS
Layout = collections.namedtuple("Layout", "name offsets residues max_nv")

ALIGNED = Layout("aligned", (0, 0, 0), (0, 0, 0), 4)


def _one(which, value):
    i = BUFFERS.index(which)
    return tuple(value if j == i else 0 for j in range(3))


def layout(cls, which=None):
    """A8 / A4: every buffer at base + 8 / + 4 with a stride of that residue mod 16 (A4: 4 and
    12 across the buffers). ONE8 / ONE4: only the buffer `which` at + 8 / + 4, strides
    unchanged. STRIDE4: only the stride of `which`, = 4 mod 16. ALIGNED: the control."""
    if cls == "ALIGNED":
        return ALIGNED
    if cls == "A8":
        return Layout(cls, (8, 8, 8), (8, 8, 8), 2)
    if cls == "A4":
        return Layout(cls, (4, 4, 4), (4, 12, 4), 1)
    assert which in BUFFERS, which
    if cls == "ONE8":
        return Layout(f"{cls}-{which}", _one(which, 8), (0, 0, 0), 2)
    if cls == "ONE4":
        return Layout(f"{cls}-{which}", _one(which, 4), (0, 0, 0), 1)
    if cls == "STRIDE4":
        return Layout(f"{cls}-{which}", (0, 0, 0), _one(which, 4), 1)
    raise KeyError(cls)


def align_nv(values):
    """The library's rule (rs_common.cpp align_nv), restated: the widest lane, in dword pairs,
    that every pointer and stride of a call allows; 0: the call is rejected."""
    a = 0
    for v in values:
        a |= int(v)
    return 4 if a % 16 == 0 else 2 if a % 8 == 0 else 1 if a % 4 == 0 else 0


def pads_for(lay, base=(256, 128, 64)):
    """Stride paddings (original, recovery, restored) of the layout on top of 16-byte-multiple
    base paddings: with rows of whole 64-byte chunks the stride then has the class's residue."""
    assert all(b % 16 == 0 for b in base)
    return tuple(b + r for b, r in zip(base, lay.residues))


class Placed:
    """A host array [n, stride] in a flat device allocation FRAME_BYTES larger, filled with
    FRAME, the array starting `offset` bytes in. t: the 2-D device view to hand to a call."""

    def __init__(self, arr, offset, device):
        import torch
        assert 0 <= offset < FRAME_BYTES and arr.ndim == 2 and arr.dtype == np.uint8
        self.offset, self.size = offset, arr.size
        self.flat = torch.full((arr.size + FRAME_BYTES,), FRAME, dtype=torch.uint8, device=device)
        assert self.flat.data_ptr() % 16 == 0
        self.t = self.flat[offset:offset + arr.size].view(arr.shape)
        self.t.copy_(torch.from_numpy(arr))
        assert self.t.data_ptr() % 16 == offset % 16 and self.t.stride(0) == arr.shape[1]

    def frame_errors(self, what):
        flat = self.flat.cpu().numpy()
        lead, trail = flat[:self.offset], flat[self.offset + self.size:]
        out = []
        if (lead != FRAME).any():
            out.append(f"{what}: bytes before the first row were written ({_where(lead != FRAME)})")
        if (trail != FRAME).any():
            out.append(f"{what}: bytes past the last row were written ({_where(trail != FRAME)})")
        return out

    def numpy(self):
        return self.t.cpu().numpy()


def place(arrays, lay, device, buffers=BUFFERS):
    """Each array of `arrays` (in the order of `buffers`) placed at the layout's offset for its
    buffer (Placed asserts the base's residue mod 16)."""
    return [Placed(arr, lay.offsets[BUFFERS.index(name)], device) for arr, name in zip(arrays, buffers)]


def assert_class(lay, tensors):
    """For rows of whole 64-byte chunks: the tensors' bases and strides give the class's max_nv."""
    got = align_nv([t.data_ptr() for t in tensors] + [t.stride(0) for t in tensors])
    assert got == lay.max_nv, (lay, got, [(t.data_ptr() % 16, t.stride(0) % 16) for t in tensors])


def check_kernels(ran, max_nv, want, forbid=(), padded_copies=False):
    """ran: per call the kernel names it launched (rs_last_kernels). Below 16-byte alignment
    (max_nv < 4) no call launched a hipRTC kernel and no table kernel wider than the layout
    allows (`_nv<d>` suffix <= max_nv); every call launched a kernel of each wanted prefix (a
    tuple: any of them) and none of a forbidden one. padded_copies: shard tails, whose kernels
    run on the library's own aligned copies and may be of any kind and width."""
    assert ran, "no call was made"
    for kernels in ran:
        assert kernels, "the call launched nothing"
        if max_nv < 4 and not padded_copies:
            jit = [x for x in kernels if x.startswith(HIPRTC)]
            assert not jit, f"hipRTC kernels {jit} on a layout with max_nv {max_nv}: {ran}"
            wide = [x for x in kernels for d in re.findall(r"_nv(\d+)$", x) if int(d) > max_nv]
            assert not wide, f"kernels {wide} wider than max_nv {max_nv}: {ran}"
        for w in want:
            alts = w if isinstance(w, tuple) else (w,)
            assert any(x.startswith(alts) for x in kernels), f"no kernel {w} among {ran}"
        for f in forbid:
            assert not any(x.startswith(f) for x in kernels), f"forbidden kernel {f} among {ran}"


class EncodeContractError(AssertionError):
    """checks: every one of the four checks that failed (1 parity rows == expected, 2 the input
    unchanged, 3 no parity byte outside the rows' [0, m * sb) written, 4 the guard stripe
    intact); check: the first of them."""

    def __init__(self, failed):
        self.failed = failed
        self.checks = {c for c, _ in failed}
        self.check = failed[0][0]
        super().__init__("; ".join(f"check {c}: {msg}" for c, msg in failed))


def check_encode(run, k, m, data, expected, pads=(256, 64), seed=303):
    """data: [n, k, sb]; expected: the parity [n, m, sb]. pads: bytes of stride padding of the
    input and the parity buffer. The input's padding holds random nonzero bytes, the parity
    buffer GUARD everywhere, with one guard stripe past the batch. Raises EncodeContractError
    naming every failed check; returns the parity buffer."""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    n, kk, sb = data.shape
    assert kk == k
    expected = np.asarray(expected, np.uint8).reshape(n, m * sb)
    rng = np.random.default_rng(seed)
    orig = _strided(data, pads[0], rng)
    par_init = np.full((n + 1, m * sb + pads[1]), GUARD, np.uint8)
    orig_after, par = run(orig.copy(), par_init.copy())
    orig_after, par = np.asarray(orig_after, np.uint8), np.asarray(par, np.uint8)
    assert orig_after.shape == orig.shape and par.shape == par_init.shape
    failed = []
    bad = par[:n, :m * sb] != expected
    if bad.any():
        s, i = (int(x) for x in np.argwhere(bad)[0])
        failed.append((1, f"parity differs from the expected bytes: {int(bad.sum())} bytes, first in stripe {s} "
                          f"row {i // sb} byte {i % sb} (shard {sb})"))
    if not (orig_after == orig).all():
        failed.append((2, f"the input buffer was written ({_where(orig_after != orig)})"))
    bad = par[:n, m * sb:] != GUARD
    if bad.any():
        failed.append((3, f"parity stride padding was written ({_where(bad)}, counted from byte {m * sb} of the "
                          f"row; row length {par.shape[1]})"))
    bad = par[n] != GUARD
    if bad.any():
        failed.append((4, f"the guard stripe past the batch was written ({_where(bad)})"))
    if failed:
        raise EncodeContractError(failed)
    return par
