"""The missing-slot contract of every reconstruct entry point (include/reedsol.h): the slots of
missing shards lie inside the caller's rows, their contents never influence a result and they
are never written. This module checks it for any backend, array-agnostic: the CPU oracle
(tests/test_slot_contract_model.py, which also proves that the checker rejects wrong backends)
and the GPU through the C ABI (tests/test_gpu_missing_slots.py).

A backend is a callable run(orig, rec, out_init) -> (orig_after, rec_after, out_after) over
numpy uint8 arrays with one row per stripe, the row length being the stripe stride:
  orig [n, k * sb + pad], rec [n, m * sb + pad], out_init [n + 1, max_e * sb + pad]
(out_init's last row is a guard stripe past the batch). It hands them to the entry point under
test and returns all three as they are afterwards.

The checker runs the backend twice, with two poisons of the missing slots that differ from the
truth and from each other in every byte, never zero-filled: zero is the one value a GF(2)-linear
code cannot see (an erased input XORed into an output with any coefficient adds nothing)."""
import numpy as np

GUARD = 0xA5


class SlotContractError(AssertionError):
    """checks: every one of the four checks that failed (1 restored slots == expected, 2 the two
    outputs identical, 3 inputs unchanged, 4 guard bytes intact); check: the first of them."""

    def __init__(self, failed):
        self.failed = failed
        self.checks = {c for c, _ in failed}
        self.check = failed[0][0]
        super().__init__("; ".join(f"check {c}: {msg}" for c, msg in failed))


def _present2d(present_rows, n, km):
    p = np.asarray(present_rows).astype(bool).reshape(-1, km)
    assert p.shape[0] in (1, n), p.shape
    return np.broadcast_to(p, (n, km))


def poison(shards, present_rows, seed, avoid=None):
    """A copy of shards [n, k+m, sb] in which every byte of every missing slot is true ^ r, r
    in 1..255 (so no poisoned byte equals the truth, and nothing is zero-filled). present_rows:
    k+m flags, or [n, k+m] for per-stripe patterns. avoid: an earlier poison of the same shards;
    r is then drawn from the values that also differ from that poison's in every byte."""
    shards = np.ascontiguousarray(shards, dtype=np.uint8)
    n, km, _ = shards.shape
    miss = ~_present2d(present_rows, n, km)
    rng = np.random.default_rng(seed)
    r = rng.integers(1, 256, shards.shape, dtype=np.uint8)
    if avoid is not None:
        r_avoid = (np.asarray(avoid, np.uint8) ^ shards).astype(np.int64)
        d = rng.integers(1, 255, shards.shape)  # 1..254: steps around the cycle 1..255, never back to r_avoid
        r = (1 + (r_avoid - 1 + d) % 255).astype(np.uint8)
    out = shards.copy()
    out[miss] ^= r[miss]
    return out


def _strided(rows3d, pad, rng):
    """[n, rows, sb] -> [n, rows * sb + pad], the padding filled with random nonzero bytes."""
    n = rows3d.shape[0]
    flat = rows3d.reshape(n, -1)
    buf = rng.integers(1, 256, (n, flat.shape[1] + pad), dtype=np.uint8)
    buf[:, :flat.shape[1]] = flat
    return buf


def _where(bad):
    idx = np.argwhere(bad)
    return f"{len(idx)} bytes, first at {tuple(int(x) for x in idx[0])}"


def check_reconstruct(run, k, m, shards, present, expected, max_e=None, pads=(256, 128, 64), seeds=(101, 202)):
    """shards: the true [n, k+m, sb] (originals, then recovery). present: k+m flags, or
    [n, k+m]. expected: per stripe the rows the entry point documents as written, [w_s, sb]
    (an [n, e, sb] array for one pattern per batch; w_s = 0 for a stripe that restores nothing,
    min(e_s, max_e) for one that loses more than max_e). max_e: slots of the output row
    (default: the widest expectation, at least 1). pads: bytes of stride padding of the
    original, recovery and restored buffers. Raises SlotContractError naming every failed check;
    returns the two output buffers."""
    shards = np.ascontiguousarray(shards, dtype=np.uint8)
    n, km, sb = shards.shape
    assert km == k + m
    expected = [np.asarray(x, np.uint8).reshape(-1, sb) for x in expected]
    assert len(expected) == n
    if max_e is None:
        max_e = max(1, max(x.shape[0] for x in expected))
    assert all(x.shape[0] <= max_e for x in expected)
    miss = ~_present2d(present, n, km)
    outs, failed = [], []
    first = None
    for seed in seeds:
        poisoned = poison(shards, present, seed, avoid=first)
        assert (poisoned[miss] != shards[miss]).all() and (poisoned[~miss] == shards[~miss]).all()
        if first is not None:
            assert (poisoned[miss] != first[miss]).all()
        first = poisoned if first is None else first
        rng = np.random.default_rng(seed + 7)
        orig = _strided(poisoned[:, :k], pads[0], rng)
        rec = _strided(poisoned[:, k:], pads[1], rng)
        out_init = np.full((n + 1, max_e * sb + pads[2]), GUARD, np.uint8)
        orig_after, rec_after, out = run(orig.copy(), rec.copy(), out_init.copy())
        orig_after, rec_after, out = (np.asarray(a, np.uint8) for a in (orig_after, rec_after, out))
        assert out.shape == out_init.shape and orig_after.shape == orig.shape and rec_after.shape == rec.shape
        outs.append(out)
        written = np.zeros(out.shape, bool)
        wrong = []
        for s in range(n):
            w = expected[s].size
            written[s, :w] = True
            bad = out[s, :w] != expected[s].reshape(-1)
            if bad.any():
                i = int(np.argmax(bad))
                wrong.append(f"stripe {s} restored slot {i // sb} byte {i % sb} ({int(bad.sum())} bytes of the stripe)")
        if wrong:
            failed.append((1, f"poison {seed}: restored bytes are not the expected ones: " + ", ".join(wrong[:4])))
        if not (orig_after == orig).all():
            failed.append((3, f"poison {seed}: the original buffer was written ({_where(orig_after != orig)})"))
        if not (rec_after == rec).all():
            failed.append((3, f"poison {seed}: the recovery buffer was written ({_where(rec_after != rec)})"))
        bad = ~written & (out != GUARD)
        if bad.any():
            failed.append((4, f"poison {seed}: output bytes outside the documented rows were written "
                              f"({_where(bad)}; row length {out.shape[1]}, shard {sb})"))
    if not (outs[0] == outs[1]).all():
        failed.append((2, f"the outputs under the two poisons differ ({_where(outs[0] != outs[1])})"))
    if failed:
        failed.sort(key=lambda f: f[0])
        raise SlotContractError(failed)
    return outs


def stripe_rows(buf2d, rows, sb):
    """The [n, rows, sb] shards at the start of each row of a strided buffer [n, stride] (a copy)."""
    return np.ascontiguousarray(buf2d[:, :rows * sb]).reshape(buf2d.shape[0], rows, sb)
