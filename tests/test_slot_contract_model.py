"""The missing-slot checker (tests/slot_contract.py) on the CPU: it passes a backend that keeps
the contract (the oracle's reconstruct) and rejects, by the intended check, backends that break
it in each of the ways a kernel could: an erased slot treated as received, a missing recovery
row read, an erased original XORed into an output (which a zero-filled slot would hide), an
input slot used as scratch, a restored slot past e_s or stride padding written."""
import numpy as np
import pytest

from slot_contract import GUARD, SlotContractError, check_reconstruct, poison, stripe_rows

# (k, m, flags, sb, lost originals, lost recovery rows): every pattern loses the first recovery row
# and a row next to a used one; all but the last leave exactly k shards present
CODES = {
    "rs10_4": (10, 4, 0, 192, [1, 4], [0, 2]),
    "rs5_5": (5, 5, 0, 192, [0, 3, 4], [0, 3]),
    "rs33_17": (33, 17, 0, 192, [0, 5, 16, 17, 31, 32], [0, 1, 2, 4, 6, 7, 9, 11, 12, 14, 16]),
    "rs8_4_d2": (8, 4, 2, 192, [2, 7], [0]),  # D2 drops the last chunk: the literal decode, every present row read
}
N = 3


def case(oracle, name):
    k, m, flags, sb, lost, lost_rec = CODES[name]
    rng = np.random.default_rng(k * 100 + m)
    data = rng.integers(0, 256, (N, k, sb), dtype=np.uint8)
    par = oracle.encode_batch(k, m, data, quirks=flags)
    shards = np.concatenate([data, par], axis=1)
    present = np.ones(k + m, np.uint8)
    present[lost] = 0
    present[[k + r for r in lost_rec]] = 0
    expected = oracle.reconstruct_batch(k, m, present, shards, quirks=flags)
    if flags == 0:
        assert (expected == data[:, lost]).all()
    return k, m, flags, sb, lost, lost_rec, shards, present, expected


def oracle_backend(oracle, k, m, sb, present, flags, tamper=None):
    """run() for check_reconstruct on oracle.reconstruct_batch; tamper(orig, rec, out, e) then
    breaks the contract on the buffers about to be returned."""
    def run(orig, rec, out):
        n = orig.shape[0]
        shards = np.concatenate([stripe_rows(orig, k, sb), stripe_rows(rec, m, sb)], axis=1)
        got = oracle.reconstruct_batch(k, m, present, shards, quirks=flags)
        e = got.shape[1]
        out[:n, :e * sb] = got.reshape(n, -1)
        if tamper:
            tamper(orig, rec, out, e)
        return orig, rec, out
    return run


@pytest.mark.parametrize("name", list(CODES))
def test_oracle_keeps_the_contract(oracle, name):
    k, m, flags, sb, lost, _, shards, present, expected = case(oracle, name)
    e = len(lost)
    check_reconstruct(oracle_backend(oracle, k, m, sb, present, flags), k, m, shards, present, expected)
    check_reconstruct(oracle_backend(oracle, k, m, sb, present, flags), k, m, shards, present, expected,
                      max_e=e + 2, pads=(64, 0, 0))


def test_poison_properties():
    rng = np.random.default_rng(5)
    shards = rng.integers(0, 256, (4, 9, 128), dtype=np.uint8)
    shards[0, 1] = 0  # a true shard of zeros is poisoned like any other
    present = np.ones((4, 9), np.uint8)
    present[0, [1, 8]] = present[1, [0, 4, 5]] = present[3, 2] = 0
    miss = present == 0
    a = poison(shards, present, 1)
    b = poison(shards, present, 2, avoid=a)
    c = poison(shards, present, 1)
    assert (a == c).all()
    for p in (a, b):
        assert (p[miss] != shards[miss]).all()    # every poisoned byte differs from the truth
        assert (p[~miss] == shards[~miss]).all()  # nothing else is touched
    assert (a[miss] != b[miss]).all()             # and the two poisons from each other, in every byte
    assert (a[0, 1] != 0).all() and (b[0, 1] != 0).all()
    one = np.array([1, 0, 1, 1, 1, 1, 1, 1, 0], np.uint8)  # one row of flags for the whole batch
    d = poison(shards, one, 3)
    kept = [0, 2, 3, 4, 5, 6, 7]
    assert (d[:, [1, 8]] != shards[:, [1, 8]]).all() and (d[:, kept] == shards[:, kept]).all()


def rejected(oracle, name, tamper=None, present_used=None, max_e=None):
    k, m, flags, sb, lost, _, shards, present, expected = case(oracle, name)
    used = present if present_used is None else present_used(present.copy(), k)
    with pytest.raises(SlotContractError) as err:
        check_reconstruct(oracle_backend(oracle, k, m, sb, used, flags, tamper), k, m, shards, present, expected,
                          max_e=max_e)
    return err.value


@pytest.mark.parametrize("name", ["rs10_4", "rs33_17"])
def test_rejects_erased_slot_copied_through(oracle, name):
    """(a) an erased original's slot taken as received: its bytes come out as the restored shard."""
    k, _, _, sb, lost, *_ = case(oracle, name)

    def tamper(orig, rec, out, e):
        out[:orig.shape[0], :sb] = orig[:, lost[0] * sb:(lost[0] + 1) * sb]

    assert rejected(oracle, name, tamper).checks == {1, 2}


@pytest.mark.parametrize("name", ["rs10_4", "rs5_5", "rs8_4_d2"])
def test_rejects_missing_recovery_row_read(oracle, name):
    """(b) the decode runs with the first (missing) recovery row marked present."""
    def present_used(p, k):
        assert p[k] == 0
        p[k] = 1
        return p

    assert rejected(oracle, name, present_used=present_used).checks == {1, 2}


def test_rejects_erased_original_xored_in_and_zero_fill_would_not(oracle):
    """(c) an erased original XORed into one output. With the lost slots zero-filled, as three
    tests used to do, the same backend returns the expected bytes; the poison is never
    zero-equivalent to the truth, so the checker sees it."""
    name = "rs10_4"
    k, m, flags, sb, lost, lost_rec, shards, present, expected = case(oracle, name)

    def tamper(orig, rec, out, e):
        n = orig.shape[0]
        out[:n, sb:2 * sb] ^= orig[:, lost[0] * sb:(lost[0] + 1) * sb]

    assert rejected(oracle, name, tamper).checks == {1, 2}
    zeroed = shards.copy()
    zeroed[:, present == 0] = 0
    n = shards.shape[0]
    out = np.full((n + 1, len(lost) * sb), GUARD, np.uint8)
    run = oracle_backend(oracle, k, m, sb, present, flags, tamper)
    _, _, got = run(zeroed[:, :k].reshape(n, -1).copy(), zeroed[:, k:].reshape(n, -1).copy(), out)
    assert (got[:n].reshape(n, len(lost), sb) == expected).all()  # zero-fill: the defect is invisible
    for seed in (1, 2):
        p = poison(shards, present, seed)
        assert ((p ^ shards)[:, present == 0] != 0).all()


@pytest.mark.parametrize("where", ["original", "recovery", "padding"])
def test_rejects_input_written(oracle, where):
    """(d) one byte written into a missing input slot (an erased slot as scratch), or into the
    inputs' stride padding."""
    k, _, _, sb, lost, lost_rec, *_ = case(oracle, "rs10_4")

    def tamper(orig, rec, out, e):
        if where == "original":
            orig[1, lost[1] * sb + 7] ^= 0x10
        elif where == "recovery":
            rec[2, lost_rec[0] * sb + sb - 1] ^= 1
        else:
            orig[0, k * sb + 3] ^= 0x80

    assert rejected(oracle, "rs10_4", tamper).checks == {3}


def test_rejects_slot_past_e_written(oracle):
    """(e) slot e_s of a row with max_e > e_s slots written."""
    _, _, _, sb, lost, *_ = case(oracle, "rs5_5")

    def tamper(orig, rec, out, e):
        out[1, e * sb:(e + 1) * sb] = 0

    assert rejected(oracle, "rs5_5", tamper, max_e=len(lost) + 1).checks == {4}


@pytest.mark.parametrize("where", ["padding", "guard stripe"])
def test_rejects_output_padding_written(oracle, where):
    """(f) one byte of the output's stride padding, or of the guard stripe past the batch."""
    _, _, _, sb, lost, *_ = case(oracle, "rs10_4")

    def tamper(orig, rec, out, e):
        if where == "padding":
            out[0, e * sb + 1] = GUARD ^ 1
        else:
            out[orig.shape[0], 0] = 0

    assert rejected(oracle, "rs10_4", tamper).checks == {4}


def test_rejects_wrong_bytes_equal_under_both_poisons(oracle):
    """A wrong restored byte that does not depend on the poison: check 1 alone."""
    def tamper(orig, rec, out, e):
        out[0, 0] ^= 1

    assert rejected(oracle, "rs10_4", tamper).checks == {1}
