"""The locate algorithm restated in numpy on the oracle's encode: with the
corrected arithmetic parity[r] = sum_j c[r][j] * original[j], so the syndromes
S_r = encode(originals)[r] ^ stored[r] of one corrupt original j are S_r = c[r][j] * err, the
ratio S_1 / S_0 at one nonzero symbol names j, and S_r == (c[r][j] / c[0][j]) * S_0 everywhere
confirms it. The model itself lives in tests/locate_model.py (tests/scrub_sweep.py shares it);
here it is checked against the library's host selftest for the same codes."""
import pytest

from locate_model import CLEAN, UNLOCATED, Code
from rs_amd import reedsol_amd as R

CODES = [(10, 4), (5, 2), (200, 55), (3, 10)]


@pytest.fixture(scope="module", params=CODES, ids=lambda c: f"rs{c[0]}_{c[1]}")
def code(request):
    return Code(*request.param)


def test_ratios_distinct(code):
    assert len(set(code.dl[1].tolist())) == code.k
    assert R.locate_selftest(code.k, code.m, trials=4, seed=5) == 0


def test_clean(code):
    assert code.locate(code.data, code.par) == CLEAN


def test_corrupt_original_is_named(code):
    for j in (0, code.k // 2, code.k - 1):
        broken = code.data.copy()
        broken[j, 5] ^= 0x21  # low byte of symbol 5
        broken[j, 64 + 32 + 9] ^= 0x80  # high byte of symbol 32 + 9
        assert code.locate(broken, code.par) == j


def test_corrupt_recovery_is_named(code):
    for r in (0, code.m - 1):
        stored = code.par.copy()
        stored[r, 77] ^= 0x04
        assert code.locate(code.data, stored) == code.k + r


def test_two_corrupt_originals_are_rejected(code):
    a, b = 0, code.k - 1
    broken = code.data.copy()
    broken[a, 3] ^= 0x10
    broken[b, 70] ^= 0x02  # another symbol: the two ratios cannot both hold
    assert code.locate(broken, code.par) == UNLOCATED
    if code.m >= 3:  # the same symbol: a weight-2 error never imitates a single shard
        broken = code.data.copy()
        broken[a, 3] ^= 0x10
        broken[b, 3] ^= 0x44
        assert code.locate(broken, code.par) == UNLOCATED
