"""The locate algorithm restated in numpy on the oracle's encode: with the
corrected arithmetic parity[r] = sum_j c[r][j] * original[j], so the syndromes
S_r = encode(originals)[r] ^ stored[r] of one corrupt original j are S_r = c[r][j] * err, the
ratio S_1 / S_0 at one nonzero symbol names j, and S_r == (c[r][j] / c[0][j]) * S_0 everywhere
confirms it. Checked against the library's host selftest for the same codes."""
import numpy as np
import pytest

import oracle as O
from helpers import splitmix_bytes
from rs_amd import reedsol_amd as R

CODES = [(10, 4), (5, 2), (200, 55), (3, 10)]
SB = 128  # two chunks: 64 symbols per shard
CLEAN, RECOVERY_SET, UNLOCATED = R.LOCATE_CLEAN, R.LOCATE_RECOVERY_SET, R.LOCATE_UNLOCATED


def encode(k, m, data):
    st, rec = (O.encode if O.use_high_rate(k, m) == 1 else O.encode_low)(k, m, data)
    assert st == 0
    return rec


def symbols(shards):
    """[rows, sb] bytes -> [rows, sb / 2] symbols (low bytes at [0, 32), high at [32, 64) of a chunk)"""
    c = shards.reshape(shards.shape[0], -1, 64)
    return (c[:, :, :32].astype(np.uint16) | c[:, :, 32:].astype(np.uint16) << 8).reshape(shards.shape[0], -1)


class Code:
    def __init__(self, k, m):
        self.k, self.m = k, m
        self.log = O.table("log").astype(np.int64)
        assert O.table("exp")[0] == 1  # symbol 1 is the field's one
        c = np.zeros((m, k), np.uint16)
        for j in range(k):  # the coefficients: the encode of unit vectors (symbol 1, one chunk)
            unit = np.zeros((k, 64), np.uint8)
            unit[j, :32] = 1
            s = symbols(encode(k, m, unit))
            assert (s == s[:, :1]).all()
            c[:, j] = s[:, 0]
        assert (c != 0).all()
        self.c = c
        self.dl = (self.log[c] - self.log[c[0]][None, :]) % 65535  # log(c[r][j] / c[0][j])
        data = splitmix_bytes(k * 7 + m, k * SB).reshape(k, SB)
        self.data, self.par = data, encode(k, m, data)

    def locate(self, data, stored):
        k, m = self.k, self.m
        S = symbols(encode(k, m, data) ^ stored)
        flags = (S != 0).any(axis=1)
        if not flags.any():
            return CLEAN
        if m < 2:
            return UNLOCATED
        if flags.sum() == 1:
            return k + int(np.flatnonzero(flags)[0])
        if flags.sum() < m:
            return RECOVERY_SET
        p = int(np.flatnonzero(S[0])[0])
        if S[1, p] == 0:
            return UNLOCATED
        want = (self.log[S[1, p]] - self.log[S[0, p]]) % 65535
        match = np.flatnonzero(self.dl[1] == want)
        if match.size == 0:
            return UNLOCATED
        assert match.size == 1
        j = int(match[0])
        for r in range(1, m):
            for q in np.flatnonzero((S[0] != 0) | (S[r] != 0)):
                if O.mul16(int(S[0, q]), int(self.dl[r, j])) != S[r, q]:
                    return UNLOCATED
        return j


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
