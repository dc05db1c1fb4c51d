"""The locate algorithm restated in numpy on the oracle's encode, shared by
tests/test_locate_model.py (which checks it against the library's host selftest) and
tests/scrub_sweep.py (whose reference back end it is). With the corrected arithmetic
parity[r] = sum_j c[r][j] * original[j], so the syndromes S_r = encode(originals)[r] ^ stored[r] of
one corrupt original j are S_r = c[r][j] * err, the ratio S_1 / S_0 at one nonzero symbol names j,
and S_r == (c[r][j] / c[0][j]) * S_0 everywhere confirms it.

Symbols: a whole 64-byte chunk holds 32 symbols, low bytes at [0, 32), high bytes at [32, 64); the
tail chunk of t = sb % 64 bytes holds h = t / 2, low bytes at [0, h), high bytes at [h, 2h)."""
import numpy as np

import oracle as O
from helpers import splitmix_bytes
from rs_amd import reedsol_amd as R

SB = 128  # two chunks: 64 symbols per shard
CLEAN, RECOVERY_SET, UNLOCATED = R.LOCATE_CLEAN, R.LOCATE_RECOVERY_SET, R.LOCATE_UNLOCATED
ROW_GROUP = 16  # the rows one work item of k_locate_confirm walks (dev::kRows)


def encode(k, m, data):
    st, rec = (O.encode if O.use_high_rate(k, m) == 1 else O.encode_low)(k, m, data)
    assert st == 0
    return rec


def symbols(shards):
    """[rows, sb] bytes -> [rows, sb / 2] symbols: the whole chunks' in byte order of their low
    bytes, then the tail chunk's"""
    rows, sb = shards.shape
    assert sb % 2 == 0
    t = sb % 64
    whole, h = sb - t, t // 2
    c = shards[:, :whole].reshape(rows, -1, 64)
    s = (c[:, :, :32].astype(np.uint16) | c[:, :, 32:].astype(np.uint16) << 8).reshape(rows, -1)
    if t:
        tail = shards[:, whole:whole + h].astype(np.uint16) | shards[:, whole + h:].astype(np.uint16) << 8
        s = np.concatenate([s, tail], axis=1)
    return s


def symbol_of(sb, o):
    """the index (as symbols() orders them) of the symbol byte o of a shard belongs to"""
    whole = sb - sb % 64
    if o < whole:
        return o // 64 * 32 + o % 32
    return whole // 2 + (o - whole) % (sb % 64 // 2)


def symbol_bytes(sb, q):
    """(offset of the low byte, offset of the high byte) of symbol q"""
    whole = sb - sb % 64
    if q < whole // 2:
        lo = q // 32 * 64 + q % 32
        return lo, lo + 32
    lo = whole + q - whole // 2
    return lo, lo + sb % 64 // 2


class Code:
    def __init__(self, k, m):
        self.k, self.m = k, m
        self.log = O.table("log").astype(np.int64)
        self.exp = O.table("exp")
        assert self.exp[0] == 1  # symbol 1 is the field's one
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
        return self.locate_syndromes(encode(self.k, self.m, data) ^ stored)

    def candidate(self, Sb, S):
        """(S_0, S_1) at the symbol the candidate is taken from: the first where S_0 is nonzero.
        Sb: the syndromes as bytes [m, sb], S: as symbols."""
        p = int(np.flatnonzero(S[0])[0])
        return int(S[0, p]), int(S[1, p])

    def confirm_symbols(self, sb):
        """the symbols the confirm reads (a mask over symbols()'s order): all of them"""
        return np.ones(sb // 2, bool)

    def confirm_rows(self):
        """the rows r >= 1 the confirm compares with S_0: all of them"""
        return range(1, self.m)

    def locate_syndromes(self, Sb):
        """Sb [m, sb] = encode(originals) ^ stored, as bytes"""
        k, m = self.k, self.m
        S = symbols(Sb)
        flags = (S != 0).any(axis=1)
        if not flags.any():
            return CLEAN
        if m < 2:
            return UNLOCATED
        if flags.sum() == 1:
            return k + int(np.flatnonzero(flags)[0])
        if flags.sum() < m:
            return RECOVERY_SET
        s0, s1 = self.candidate(Sb, S)
        if s0 == 0 or s1 == 0:
            return UNLOCATED
        want = (self.log[s1] - self.log[s0]) % 65535
        match = np.flatnonzero(self.dl[1] == want)
        if match.size == 0:
            return UNLOCATED
        assert match.size == 1
        j = int(match[0])
        read = self.confirm_symbols(Sb.shape[1])
        for r in self.confirm_rows():
            for q in np.flatnonzero(((S[0] != 0) | (S[r] != 0)) & read):
                if O.mul16(int(S[0, q]), int(self.dl[r, j])) != S[r, q]:
                    return UNLOCATED
        return j

    def error_for(self, j, want_s0):
        """the symbol error in original j that makes S_0 == want_s0 at that symbol: want_s0 / c[0][j]"""
        assert want_s0 != 0
        err = O.mul16(int(want_s0), int((65535 - self.log[self.c[0, j]]) % 65535))
        assert O.mul16(err, int(self.log[self.c[0, j]])) == want_s0
        return err
