"""The multi-shard locate restated in numpy on the oracle's encode, on
locate_model.Code's coefficients and symbol layout. G = [C | I_m]: column j < k is the encode's
coefficients c[r][j], column k + r the unit vector e_r. With corrupt shards T the syndrome vector
of symbol p is S(p) = sum_{i in T} G_i * err_i(p); every symbol shares T, so the S(p) span a
subspace V of dimension rho <= |T| and the columns of G in V are the corrupt shards.

The rank is found as the library finds it: a basis of V in reduced echelon form (B_j[piv_l] =
delta_jl) grows by one vector per round, taken at the smallest symbol index p whose S(p) is not
sum_j B_j * S_{piv_j}(p); a round that finds none has confirmed the rank."""
import numpy as np

import oracle as O
from locate_model import Code, encode, symbol_bytes, symbols
from rs_amd import reedsol_amd as R

UNLOCATED = R.LOCATE_UNLOCATED


class MultiCode(Code):
    def __init__(self, k, m):
        super().__init__(k, m)
        self.G = np.concatenate([self.c, np.eye(m, dtype=np.uint16)], axis=1)  # [m, k + m]

    def mul(self, a, b):
        """elementwise product of two arrays of symbols"""
        a, b = np.broadcast_arrays(np.asarray(a, np.uint16), np.asarray(b, np.uint16))
        prod = self.exp[(self.log[a] + self.log[b]) % 65535]
        return np.where((a != 0) & (b != 0), prod, 0).astype(np.uint16)

    def inv(self, a):
        return int(self.exp[(65535 - self.log[a]) % 65535])

    def check_symbols(self, sb):
        """the symbols the check reads (a mask over symbols()'s order): all of them"""
        return np.ones(sb // 2, bool)

    def check_rows(self):
        """the rows the check compares with the span: all of them"""
        return range(self.m)

    def span(self, S, max_t):
        """(basis [rho, m], pivot rows) of the span of the columns of S [m, P], or None when
        its rank exceeds max_t"""
        B = np.zeros((0, self.m), np.uint16)
        piv = []
        read, rows = self.check_symbols(2 * S.shape[1]), list(self.check_rows())
        for rnd in range(max_t + 1):
            res = S.copy()  # S(p) reduced by the basis, every p at once
            for j, row in enumerate(piv):
                res ^= self.mul(B[j][:, None], S[row][None, :])
            failing = np.flatnonzero((res[rows] != 0).any(axis=0) & read)
            if failing.size == 0:
                return B, piv
            if rnd == max_t:
                return None
            v = res[:, failing[0]]
            rho = int(np.flatnonzero(v)[0])
            v = self.mul(v, self.inv(v[rho]))
            assert v[rho] == 1
            B = B ^ self.mul(B[:, rho][:, None], v[None, :])
            B = np.concatenate([B, v[None, :]])
            piv.append(rho)
        raise AssertionError("not reached")

    def members(self, B, piv):
        """the columns of G in the span of the reduced basis B, ascending"""
        coef = self.G[piv, :]  # [rho, k + m]: a column's coordinates are its entries at the pivots
        comb = np.zeros_like(self.G)
        for l in range(len(piv)):
            comb ^= self.mul(B[l][:, None], coef[l][None, :])
        return np.flatnonzero((comb == self.G).all(axis=0)).tolist()

    def locate_multi_syndromes(self, Sb, max_t):
        """Sb [m, sb] = encode(originals) ^ stored, as bytes -> (count, located shards)"""
        found = self.span(symbols(Sb), max_t)
        if found is None:
            return UNLOCATED, []
        B, piv = found
        T = self.members(B, piv)
        assert len(T) <= len(piv)  # any m columns of G are independent
        if len(T) != len(piv):
            return UNLOCATED, []
        return len(T), T

    def locate_multi(self, data, stored, max_t):
        return self.locate_multi_syndromes(encode(self.k, self.m, data) ^ stored, max_t)


def xor_symbol(shard, q, err):
    """shard (bytes of one shard, modified in place): symbol q ^= err"""
    lo, hi = symbol_bytes(shard.shape[0], q)
    shard[lo] ^= err & 0xFF
    shard[hi] ^= err >> 8


def corrupt(code, rng, shards, full_rank=True):
    """(data, stored) of code.data / code.par with the shards `shards` (indices in [0, k + m))
    corrupt. full_rank: shard i alone is wrong at a symbol of its own, so the errors are
    independent rows; the symbols that belong to no shard are wrong at random."""
    data, stored = code.data.copy(), code.par.copy()
    P = data.shape[1] // 2
    own = rng.permutation(P)[:len(shards)] if full_rank else []
    free = np.setdiff1d(np.arange(P), own)
    for i, sh in enumerate(shards):
        row = data[sh] if sh < code.k else stored[sh - code.k]
        if full_rank:
            xor_symbol(row, int(own[i]), int(rng.integers(1, 65536)))
        for q in free[rng.random(free.size) < 0.5]:
            xor_symbol(row, int(q), int(rng.integers(1, 65536)))
    return data, stored


def mul16(a, b):
    """the product of two symbols by the oracle's multiply"""
    return O.mul16(int(a), int(O.table("log")[b])) if b else 0
