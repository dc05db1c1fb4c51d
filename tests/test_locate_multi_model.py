"""The multi-shard locate's numpy model (tests/locate_multi_model.py) against the
construction (the corrupt sets are known), against the library's host selftest of the same
algorithm, and against the single-shard model (tests/locate_model.py) wherever that one answers."""
import functools

import numpy as np
import pytest

from locate_model import CLEAN, RECOVERY_SET, encode, symbols
from locate_multi_model import UNLOCATED, MultiCode, corrupt, mul16, xor_symbol
from rs_amd import reedsol_amd as R

CODES = [(10, 4), (5, 2), (3, 10), (16, 16)]
SETS = 12  # random shard sets per size


def radius(m):
    return min(m // 2, R.LOCATE_MAX_T)


@functools.lru_cache(maxsize=None)
def model(k, m):
    return MultiCode(k, m)


@pytest.fixture(params=CODES, ids=lambda c: f"rs{c[0]}_{c[1]}")
def code(request):
    return model(*request.param)


@pytest.fixture(params=[c for c in CODES if c[1] >= 4], ids=lambda c: f"rs{c[0]}_{c[1]}")
def code4(request):
    """the codes whose radius m / 2 holds two corrupt shards"""
    return model(*request.param)


def test_selftest(code):
    assert R.locate_multi_selftest(code.k, code.m, radius(code.m), trials=4, seed=7) == 0


def test_any_m_columns_are_independent(code):
    """the MDS property the soundness rests on, sampled: a span of max_t columns holds no other"""
    rng = np.random.default_rng(code.k * 100 + code.m)
    t = radius(code.m)
    for _ in range(SETS):
        T = sorted(rng.choice(code.k + code.m, t, replace=False).tolist())
        B, piv = code.span(code.G[:, T], t)
        assert len(piv) == t and code.members(B, piv) == T


def test_every_set_within_the_radius_is_located(code):
    rng = np.random.default_rng(code.k * 1000 + code.m)
    max_t = radius(code.m)
    for t in range(max_t + 1):
        for _ in range(SETS):
            T = sorted(rng.choice(code.k + code.m, t, replace=False).tolist())
            data, stored = corrupt(code, rng, T)
            assert code.locate_multi(data, stored, max_t) == (t, T), (t, T)


def test_nothing_is_reported_beyond_the_radius(code):
    """t > max_t shards with independent errors: rank t > max_t"""
    rng = np.random.default_rng(code.k * 1000 + code.m + 1)
    max_t = radius(code.m)
    for t in range(max_t + 1, code.m + 1):
        for _ in range(SETS):
            T = rng.choice(code.k + code.m, t, replace=False).tolist()
            data, stored = corrupt(code, rng, T)
            assert code.locate_multi(data, stored, max_t) == (UNLOCATED, []), (t, T)


def test_smaller_max_t_gives_unlocated_not_a_subset(code4):
    code = code4
    rng = np.random.default_rng(3)
    data, stored = corrupt(code, rng, [0, code.k + 1])
    assert code.locate_multi(data, stored, 1) == (UNLOCATED, [])
    assert code.locate_multi(data, stored, 2) == (2, [0, code.k + 1])


def test_rank_deficient_pair_is_unlocated(code4):
    """err_b = alpha * err_a at every symbol: rank 1, and no single column explains it"""
    code = code4
    rng = np.random.default_rng(11)
    P = code.data.shape[1] // 2
    for a, b in [(0, code.k - 1), (1, code.k), (code.k, code.k + code.m - 1)]:
        data, stored = code.data.copy(), code.par.copy()
        alpha = int(rng.integers(2, 65536))
        for q in rng.choice(P, 5, replace=False):
            e = int(rng.integers(1, 65536))
            xor_symbol(data[a] if a < code.k else stored[a - code.k], int(q), e)
            xor_symbol(data[b] if b < code.k else stored[b - code.k], int(q), mul16(e, alpha))
        assert code.locate_multi(data, stored, radius(code.m)) == (UNLOCATED, [])


def test_fewer_corrupt_positions_than_shards_is_unlocated(code4):
    """two shards wrong at one and the same symbol only: rank 1"""
    code = code4
    data, stored = code.data.copy(), code.par.copy()
    xor_symbol(data[0], 9, 0x1234)
    xor_symbol(data[code.k - 1], 9, 0x0101)
    assert code.locate_multi(data, stored, radius(code.m)) == (UNLOCATED, [])


def test_agrees_with_the_single_shard_model(code):
    """<= 1 corrupt shard: the same index. Bad recovery shards only: locate's RECOVERY_SET flags
    are the rows the multi form names."""
    rng = np.random.default_rng(code.k + code.m)
    max_t = radius(code.m)
    assert code.locate_multi(code.data, code.par, max_t) == (0, [])
    assert code.locate(code.data, code.par) == CLEAN
    for sh in [0, code.k - 1, code.k, code.k + code.m - 1] + rng.choice(code.k + code.m, 6).tolist():
        data, stored = corrupt(code, rng, [sh])
        assert code.locate_multi(data, stored, max_t) == (1, [sh])
        assert code.locate(data, stored) == sh
    for t in range(2, min(max_t, code.m - 1) + 1):
        rows = sorted(rng.choice(code.m, t, replace=False).tolist())
        data, stored = corrupt(code, rng, [code.k + r for r in rows])
        Sb = encode(code.k, code.m, data) ^ stored
        assert code.locate_syndromes(Sb) == RECOVERY_SET
        assert np.flatnonzero((symbols(Sb) != 0).any(axis=1)).tolist() == rows
        assert code.locate_multi_syndromes(Sb, max_t) == (t, [code.k + r for r in rows])
