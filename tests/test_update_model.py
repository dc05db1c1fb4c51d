"""The update identity restated on the oracle: the corrected encode is linear
over GF(2^16), parity[r] = sum_j c[r][j] * original[j], so with delta = old ^ new
    encode(old) ^ encode(a stripe holding only the deltas) == encode(new),
and every whole chunk of the parity delta of one changed original j is mul_chunk(delta chunk,
log c[r][j]); the tail chunk (sb % 64 bytes: low bytes first, high bytes after) is the same
multiply symbol by symbol. This is the algebra tests/test_gpu_update.py expects of the GPU."""
import numpy as np
import pytest

import oracle as O
from helpers import splitmix_bytes

CODES = [(10, 4), (5, 2), (16, 16), (200, 55), (3, 1)]
SIZES = [64, 130, 4096 + 34]


def coefficient_logs(k, m):
    """log c[r][j], [m, k]: the encode of unit vectors (symbol 1, one chunk)"""
    log = O.table("log").astype(np.int64)
    assert O.table("exp")[0] == 1  # symbol 1 is the field's one
    cl = np.zeros((m, k), np.int64)
    for j in range(k):
        unit = np.zeros((1, k, 64), np.uint8)
        unit[0, j, :32] = 1
        par = O.encode_batch(k, m, unit)[0]
        sym = par[:, :32].astype(np.uint16) | par[:, 32:].astype(np.uint16) << 8
        assert (sym == sym[:, :1]).all() and (sym != 0).all()
        cl[:, j] = log[sym[:, 0]]
    return cl


@pytest.fixture(scope="module", params=CODES, ids=lambda c: f"rs{c[0]}_{c[1]}")
def code(request):
    k, m = request.param
    return k, m, coefficient_logs(k, m)


@pytest.mark.parametrize("sb", SIZES)
def test_parity_delta_is_the_encode_of_the_deltas(code, sb):
    k, m, _ = code
    n = 2
    old = splitmix_bytes(k * 31 + m + sb, n * k * sb).reshape(n, k, sb)
    new = old.copy()
    changed = sorted({0, k // 2, k - 1})
    for s in range(n):
        for j in changed[:1 + s]:  # one original in stripe 0, two in stripe 1 (where k allows)
            new[s, j] = splitmix_bytes(1000 * s + j + sb, sb)
    only = old ^ new  # zero everywhere but the changed shards
    assert (O.encode_batch(k, m, old) ^ O.encode_batch(k, m, only) == O.encode_batch(k, m, new)).all()


@pytest.mark.parametrize("sb", SIZES)
def test_parity_delta_is_the_coefficient_multiply(code, sb):
    k, m, cl = code
    whole, t = sb - sb % 64, sb % 64
    h = t // 2
    for j in sorted({0, k - 1}):
        only = np.zeros((1, k, sb), np.uint8)
        delta = splitmix_bytes(77 + j + sb, sb)
        only[0, j] = delta
        pd = O.encode_batch(k, m, only)[0]  # = encode(old) ^ encode(new) for any old with old ^ new == only
        for r in sorted({0, m - 1}):
            lm = int(cl[r, j])
            for c in range(0, whole, 64):
                assert (pd[r, c:c + 64] == O.mul_chunk(delta[c:c + 64], lm)).all(), (j, r, c)
            for i in range(h):  # the tail: symbol i = low byte at whole + i, high byte at whole + h + i
                x = int(delta[whole + i]) | int(delta[whole + h + i]) << 8
                y = int(pd[r, whole + i]) | int(pd[r, whole + h + i]) << 8
                assert O.mul16(x, lm) == y, (j, r, i)
