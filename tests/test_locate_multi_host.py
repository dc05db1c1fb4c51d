"""Multi-shard locate, host side: the constant, the path names, the argument checks of
rs_locate_multi_batch_dev (all of which come back before any device call) and the host selftest
of the algebra."""
import ctypes as C

import pytest

from rs_amd import reedsol_amd as R


def test_constant():
    assert R.LOCATE_MAX_T == 8
    with open(__import__("rs_amd").HEADER) as f:
        assert "#define RS_LOCATE_MAX_T 8" in f.read()


@pytest.mark.parametrize("k,m,sb,max_t", [(10, 4, 1 << 20, 2), (10, 4, 1024, 1), (200, 55, 4096, 8),
                                          (10, 4, 4096 + 34, 2), (3, 10, 4096, 5)])
def test_kernel_names(k, m, sb, max_t):
    assert R.locate_multi_kernel_name(k, m, sb, max_t) == \
        R.encode_kernel_name(k, m, sb) + f"+verify_compare+locate_multi_t{max_t}"


def test_validation_precedes_device():
    L = R.lib()
    buf = (C.c_uint8 * 64)()
    p = C.c_void_p(C.addressof(buf))  # never dereferenced: every call below fails or returns first

    def call(k, m, sb, n, max_t, count, located=None, located_stride=0, present=None, present_stride=0, ostride=0,
             rstride=0, flags=0, orig=p):
        return L.rs_locate_multi_batch_dev(k, m, sb, n, max_t, orig, ostride, p, rstride, count, located,
                                           located_stride, present, present_stride, None, flags, None)

    assert call(0, 4, 4096, 1, 2, p) == 1  # TooFewOriginalShards
    assert call(10, 4, 4095, 1, 2, p) == 3  # InvalidShardSize (check_codec, as the encode)
    assert call(10, 4, 4096, 0, 2, p) == 0  # nothing to do, nothing written
    assert call(10, 4, 4096, 0, 0, None) == 0  # ... whatever the other arguments
    assert call(10, 4, 4096, 1, 2, None) == 14  # InvalidArgument: NULL d_count
    assert call(10, 4, 4096, 1, 2, p, ostride=10 * 4096 - 16) == 14  # a stride below the row size
    assert call(10, 4, 4096, 1, 2, p, rstride=4 * 4096 - 16) == 14
    for flags in (1, 2, 3):  # D1: no field multiplication; D2: originals left out of the parity
        assert call(10, 4, 4096, 1, 2, p, flags=flags) == 14
    assert call(10, 4, 4096, 1, 2, p, orig=C.c_void_p(C.addressof(buf) + 2)) == 14  # d_original not 4-byte aligned
    assert call(10, 4, 4096, 1, 2, p, ostride=10 * 4096 + 2) == 14
    assert call(10, 4, 4096, 1, 0, p) == 14  # max_t == 0
    assert call(10, 4, 4096, 1, 3, p) == 14  # max_t > m / 2
    assert call(5, 2, 4096, 1, 2, p) == 14
    assert call(3, 1, 4096, 1, 1, p) == 14  # m < 2: no max_t is valid
    assert call(16, 16, 4096, 1, 9, p) == 14  # m / 2 allows it, RS_LOCATE_MAX_T does not
    assert call(200, 55, 4096, 1, 9, p) == 14
    assert call(10, 4, 4096, 1, 2, p, located=p, located_stride=1) == 14  # below max_t
    assert call(10, 4, 4096, 1, 2, p, present=p, present_stride=13) == 14  # k + m - 1
    assert call(10, 4, 4096, 1, 2, p, present=p, present_stride=1) == 14
    assert R.last_kernels() == []  # nothing launched


@pytest.mark.parametrize("k,m", [(10, 4), (5, 2), (6, 3), (16, 16), (32, 8), (200, 55), (3, 10), (300, 1000)])
def test_selftest(k, m):
    assert R.locate_multi_selftest(k, m, min(m // 2, 8), trials=8, seed=k * 1000 + m) == 0


def test_selftest_rejects_k0():
    with pytest.raises(R.InvalidArgument):
        R.locate_multi_selftest(0, 4, 2)
