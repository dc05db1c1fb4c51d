"""Locate, host side: the path names, the argument checks of rs_locate_batch_dev (all of which
come back before any device call) and the host selftest of the algebra."""
import ctypes as C

import pytest

from rs_amd import reedsol_amd as R


def test_constants():
    assert (R.LOCATE_CLEAN, R.LOCATE_RECOVERY_SET, R.LOCATE_UNLOCATED) == (-1, -2, -3)
    with open(__import__("rs_amd").HEADER) as f:
        header = f.read()
    for name, value in [("RS_LOCATE_CLEAN", -1), ("RS_LOCATE_RECOVERY_SET", -2), ("RS_LOCATE_UNLOCATED", -3)]:
        assert f"#define {name} ({value})" in header


@pytest.mark.parametrize("k,m,sb", [(10, 4, 1 << 20), (10, 4, 1024), (200, 55, 4096), (10, 4, 4096 + 34), (3, 10, 4096)])
def test_kernel_names(k, m, sb):
    assert R.locate_kernel_name(k, m, sb) == R.encode_kernel_name(k, m, sb) + "+verify_compare+locate"


def test_validation_precedes_device():
    L = R.lib()
    buf = (C.c_uint8 * 64)()
    p = C.c_void_p(C.addressof(buf))  # never dereferenced: every call below fails or returns first

    def call(k, m, sb, n, located, present=None, present_stride=0, ostride=0, rstride=0, flags=0):
        return L.rs_locate_batch_dev(k, m, sb, n, p, ostride, p, rstride, located, present, present_stride, None,
                                     flags, None)

    assert call(0, 4, 4096, 1, p) == 1  # TooFewOriginalShards
    assert call(10, 4, 4095, 1, p) == 3  # InvalidShardSize (check_codec, as the encode)
    assert call(10, 4, 4096, 0, p) == 0  # nothing to do, nothing written
    assert call(10, 4, 4096, 0, None) == 0  # ... whatever the pointers
    assert call(10, 4, 4096, 1, None) == 14  # InvalidArgument: NULL d_located
    assert call(10, 4, 4096, 1, p, present=p, present_stride=13) == 14  # present_stride = k + m - 1
    assert call(10, 4, 4096, 1, p, present=p, present_stride=1) == 14
    assert call(10, 4, 4096, 1, p, ostride=10 * 4096 - 16) == 14  # a stride below the row size
    assert call(10, 4, 4096, 1, p, rstride=4 * 4096 - 16) == 14
    for flags in (1, 2, 3):  # D1: no field multiplication; D2: originals left out of the parity
        assert call(10, 4, 4096, 1, p, flags=flags) == 14
    assert R.last_kernels() == []  # nothing launched


@pytest.mark.parametrize("k,m", [(10, 4), (5, 2), (6, 3), (16, 16), (32, 8), (200, 55), (3, 10), (300, 1000)])
def test_selftest(k, m):
    assert R.locate_selftest(k, m, trials=8, seed=k * 1000 + m) == 0


def test_selftest_rejects_k0():
    with pytest.raises(R.InvalidArgument):
        R.locate_selftest(0, 4)
