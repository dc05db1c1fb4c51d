"""Verify (scrub), host side: the path names and the argument checks of rs_verify_batch_dev,
all of which come back before any device call."""
import ctypes as C

import pytest

from rs_amd import reedsol_amd as R


@pytest.mark.parametrize("k,m,sb", [(10, 4, 1 << 20), (10, 4, 1024), (200, 55, 4096), (10, 4, 4096 + 34), (3, 10, 4096)])
def test_kernel_names(k, m, sb):
    assert R.verify_kernel_name(k, m, sb) == R.encode_kernel_name(k, m, sb) + "+verify_compare"


def test_validation_precedes_device():
    L = R.lib()
    buf = (C.c_uint8 * 64)()
    p = C.c_void_p(C.addressof(buf))  # never dereferenced: every call below fails or returns first

    def call(k, m, sb, n, bad, bad_stride, ostride=0, rstride=0):
        return L.rs_verify_batch_dev(k, m, sb, n, p, ostride, p, rstride, bad, bad_stride, None, 0, None)

    assert call(0, 4, 4096, 1, p, 0) == 1  # TooFewOriginalShards
    assert call(10, 4, 4095, 1, p, 0) == 3  # InvalidShardSize (check_codec, as the encode)
    assert call(10, 4, 4096, 0, p, 0) == 0  # nothing to do, nothing written
    assert call(10, 4, 4096, 0, None, 0) == 0  # ... whatever the pointers
    assert call(10, 4, 4096, 1, None, 0) == 14  # InvalidArgument: NULL d_bad
    assert call(10, 4, 4096, 1, p, 3) == 14  # bad_stride = m - 1
    assert call(10, 4, 4096, 1, p, 0, ostride=10 * 4096 - 16) == 14  # a stride below the row size
    assert call(10, 4, 4096, 1, p, 0, rstride=4 * 4096 - 16) == 14
    assert R.last_kernels() == []  # nothing launched
