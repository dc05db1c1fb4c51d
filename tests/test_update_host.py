"""Update, host side: the RS_UPDATE_NONE constant, the argument checks of rs_update_batch_dev (all
of which come back before any device call, in the header's order) and the host selftest of the
algebra."""
import ctypes as C

import pytest

from rs_amd import reedsol_amd as R


def test_constant():
    assert R.UPDATE_NONE == 0xFFFFFFFF
    with open(__import__("rs_amd").HEADER) as f:
        assert "#define RS_UPDATE_NONE 0xFFFFFFFFu" in f.read()


def test_validation_precedes_device():
    L = R.lib()
    buf = (C.c_uint8 * 64)()
    base = C.addressof(buf) // 16 * 16 + 16  # never dereferenced: every call below fails or returns first
    far = 1 << 40  # where the recovery range lies unless a case says otherwise: overlaps nothing
    p = C.c_void_p(base)

    def call(k=10, m=4, sb=4096, n=1, max_u=2, index=p, istride=0, old=p, new=p, cstride=0, rec=C.c_void_p(far),
             rstride=0, flags=0):
        return L.rs_update_batch_dev(k, m, sb, n, max_u, index, istride, old, new, cstride, rec, rstride, None, flags,
                                     None)

    assert call(k=0) == 1  # TooFewOriginalShards
    assert call(k=0, n=0, flags=3) == 1  # ... before anything else
    assert call(sb=4095) == 3  # InvalidShardSize (check_codec, as the encode)
    assert call(k=40000, m=40000) == 4  # UnsupportedShardCount
    assert call(n=0) == 0  # nothing to do, nothing written
    assert call(n=0, index=None, new=None, rec=None, flags=3) == 0  # ... whatever the other arguments
    assert call(max_u=0) == 0
    assert call(max_u=0, index=None, new=None, rec=None, cstride=1, flags=3) == 0
    assert call(index=None) == 14  # InvalidArgument: a NULL pointer
    assert call(new=None) == 14
    assert call(rec=None) == 14
    assert call(max_u=11) == 14  # max_u > k
    assert call(max_u=11, index=None) == 14
    assert call(istride=1) == 14  # a stride below its row size
    assert call(cstride=2 * 4096 - 16) == 14
    assert call(rstride=4 * 4096 - 16) == 14
    for flags in (1, 2, 3):  # D1: no field multiplication; D2: originals left out of the parity
        assert call(flags=flags) == 14
    # whole chunks: every buffer and stride a multiple of 4
    assert call(old=C.c_void_p(base + 2)) == 14
    assert call(new=C.c_void_p(base + 2)) == 14
    assert call(rec=C.c_void_p(far + 2)) == 14
    assert call(cstride=2 * 4096 + 2) == 14
    assert call(rstride=4 * 4096 + 2) == 14
    # in place: the recovery range [rec, rec + n * stride) may hold neither change buffer
    assert call(rec=p) == 14  # the same address
    assert call(n=3, rec=C.c_void_p(base - 3 * 4 * 4096 + 4)) == 14  # its last bytes reach into new
    assert call(n=3, rec=C.c_void_p(base + 3 * 2 * 4096 - 4)) == 14  # it starts in new's last bytes
    assert call(old=C.c_void_p(far + 4096), new=C.c_void_p(base)) == 14  # old alone overlaps
    assert call(sb=130, rec=C.c_void_p(base + 1), old=None) == 14  # tails: any alignment, the overlap still counts
    assert R.last_kernels() == []  # nothing launched


def test_delta_form_passes_the_host_checks():
    """old == NULL is accepted by every host check: the first failure of such a call, with an
    overlapping recovery range, is the overlap (InvalidArgument), not the NULL."""
    L = R.lib()
    buf = (C.c_uint8 * 64)()
    p = C.c_void_p(C.addressof(buf) // 16 * 16 + 16)
    assert L.rs_update_batch_dev(10, 4, 4096, 1, 1, p, 0, None, p, 0, p, 0, None, 0, None) == 14
    assert b"overlap" in L.rs_last_error()
    assert R.last_kernels() == []


@pytest.mark.parametrize("k,m", [(10, 4), (5, 2), (6, 3), (16, 16), (32, 8), (200, 55), (3, 10), (300, 1000)])
def test_selftest(k, m):
    assert R.update_selftest(k, m, max_u=4, trials=8, seed=k * 1000 + m) == 0


def test_selftest_max_u_above_k():
    assert R.update_selftest(3, 1, max_u=7, trials=8, seed=3) == 0  # 1..min(max_u, k) originals change


def test_selftest_rejects_k0():
    with pytest.raises(R.InvalidArgument):
        R.update_selftest(0, 4)
