"""Rebuild, host side: the argument checks of rs_rebuild_batch_dev (all of which come back before
any device call, in the header's order), the path names, the host selftest of the plan kernel's
algebra and the compile check of the rebuild variant of the syndrome network."""
import ctypes as C

import pytest

from rs_amd import reedsol_amd as R


def test_validation_precedes_device():
    L = R.lib()
    buf = (C.c_uint8 * 64)()
    base = C.addressof(buf) // 16 * 16 + 16  # never dereferenced: every call below fails or returns first
    far, farther = 1 << 40, 1 << 41  # recovery and rebuilt lie here unless a case says otherwise: no overlap
    p = C.c_void_p(base)

    def call(k=10, m=4, sb=4096, n=1, present=p, pstride=0, max_e=2, orig=p, ostride=0, rec=C.c_void_p(far), rstride=0,
             out=C.c_void_p(farther), outstride=0, flags=0):
        return L.rs_rebuild_batch_dev(k, m, sb, n, present, pstride, max_e, orig, ostride, rec, rstride, out, outstride,
                                      None, flags, None)

    assert call(k=0) == 1  # TooFewOriginalShards
    assert call(k=0, n=0, flags=3) == 1  # ... before anything else
    assert call(sb=4095) == 3  # InvalidShardSize (check_codec, as the encode)
    assert call(k=40000, m=40000) == 4  # UnsupportedShardCount
    assert call(n=0) == 0  # nothing to do, nothing written
    assert call(n=0, present=None, orig=None, rec=None, out=None, flags=3) == 0  # ... whatever the other arguments
    assert call(max_e=0) == 0
    assert call(max_e=0, present=None, orig=None, rec=None, out=None, ostride=1, flags=3) == 0
    assert call(present=None) == 14  # InvalidArgument: a NULL pointer
    assert call(orig=None) == 14
    assert call(rec=None) == 14
    assert call(out=None) == 14
    assert call(max_e=5) == 14  # max_e > m
    assert b"max_e" in L.rs_last_error()
    assert call(max_e=5, out=None) == 14 and b"NULL" in L.rs_last_error()  # the NULL comes first
    assert call(pstride=13) == 14  # a stride below its row size
    assert call(ostride=10 * 4096 - 16) == 14
    assert call(rstride=4 * 4096 - 16) == 14
    assert call(outstride=2 * 4096 - 16) == 14
    assert call(outstride=2 * 4096 - 16, flags=1) == 14 and b"stride" in L.rs_last_error()  # ... before the flags
    for flags in (1, 2, 3):  # D1: no field multiplication; D2: originals left out of the parity
        assert call(flags=flags) == 14
        assert call(flags=flags, orig=C.c_void_p(base + 2)) == 14 and b"flags" in L.rs_last_error()
    # whole chunks: every data buffer and stride a multiple of 4
    assert call(orig=C.c_void_p(base + 2)) == 14
    assert call(rec=C.c_void_p(far + 2)) == 14
    assert call(out=C.c_void_p(farther + 2)) == 14
    assert call(ostride=10 * 4096 + 2) == 14
    assert call(rstride=4 * 4096 + 2) == 14
    assert call(outstride=2 * 4096 + 2) == 14
    assert call(out=C.c_void_p(base + 2)) == 14 and b"aligned" in L.rs_last_error()  # ... before the overlap
    # the rebuilt range [out, out + n * stride) may hold neither input
    assert call(out=p) == 14 and b"overlap" in L.rs_last_error()  # the same address as the originals
    assert call(out=C.c_void_p(far)) == 14 and b"overlap" in L.rs_last_error()  # ... as the recovery shards
    assert call(n=3, out=C.c_void_p(base - 3 * 2 * 4096 + 4)) == 14  # its last bytes reach into the originals
    assert call(n=3, out=C.c_void_p(base + 3 * 10 * 4096 - 4)) == 14  # it starts in their last bytes
    assert call(n=3, out=C.c_void_p(far + 3 * 4 * 4096 - 4)) == 14  # ... in the recovery shards' last bytes
    assert call(sb=130, out=C.c_void_p(base + 1)) == 14  # tails: any alignment, the overlap still counts
    assert R.last_kernels() == []  # nothing launched


@pytest.mark.parametrize("k,m", [(10, 4), (33, 5), (4, 4), (200, 55), (3, 9)])
def test_selftest(k, m):
    assert R.rebuild_selftest(k, m, trials=16, seed=k * 1000 + m) == 0


def test_selftest_rejects_k0():
    with pytest.raises(R.InvalidArgument):
        R.rebuild_selftest(0, 4)


@pytest.mark.parametrize("k,m", [(10, 4), (33, 5)])
def test_compile_check(k, m):
    r = R.rebuild_compile_check(k, m)
    assert r["code_bytes"] > 0


@pytest.mark.parametrize("k,m", [(200, 55), (3, 9), (10, 9)])
def test_compile_check_rejects(k, m):
    """wide codes (m > 8) and low-rate codes have no syndrome network"""
    with pytest.raises(R.InvalidArgument):
        R.rebuild_compile_check(k, m)


def test_path_names(monkeypatch):
    assert R.rebuild_kernel_name(10, 4, 4096, 2) == "psyn_rebuild_k10_m4"
    assert R.rebuild_kernel_name(33, 5, 1 << 20, 5) == "psyn_rebuild_k33_m5"
    # a tail, a wide code and a low-rate code: the general form around the paths of its two calls
    # ... and low-rate codes within the network's shape limits (m <= 8): their parity is the low-rate
    # construction's, so the dispatch keeps them off the fast form as this name says
    for k, m, sb, max_e in [(10, 4, 100, 2), (10, 4, 4096 + 64, 4), (200, 55, 2048, 20), (3, 9, 4096, 3),
                            (3, 5, 4096, 5), (2, 4, 4096, 2), (4, 8, 8192, 8), (1, 2, 4096, 1)]:
        want = (R.patterns_kernel_name(k, m, sb, max_e) + "+rebuild_gather+" + R.encode_kernel_name(k, m, sb) +
                "+rebuild_pick")
        assert R.rebuild_kernel_name(k, m, sb, max_e) == want
        assert "psyn_rebuild" not in want
    monkeypatch.setenv("RS_AMD_JIT", "0")
    name = R.rebuild_kernel_name(10, 4, 4096, 2)
    assert name == (R.patterns_kernel_name(10, 4, 4096, 2) + "+rebuild_gather+" + R.encode_kernel_name(10, 4, 4096) +
                    "+rebuild_pick")
    assert "psyn" not in name
