"""tests/scrub_sweep.py on the CPU: the generator's coverage conditions hold for every shard size
the GPU file uses, the reference back ends (verify, locate and the multi-shard locate at max_t = 1)
pass every sweep, and eleven back ends that each skip a region (what a kernel with a wrong loop
bound, lane mask or row count would do) are caught, with every failing probe inside the region
skipped. Small shards and a 256-byte segment keep the file at a few seconds; the geometry
(segments, 4 passes, 16-byte slots, chunk halves, tail) is the kernels'."""
import numpy as np
import pytest

import oracle as O
import scrub_sweep as W
from locate_model import UNLOCATED, Code
from locate_multi_model import MultiCode

SEG = 256
K, M = 3, 2
# 866 = three whole segments, then 64 + 34: a partial last segment with a 17-symbol tail;
# 832: the same without the tail; 2, 66, 130: tail-only, one and two chunks
SIZES = [866, 832, 2, 66, 130]
GPU_SIZES = [20480, 20514, 2, 66, 130]  # tests/test_gpu_scrub_sweep.py, at the kernels' 16 KiB segment


@pytest.fixture(scope="module", params=SIZES, ids=lambda sb: f"sb{sb}")
def batch(request):
    sb = request.param
    return W.Batch(K, M, sb, W.positions(sb, SEG), seg=SEG)


@pytest.fixture(scope="module")
def big():
    """sb = 866: every region a mutant below skips exists in it"""
    return W.Batch(K, M, 866, W.positions(866, SEG), seg=SEG)


# ------------------------------------------------------------------------ generator
@pytest.mark.parametrize("sb", GPU_SIZES + [640, 674, 64, 4096])  # 640, 674: the highbyte sweep of RS(200, 55)
def test_positions_cover_the_gpu_sizes(sb):
    probes = W.positions(sb)  # asserts its own coverage conditions
    offs = {o for o, _ in probes}
    assert {o // 16 for o in offs} == set(range(-(-sb // 16)))
    for base in range(0, sb, W.SEG):
        assert base in offs and min(base + W.SEG, sb) - 1 in offs
    if sb <= 130:
        assert offs == set(range(sb))  # every byte a probe
    print(f"sb {sb}: {len(probes)} probes")


def test_probe_counts():
    # a slot each, the rest of the first and the last chunk, bytes 16383 and 16384
    assert len(W.positions(20480)) == 1280 + 60 + 60 + 2
    assert len(W.positions(20514)) == 1283 + 60 + 60 + 31 + 2  # and the rest of the 34-byte tail
    assert len(W.positions(2)) == 16  # two bytes x eight bits


def test_coverage_conditions_reject_a_thinned_probe_set():
    probes = W.positions(866, SEG)
    for drop in (lambda o, b: o // 16 == 20,  # a slot
                 lambda o, b: o % 16 == 15 and b == 7,  # a pair
                 lambda o, b: o == 840,  # a tail byte
                 lambda o, b: o == 511):  # a segment's last byte
        with pytest.raises(AssertionError):
            W._assert_coverage([p for p in probes if not drop(*p)], 866, SEG)


# -------------------------------------------------------------- the reference passes
def test_reference_passes_every_sweep(batch):
    for build in (W.recovery_sweep, W.original_sweep):
        sweep = build(batch)
        W.check_verify(sweep, W.verify_reference)
        W.check_locate(sweep, W.locate_reference())
    for sweep in (W.reject_sweep(batch), W.highbyte_sweep(batch, originals=range(K))):
        assert sweep.nprobes == len(batch.probes)
        W.check_locate(sweep, W.locate_reference())


def test_multi_reference_passes_every_sweep(batch):
    """the multi-shard model at max_t = 1 gives locate's answers on every sweep (a reject stripe
    has rank 2 > max_t), and its own guard excludes no stripe"""
    for build in (W.recovery_sweep, W.original_sweep, W.reject_sweep):
        sweep = build(batch)
        W.check_locate(sweep, W.locate_multi_reference(), reference=MultiCode)
    sweep = W.highbyte_sweep(batch, originals=range(K))
    assert sweep.nprobes == len(batch.probes)
    W.check_locate(sweep, W.locate_multi_reference(), reference=MultiCode)


def test_multi_adapter():
    """multi_as_locate: count 0 -> CLEAN, 1 -> located[0], unlocated -> UNLOCATED, the present
    rows as returned, counts[3] -> [clean, one, 0, unlocated]"""
    present = np.ones((3, K + M), np.uint8)
    present[1, 4] = 0

    def backend(k, m, data, stored):
        return np.array([0, 1, UNLOCATED], np.int32), np.array([[-1], [4], [-1]], np.int32), present, [1, 1, 1], True

    located, pres, counts, unchanged = W.multi_as_locate(backend)(K, M, None, None)
    assert located.tolist() == [W.CLEAN, 4, UNLOCATED] and pres is present and counts == [1, 1, 0, 1] and unchanged


def test_sweep_expectations(big):
    sweep = W.recovery_sweep(big)
    assert sweep.flags.sum() == sweep.nprobes and sweep.counts == [3, sweep.nprobes, 0, 0]
    assert all((p is None) == (sweep.flags[s].sum() == 0) for s, p in enumerate(sweep.stripes))
    sweep = W.original_sweep(big)
    assert sweep.flags.sum() == sweep.nprobes * M
    assert {p.shard for p in sweep.stripes if p} == set(range(K))
    sweep = W.reject_sweep(big)
    assert sweep.counts == [3, 0, 0, sweep.nprobes] and sweep.present.all()
    assert all((p is None) != (sweep.located[s] == UNLOCATED) for s, p in enumerate(sweep.stripes))
    assert {p.anchor for p in sweep.stripes if p} == {0, 865}
    assert all(W.symbol_of(866, p.anchor) != W.symbol_of(866, p.offset) for p in sweep.stripes if p)


# ----------------------------------------------------------------- checker behaviour
def test_checker_sees_a_leak_a_count_and_a_write(big):
    sweep = W.recovery_sweep(big)

    def leak(k, m, data, stored):
        flags, count, _ = W.verify_reference(k, m, data, stored)
        flags[1, 0] = 1  # the clean stripe next to stripe 0
        return flags, count + 1, True

    with pytest.raises(W.ScrubSweepError) as e:
        W.check_verify(sweep, leak)
    assert e.value.stripe == 1 and e.value.offset is None and "clean stripe" in str(e.value)
    with pytest.raises(AssertionError):
        W.check_verify(sweep, lambda *a: W.verify_reference(*a)[:1] + (0, True))
    with pytest.raises(AssertionError, match="wrote an input"):
        W.check_verify(sweep, lambda *a: W.verify_reference(*a)[:2] + (False,))

    def wrong_counts(k, m, data, stored):
        located, present, counts, _ = W.locate_reference()(k, m, data, stored)
        return located, present, [counts[0] + 1] + counts[1:], True

    with pytest.raises(AssertionError):
        W.check_locate(sweep, wrong_counts)

    def wrong_present(k, m, data, stored):
        located, present, counts, _ = W.locate_reference()(k, m, data, stored)
        present[5] = 1
        return located, present, counts, True

    with pytest.raises(W.ScrubSweepError) as e:
        W.check_locate(sweep, wrong_present)
    assert e.value.stripe == 5 and "present row" in str(e.value)


def test_checker_counts_the_stripes_it_judged(big):
    sweep = W.recovery_sweep(big)
    sweep.stripes[7] = None  # a probe lost after generation
    with pytest.raises(AssertionError, match="stripes judged"):
        W.check_verify(sweep, W.verify_reference)


def test_error_names_the_position(big):
    sweep = W.recovery_sweep(big)
    s = next(s for s, p in enumerate(sweep.stripes) if p and p.offset == 511)

    def blind(k, m, data, stored):
        flags, count, _ = W.verify_reference(k, m, data, stored)
        flags[s] = 0
        return flags, count - 1, True

    with pytest.raises(W.ScrubSweepError) as e:
        W.check_verify(sweep, blind)
    p = sweep.stripes[s]
    assert (e.value.sweep, e.value.stripe, e.value.offset, e.value.bit, e.value.shard) == \
        ("recovery", s, 511, p.bit, K + s % M)
    assert f"stripe {s}, offset 511 bit {p.bit} in shard {K + s % M} (segment 1, pass 3, 16-byte slot 31, byte lane 15" \
        in str(e.value)


# -------------------------------------------------------------------- verify mutants
def masked_verify(mask):
    """a verify that sees only the bits of mask [sb] (uint8 per byte offset)"""
    def run(k, m, data, stored):
        flags = ((stored ^ O.encode_batch(k, m, data)) & mask[None, None, :]).any(axis=2)
        return flags.astype(np.uint8), int(flags.sum()), True
    return run


OFF = np.arange(866)
VERIFY_MUTANTS = {  # name -> (the mask it reads, the probes (offset, bit) it cannot see)
    "first half of a segment only": (np.where(OFF % SEG < SEG // 2, 0xFF, 0), lambda o, b: o % SEG >= SEG // 2),
    "no tail chunk": (np.where(OFF < 832, 0xFF, 0), lambda o, b: o >= 832),
    "no byte 15 of 16": (np.where(OFF % 16 != 15, 0xFF, 0), lambda o, b: o % 16 == 15),
    "no byte 3 of 4": (np.where(OFF % 4 != 3, 0xFF, 0), lambda o, b: o % 4 == 3),
    "no bit 7": (np.full(866, 0x7F), lambda o, b: b == 7),
    "no partial last segment": (np.where(OFF < 768, 0xFF, 0), lambda o, b: o >= 768),
}


@pytest.mark.parametrize("name", list(VERIFY_MUTANTS))
def test_verify_mutant_is_caught(big, name):
    mask, blind = VERIFY_MUTANTS[name]
    sweep = W.recovery_sweep(big)
    with pytest.raises(W.ScrubSweepError) as e:
        W.check_verify(sweep, masked_verify(mask.astype(np.uint8)))
    assert blind(e.value.offset, e.value.bit), str(e.value)
    # exactly the probes inside the region the mutant ignores fail, and the region holds some
    want = {s for s, p in enumerate(sweep.stripes) if p and blind(p.offset, p.bit)}
    assert want and {s for _, s, _, _ in e.value.failures} == want


# -------------------------------------------------------------------- locate mutants
class HalfSegmentConfirm(Code):
    def confirm_symbols(self, sb):
        return np.array([W.symbol_bytes(sb, q)[0] % SEG < SEG // 2 for q in range(sb // 2)])


class NoTailConfirm(Code):
    def confirm_symbols(self, sb):
        return np.arange(sb // 2) < (sb - sb % 64) // 2


class FirstGroupConfirm(Code):
    def confirm_rows(self):
        return range(1, min(self.m, 17))


class HighAsLow(Code):
    """classify's scan lands on a byte of S_0 and takes it for a symbol's low byte"""

    def candidate(self, Sb, S):
        sb = Sb.shape[1]
        lo = int(np.flatnonzero(Sb[0])[0])
        hi = lo + (32 if lo < sb - sb % 64 else sb % 64 // 2)
        at = lambda r, o: int(Sb[r, o]) if o < sb else 0  # noqa: E731
        return at(0, lo) | at(0, hi) << 8, at(1, lo) | at(1, hi) << 8


def failing(sweep, cls):
    with pytest.raises(W.ScrubSweepError) as e:
        W.check_locate(sweep, W.locate_reference(cls))
    return e.value


def test_locate_mutant_half_segment_confirm(big):
    sweep = W.reject_sweep(big)
    err = failing(sweep, HalfSegmentConfirm)
    assert err.sweep == "reject" and err.offset % SEG >= SEG // 2 and "located" in str(err)
    want = {s for s, p in enumerate(sweep.stripes) if p and p.offset % SEG >= SEG // 2}
    assert want and {s for _, s, _, _ in err.failures} == want  # a located shard where UNLOCATED is due
    W.check_locate(W.original_sweep(big), W.locate_reference(HalfSegmentConfirm))  # only the reject sweep sees it


def test_locate_mutant_no_tail_confirm(big):
    sweep = W.reject_sweep(big)
    err = failing(sweep, NoTailConfirm)
    assert err.offset >= 832
    want = {s for s, p in enumerate(sweep.stripes) if p and p.offset >= 832}
    assert len(want) >= 34 and {s for _, s, _, _ in err.failures} == want  # every tail byte is a probe


def test_locate_mutant_first_row_group_only():
    """m = 18: rows 1..16 are the confirm's first group, row 17 a group of its own"""
    k, m, sb = 33, 18, 320
    assert O.use_high_rate(k, m) == 1
    coarse = W.coarse_positions(sb, SEG)
    assert len(coarse) == 5  # 4 passes of the whole segment, one of the partial one
    rows = [r for r in range(1, m) for _ in coarse]
    batch = W.Batch(k, m, sb, coarse * (m - 1), seg=SEG)
    sweep = W.reject_sweep(batch, rows)
    assert {p.shard - k for p in sweep.stripes if p} == set(range(1, 18))
    W.check_locate(sweep, W.locate_reference())
    err = failing(sweep, FirstGroupConfirm)
    assert err.shard == k + 17
    assert {p.shard for _, _, p, _ in err.failures} == {k + 17} and len(err.failures) == len(coarse)


# --------------------------------------------------------------------- multi mutants
class NoTailCheck(MultiCode):
    def check_symbols(self, sb):
        return np.arange(sb // 2) < (sb - sb % 64) // 2


class FirstGroupCheck(MultiCode):
    def check_rows(self):
        return range(min(self.m, 16))


def failing_multi(sweep, cls):
    with pytest.raises(W.ScrubSweepError) as e:
        W.check_locate(sweep, W.locate_multi_reference(cls), reference=MultiCode)
    return e.value


def test_multi_mutant_no_tail_check(big):
    """A check that never reads the tail symbols. Recovery and original sweeps: a stripe whose
    probe lies in the tail looks clean. Reject sweep: a stripe is also wrong when its anchor lies
    in the tail (every second one), because the mutant then sees the probe's shard alone."""
    for build in (W.recovery_sweep, W.original_sweep):
        sweep = build(big)
        err = failing_multi(sweep, NoTailCheck)
        assert err.offset >= 832 and "located -1" in str(err)
        want = {s for s, p in enumerate(sweep.stripes) if p and p.offset >= 832}
        assert len(want) >= 34 and {s for _, s, _, _ in err.failures} == want  # every tail byte is a probe
    sweep = W.reject_sweep(big)
    err = failing_multi(sweep, NoTailCheck)
    want = {s for s, p in enumerate(sweep.stripes) if p and (p.offset >= 832 or p.anchor >= 832)}
    assert {s for _, s, _, _ in err.failures} == want
    assert any(p.anchor < 832 for _, _, p, _ in err.failures) and any(p.offset < 832 for _, _, p, _ in err.failures)


def test_multi_mutant_first_row_group_only():
    """m = 18: rows 0..15 are the check's first group, rows 16 and 17 its second"""
    k, m, sb = 33, 18, 320
    coarse = W.coarse_positions(sb, SEG)
    rows = [r for r in range(1, m) for _ in coarse]
    batch = W.Batch(k, m, sb, coarse * (m - 1), seg=SEG)
    sweep = W.reject_sweep(batch, rows)
    W.check_locate(sweep, W.locate_multi_reference(), reference=MultiCode)
    err = failing_multi(sweep, FirstGroupCheck)
    assert {p.shard for _, _, p, _ in err.failures} == {k + 16, k + 17} and len(err.failures) == 2 * len(coarse)
    sweep = W.recovery_sweep(batch)  # shard s % m: a flip in row 16 or 17 alone looks clean
    err = failing_multi(sweep, FirstGroupCheck)
    want = {s for s, p in enumerate(sweep.stripes) if p and p.shard >= k + 16}
    assert want and {s for _, s, _, _ in err.failures} == want


def test_locate_mutant_high_byte_as_low(big):
    """Needs a code with coefficients outside GF(2^8). In RS(3, 2) every coefficient lies in the
    subfield the low bytes span, so a multiplication never mixes the bytes of a symbol: the
    quotient of the two high bytes alone is the right ratio, and the mutant is correct there. (For
    the same reason a flipped high-half bit of such a code always leaves S_0's low byte zero: the
    original sweep of RS(3, 2) already runs classify's high-byte branch at every such probe.)
    RS(200, 55) has originals at positions past 255: the sweep rotates over those."""
    assert W.mixing_originals(W.model(K, M)) == []
    W.check_locate(W.highbyte_sweep(big, originals=range(K)), W.locate_reference(HighAsLow))
    k, m, sb = 200, 55, 226  # three chunks and a 17-symbol tail
    assert W.mixing_originals(W.model(k, m)) == list(range(192, 200))
    batch = W.Batch(k, m, sb, W.positions(sb, SEG), seg=SEG)
    sweep = W.highbyte_sweep(batch)
    W.check_locate(sweep, W.locate_reference())
    W.check_locate(sweep, W.locate_multi_reference(), reference=MultiCode)
    err = failing(sweep, HighAsLow)
    assert err.sweep == "highbyte"
    for _, s, p, _ in err.failures:  # every failing byte is a high byte: of a whole chunk or of the tail
        assert 32 <= p.offset % 64 if p.offset < 192 else p.offset >= 192 + 17, p
    assert len(err.failures) >= sweep.nprobes - 2  # a wrong ratio names the right original once in 65535
    assert (sweep.located[[s for s, p in enumerate(sweep.stripes) if p]] >= 0).all()
