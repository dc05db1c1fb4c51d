"""Position sweeps for the detectors (rs_verify_batch_dev, rs_locate_batch_dev and
rs_locate_multi_batch_dev at max_t = 1).
A detector answers with a flag or a shard index per stripe, so a test observes only the byte
positions it corrupts: a compare that never reads some bytes passes every test that leaves those
bytes alone. This module corrupts them all, one stripe per probe. It is numpy and the oracle only
and array-agnostic like slot_contract.py and layout_contract.py: the CPU reference back ends
(tests/test_scrub_sweep_model.py, which also proves that the checker catches back ends that skip
a region) and the GPU through the Python binding (tests/test_gpu_scrub_sweep.py).

  * positions(sb): the probes (byte offset, bit) of a shard. Its coverage conditions are asserted
    on every call (_assert_coverage).
  * Batch: one stripe per probe, each with its own data and its clean oracle parity, and three
    clean stripes in between (a flag must not leak to a neighbour).
  * the sweeps, each a copy of the batch with one corruption per probed stripe:
      recovery  the probe's bit flipped in recovery shard s % m;
      original  the probe's bit flipped in original s % k;
      reject    (locate) original s % k corrupted at an anchor symbol, and the probe's bit flipped
                in a recovery row r >= 1: classify finds the anchor in row 0 and names the
                original, the confirm has to see the probe. Expected: UNLOCATED;
      highbyte  (locate, wide codes) an original gets the symbol error at the probe's symbol that
                makes the low byte of S_0 zero there, so the first nonzero byte of S_0, which
                classify takes the candidate from, is a high byte, and the original is one whose
                ratio mixes the two bytes of a symbol (mixing_originals): a classify that pairs
                the bytes of a symbol wrongly names another shard or none. A flipped bit leaves
                this to chance (a zero low byte of c[0][j] * err once in 256) or, in a code whose
                coefficients all lie in GF(2^8), cannot show it at all.
  * check_verify / check_locate: run a back end once on a sweep and compare every stripe.

A verify back end is a callable (k, m, data [n, k, sb], stored [n, m, sb]) -> (flags [n, m],
count, inputs_unchanged); a locate back end returns (located [n], present [n, k + m], counts [4],
inputs_unchanged). The multi-shard entry point at max_t = 1 is a locate back end through
multi_as_locate; check_locate is then told to consult that entry point's model (MultiCode) for
the sweeps that need one. The arrays handed over are read-only."""
import collections
import functools

import numpy as np

import oracle as O
from helpers import splitmix_bytes
from locate_model import CLEAN, RECOVERY_SET, UNLOCATED, Code, symbol_bytes, symbol_of
from locate_multi_model import MultiCode

SEG = 16384  # the scrub family's segment (dev::kSeg, kVerifySeg): the bytes of a shard one work item takes
PASSES = 4   # a segment is 4 passes of 256 lanes x 16 bytes (k_verify_compare<2>, k_locate_classify<2>)

# a probed stripe. shard: the index in [0, k + m) of the shard that holds the probe's flip (highbyte:
# the symbol error; offset is then its high byte); anchor: the reject sweep's anchor byte in original s % k
Stripe = collections.namedtuple("Stripe", "offset bit shard anchor")


class ScrubSweepError(AssertionError):
    """failures: every (sweep, stripe, Stripe or None for a clean stripe, what) that failed;
    sweep, stripe, offset, bit, shard: those of the first."""

    def __init__(self, failures, sb=None, seg=SEG):
        self.failures = failures
        self.sweep, self.stripe, probe, _ = failures[0]
        self.offset, self.bit, self.shard = (probe.offset, probe.bit, probe.shard) if probe else (None, None, None)
        lines = [f"{name} sweep, stripe {s}, {_where(p, sb, seg)}: {what}" for name, s, p, what in failures[:6]]
        more = f" (+ {len(failures) - 6} more)" if len(failures) > 6 else ""
        super().__init__(f"{len(failures)} stripes failed{more}: " + "; ".join(lines))


def _where(p, sb, seg):
    if p is None:
        return "a clean stripe"
    txt = f"offset {p.offset} bit {p.bit} in shard {p.shard}"
    if sb is not None:
        o, whole = p.offset, sb - sb % 64
        txt += (f" (segment {o // seg}, pass {o % seg // max(1, seg // PASSES)}, 16-byte slot {o // 16}, byte lane "
                f"{o % 16}, {'tail' if o >= whole else 'low half' if o % 64 < 32 else 'high half'})")
    if p.anchor is not None:
        txt += f", anchor byte {p.anchor}"
    return txt


# ------------------------------------------------------------------------- probes
def _every_byte(sb):
    """the offsets that are probes whatever else is: the first 64-byte chunk, the last whole
    chunk and the tail"""
    whole = sb - sb % 64
    out = set(range(min(64, sb))) | set(range(whole, sb))
    if whole >= 64:
        out |= set(range(whole - 64, whole))
    return out


def _segment_edges(sb, seg):
    return {e for base in range(0, sb, seg) for e in (base, min(base + seg, sb) - 1)}


def _assert_coverage(probes, sb, seg):
    offs = {o for o, _ in probes}
    assert all(0 <= o < sb and 0 <= b < 8 for o, b in probes) and len(set(probes)) == len(probes)
    slots = {o // 16 for o in offs}
    assert slots == set(range(-(-sb // 16))), "a 16-byte slot without a probe"
    pairs = {(o % 16, b) for o, b in probes}
    assert pairs == {(r, b) for r in range(min(16, sb)) for b in range(8)}, "an (offset mod 16, bit) pair without a probe"
    assert _every_byte(sb) <= offs, "a byte of the first chunk, the last whole chunk or the tail without a probe"
    assert _segment_edges(sb, seg) <= offs, "a segment's first or last byte without a probe"


def positions(sb, seg=SEG):
    """The probes of a shard of sb bytes, [(offset, bit)] in offset order: one per 16-byte slot
    (the byte lane and the bit walk with the slot index), every byte of the first chunk, the last
    whole chunk and the tail, both ends of every segment, and whatever (offset mod 16, bit) pair
    is still missing (a shard below 2 KiB has fewer than 128 slots)."""
    assert sb >= 2 and sb % 2 == 0 and seg % 64 == 0
    probes, seen, offs = [], set(), set()

    def add(o, b):
        if (o, b) not in seen:
            probes.append((o, b))
            seen.add((o, b))
            offs.add(o)

    for i in range(-(-sb // 16)):
        width, q = min(16, sb - 16 * i), i // 16
        add(16 * i + (i + q // 8) % 16 % width, q % 8)
    for o in sorted(_every_byte(sb) | _segment_edges(sb, seg)):
        if o not in offs:
            add(o, (3 * o + o // 16) % 8)
    pairs = {(o % 16, b) for o, b in probes}
    for r in range(min(16, sb)):
        for b in range(8):
            if (r, b) not in pairs:
                cnt = (sb - r + 15) // 16  # the offsets of that residue
                add(r + 16 * ((r * 8 + b) % cnt), b)
    probes.sort()
    _assert_coverage(probes, sb, seg)
    return probes


def coarse_positions(sb, seg=SEG):
    """One probe per (segment, pass of seg / 4 bytes): for the sweeps whose subject is the rows,
    not the byte slots. The offset walks through the pass and its two chunk halves."""
    out, step = [], seg // PASSES
    for i, base in enumerate(range(0, sb, step)):
        width = min(step, sb - base)
        out.append((base + (i * 1337 + 40) % width, (i * 3 + 1) % 8))
    return out


# -------------------------------------------------------------------------- batch
class Batch:
    """n = len(probes) + 3 stripes of RS(k, m): slots[s] is the probe of stripe s, None for the
    three clean ones. data and par are read-only and shared by the sweeps that do not change them."""

    def __init__(self, k, m, sb, probes, seed=None, seg=SEG):
        assert len(probes) >= 4 and O.use_high_rate(k, m) == 1  # the oracle pins high-rate parity only
        self.k, self.m, self.sb, self.seg, self.probes = k, m, sb, seg, list(probes)
        n = self.n = len(probes) + 3
        clean_at = {1, n // 2, n - 2}
        assert len(clean_at) == 3
        it = iter(range(len(probes)))
        self.slots = [None if s in clean_at else next(it) for s in range(n)]
        seed = k * 1000 + m * 10 + sb + 3 if seed is None else seed
        self.data = splitmix_bytes(seed, n * k * sb).reshape(n, k, sb)
        self.par = O.encode_batch(k, m, self.data, threads=4)
        self.data.setflags(write=False)
        self.par.setflags(write=False)

    def probed(self):
        """(stripe, offset, bit) of every probed stripe"""
        return [(s, *self.probes[pi][:2]) for s, pi in enumerate(self.slots) if pi is not None]


class Sweep:
    def __init__(self, name, batch, data, stored, stripes, flags, located):
        self.name, self.batch = name, batch
        self.k, self.m, self.sb, self.seg, self.n = batch.k, batch.m, batch.sb, batch.seg, batch.n
        self.data, self.stored, self.stripes = data, stored, stripes
        self.flags, self.located = flags, located
        self.nprobes = sum(p is not None for p in stripes)
        assert self.nprobes == len(batch.probes)  # no probe is dropped on the way
        self.present = np.ones((self.n, self.k + self.m), np.uint8)
        for s in np.flatnonzero(located >= 0):
            self.present[s, located[s]] = 0
        self.counts = class_counts(located)
        for a in (self.data, self.stored, self.flags, self.located, self.present):
            a.setflags(write=False)
        self._syndromes = None

    def syndromes(self):
        """encode(data) ^ stored [n, m, sb] by the oracle, computed once"""
        if self._syndromes is None:
            self._syndromes = O.encode_batch(self.k, self.m, self.data, threads=4) ^ self.stored
        return self._syndromes

    def error(self, failures):
        return ScrubSweepError(failures, self.sb, self.seg)


def class_counts(located):
    loc = np.asarray(located)
    return [int((loc == CLEAN).sum()), int((loc >= 0).sum()), int((loc == RECOVERY_SET).sum()),
            int((loc == UNLOCATED).sum())]


def _flip(arr, hits):
    """arr[s, row, o] ^= mask for every (s, row, o, mask): one stripe each, so no index repeats"""
    s, row, o, mask = (np.array(x) for x in zip(*hits))
    assert len(set(s.tolist())) == len(s)
    arr[s, row, o] ^= mask.astype(np.uint8)


def _blank(b):
    return [None] * b.n, np.zeros((b.n, b.m), np.uint8), np.full(b.n, CLEAN, np.int32)


def recovery_sweep(b):
    stripes, flags, located = _blank(b)
    stored, hits = b.par.copy(), []
    for s, o, bit in b.probed():
        r = s % b.m
        hits.append((s, r, o, 1 << bit))
        stripes[s] = Stripe(o, bit, b.k + r, None)
        flags[s, r] = 1
        located[s] = b.k + r if b.m >= 2 else UNLOCATED
    _flip(stored, hits)
    return Sweep("recovery", b, b.data, stored, stripes, flags, located)


def original_sweep(b):
    stripes, flags, located = _blank(b)
    data, hits = b.data.copy(), []
    for s, o, bit in b.probed():
        j = s % b.k
        hits.append((s, j, o, 1 << bit))
        stripes[s] = Stripe(o, bit, j, None)
        flags[s] = 1  # every coefficient c[r][j] is nonzero
        located[s] = j if b.m >= 2 else UNLOCATED
    _flip(data, hits)
    return Sweep("original", b, data, b.par, stripes, flags, located)


def reject_sweep(b, rows=None):
    """rows: the recovery row of each probe (default 1 + s % (m - 1)). The anchor alternates
    between byte 0 and the shard's last byte and moves to the other one where the probe lies in
    its symbol; a shard of one symbol (sb == 2) has no other, and its probes hit the anchor's
    symbol itself (then classify finds no ratio: check_locate asks the reference)."""
    assert b.m >= 2
    stripes, flags, located = _blank(b)
    data, stored, dhits, rhits = b.data.copy(), b.par.copy(), [], []
    for s, o, bit in b.probed():
        j = s % b.k
        r = 1 + s % (b.m - 1) if rows is None else rows[b.slots[s]]
        assert 1 <= r < b.m
        a, other = (0, b.sb - 1) if s % 2 == 0 else (b.sb - 1, 0)
        if symbol_of(b.sb, a) == symbol_of(b.sb, o):
            a = other
        assert symbol_of(b.sb, a) != symbol_of(b.sb, o) or b.sb == 2
        dhits.append((s, j, a, 1 + s * 37 % 255))
        rhits.append((s, r, o, 1 << bit))
        stripes[s] = Stripe(o, bit, b.k + r, a)
        flags[s] = 1
        located[s] = UNLOCATED
    _flip(data, dhits)
    _flip(stored, rhits)
    return Sweep("reject", b, data, stored, stripes, flags, located)


def mixing_originals(code):
    """The originals whose ratio c[1][j] / c[0][j] lies outside GF(2^8), the subfield the low
    bytes span. Only there does a wrong pairing of a symbol's two bytes give a wrong ratio: a
    multiplication by a subfield element never mixes the bytes, so the quotient of two high bytes
    alone is already right. RS(3, 2) has none; RS(200, 55) has the originals at positions past 255."""
    return [j for j in range(code.k) if code.exp[code.dl[1, j]] > 255]


def highbyte_sweep(b, originals=None):
    """originals: the originals the stripes rotate over (default: mixing_originals)"""
    assert b.m >= 2
    code = model(b.k, b.m)
    originals = mixing_originals(code) if originals is None else list(originals)
    assert originals, "no original of this code tells a symbol's high byte from its low byte"
    stripes, flags, located = _blank(b)
    data, lo_hits, hi_hits = b.data.copy(), [], []
    for s, o, bit in b.probed():
        j = originals[s % len(originals)]
        lo, hi = symbol_bytes(b.sb, symbol_of(b.sb, o))
        err = code.error_for(j, (1 + s * 29 % 255) << 8)
        lo_hits.append((s, j, lo, err & 0xFF))
        hi_hits.append((s, j, hi, err >> 8))
        stripes[s] = Stripe(hi, bit, j, None)
        flags[s] = 1
        located[s] = j
    _flip(data, lo_hits)
    _flip(data, hi_hits)
    sweep = Sweep("highbyte", b, data, b.par, stripes, flags, located)
    S0 = sweep.syndromes()[:, 0]
    for s, p in enumerate(stripes):  # the first nonzero byte of S_0 is the symbol's high byte
        assert p is None or int(np.flatnonzero(S0[s])[0]) == p.offset, (s, p)
    return sweep


# --------------------------------------------------------------- reference back ends
@functools.lru_cache(maxsize=None)
def model(k, m, cls=Code):
    return cls(k, m)


def verify_reference(k, m, data, stored):
    flags = (stored != O.encode_batch(k, m, data, threads=4)).any(axis=2)
    return flags.astype(np.uint8), int(flags.sum()), True


def locate_answers(code, S):
    """the model's answer per stripe of the syndromes S [n, m, sb] -> (located, present)"""
    n, m, _ = S.shape
    located = np.full(n, CLEAN, np.int32)
    present = np.ones((n, code.k + m), np.uint8)
    bad = S.any(axis=2)
    for s in np.flatnonzero(bad.any(axis=1)):
        loc = located[s] = code.locate_syndromes(S[s])
        if loc >= 0:
            present[s, loc] = 0
        elif loc == RECOVERY_SET:
            present[s, code.k:] = ~bad[s]
    return located, present


def locate_reference(cls=Code):
    """the locate back end of a model class (Code, or a mutant of it)"""
    def run(k, m, data, stored):
        located, present = locate_answers(model(k, m, cls), O.encode_batch(k, m, data, threads=4) ^ stored)
        return located, present, class_counts(located), True
    return run


def multi_as_locate(backend):
    """The multi-shard entry point at max_t = 1 as a locate back end. backend: (k, m, data, stored)
    -> (count [n], located [n, 1], present [n, k + m], counts [3], inputs_unchanged). count 0 is
    CLEAN, count 1 the located shard, unlocated stays UNLOCATED; counts [clean, one, unlocated]
    become [clean, one, 0, unlocated]: the multi form has no RECOVERY_SET class."""
    def run(k, m, data, stored):
        count, located, present, counts, unchanged = backend(k, m, data, stored)
        count, located = np.asarray(count), np.asarray(located)
        assert located.shape == (count.shape[0], 1) and len(counts) == 3
        assert np.isin(count, (0, 1, UNLOCATED)).all(), np.unique(count)
        one = np.where(count == 1, located[:, 0], UNLOCATED)
        loc = np.where(count == 0, CLEAN, one).astype(np.int32)
        return loc, present, [counts[0], counts[1], 0, counts[2]], unchanged
    return run


def locate_multi_answers(code, S):
    """the multi model's answer at max_t = 1 per stripe of the syndromes S [n, m, sb], in locate's
    form -> (located, present)"""
    n, m, _ = S.shape
    located = np.full(n, CLEAN, np.int32)
    present = np.ones((n, code.k + m), np.uint8)
    for s in np.flatnonzero(S.any(axis=(1, 2))):
        count, T = code.locate_multi_syndromes(S[s], 1)
        if count == 1:
            located[s], present[s, T[0]] = T[0], 0
        elif count != 0:  # 0: a model that reads less than the whole stripe may see nothing
            located[s] = UNLOCATED
    return located, present


def locate_multi_reference(cls=MultiCode):
    """the locate back end of a multi model class (MultiCode, or a mutant of it) at max_t = 1"""
    def run(k, m, data, stored):
        located, present = locate_multi_answers(model(k, m, cls), O.encode_batch(k, m, data, threads=4) ^ stored)
        return located, present, class_counts(located), True
    return run


# ------------------------------------------------------------------------ checker
def _judge(sweep, rows_differ, what):
    """every stripe is judged: rows_differ [n] bool -> the failures, after the count of probed
    stripes seen is compared with the probes generated"""
    assert rows_differ.shape == (sweep.n,)
    judged, failures = 0, []
    for s, p in enumerate(sweep.stripes):
        judged += p is not None
        if rows_differ[s]:
            failures.append((sweep.name, s, p, what(s)))
    if judged != len(sweep.batch.probes):
        raise AssertionError(f"{sweep.name} sweep: {judged} stripes judged, {len(sweep.batch.probes)} probes generated")
    return failures


def check_verify(sweep, backend):
    """Run a verify back end on the sweep: exactly the expected flags, the count they imply,
    inputs unwritten. Raises ScrubSweepError naming every stripe that differs."""
    flags, count, unchanged = backend(sweep.k, sweep.m, sweep.data, sweep.stored)
    flags = np.asarray(flags)
    assert flags.shape == sweep.flags.shape, flags.shape
    failures = _judge(sweep, (flags != sweep.flags).any(axis=1),
                      lambda s: f"verify flags {flags[s].tolist()}, expected {sweep.flags[s].tolist()}")
    if failures:
        raise sweep.error(failures)
    assert int(count) == int(sweep.flags.sum()), (sweep.name, count, int(sweep.flags.sum()))
    assert unchanged, f"{sweep.name} sweep: verify wrote an input"


def check_locate(sweep, backend, reference=Code):
    """Run a locate back end on the sweep: exactly the expected answers and present rows, the
    counts they imply, inputs unwritten. For the sweeps whose expectation rests on more than one
    flipped bit (reject, highbyte) the model of the back end under test must give it for every
    stripe first: reference is that model's class, Code for locate, MultiCode for the multi-shard
    locate at max_t = 1."""
    if sweep.name in ("reject", "highbyte"):
        answers = locate_multi_answers if issubclass(reference, MultiCode) else locate_answers
        ref, _ = answers(model(sweep.k, sweep.m, reference), sweep.syndromes())
        failures = _judge(sweep, ref != sweep.located, lambda s: f"the reference back end says {ref[s]}, the sweep "
                          f"expects {sweep.located[s]}: a degenerate probe")
        if failures:
            raise sweep.error(failures)
    located, present, counts, unchanged = backend(sweep.k, sweep.m, sweep.data, sweep.stored)
    located, present = np.asarray(located), np.asarray(present)
    assert located.shape == sweep.located.shape and present.shape == sweep.present.shape
    failures = _judge(sweep, located != sweep.located, lambda s: f"located {located[s]}, expected {sweep.located[s]}")
    failures += _judge(sweep, (present != sweep.present).any(axis=1) & (located == sweep.located),
                       lambda s: f"present row {present[s].tolist()}, expected {sweep.present[s].tolist()}")
    if failures:
        raise sweep.error(failures)
    assert [int(c) for c in counts] == sweep.counts, (sweep.name, counts, sweep.counts)
    assert unchanged, f"{sweep.name} sweep: locate wrote an input"
