"""The device entry points on 4- and 8-byte-aligned layouts (include/reedsol.h, "Alignment"):
rs_encode_batch_dev, rs_reconstruct_batch_dev, rs_reconstruct_batch_dev_patterns and
rs_verify_batch_dev with bases and stripe strides below 16-byte alignment, one case per
table-kernel family and layout class of tests/layout_contract.py. Bit-exact: parity against the
CPU oracle through check_encode, restored shards against the true data through
check_reconstruct (two poisons of the missing slots, guard-filled outputs), every array in a
guard-framed allocation at the class's offset with random or guard bytes in the stride padding.
Each case asserts the kernels it launched (rs_last_kernels): no hipRTC kernel and no `_nv`
wider than the layout allows, and the family it names did launch.

Also: one pattern used on aligned and misaligned buffers in turn (the plan cache must serve
both), and the layouts the entry points reject (2-byte alignment), which must write nothing."""
import ctypes as C

import numpy as np
import pytest

from layout_contract import (BUFFERS, FRAME, Placed, assert_class, check_encode, check_kernels, layout, pads_for,
                             place)
from slot_contract import GUARD, check_reconstruct

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import oracle as O  # noqa: E402
from rs_amd import reedsol_amd as R  # noqa: E402  (after torch: share its HIP runtime)
from test_gpu_missing_slots import every, expected_rows, ptr, set_knobs, stripe_patterns, truth  # noqa: E402

DEV = torch.device("cuda:0")
INVALID_ARGUMENT = 14
TABLE = ("encode_", "decode_", "low_blocks")  # the precompiled table kernels' names


def lay_of(name):
    """"A4", "ONE8-recovery", ... -> the Layout."""
    cls, _, which = name.partition("-")
    return layout(cls, which or None)


def sync_frames(placed, names):
    torch.cuda.synchronize()
    errors = [e for p, name in zip(placed, names) for e in p.frame_errors(name)]
    assert not errors, errors


# ------------------------------------------------------------ rs_encode_batch_dev
def encode_truth(k, m, sb, n, flags):
    """(data, parity): the oracle's encode_batch (shared with the reconstruct cases), for
    low-rate codes its encode_low stripe by stripe."""
    if R.use_high_rate(k, m):
        shards = truth(k, m, sb, n, flags)
        return shards[:, :k], shards[:, k:]
    data = np.random.default_rng(k * 7 + m + sb).integers(0, 256, (n, k, sb), dtype=np.uint8)
    rows = []
    for stripe in data:
        st, par = O.encode_low(k, m, stripe)
        assert st == 0
        rows.append(par)
    return data, np.stack(rows)


def encode_case(monkeypatch, k, m, sb, lay, want, env=None, flags=0, n=3, tail=False, forbid=()):
    set_knobs(monkeypatch, env or {})
    data, expected = encode_truth(k, m, sb, n, flags)
    ran = []

    def run(orig, par):
        placed = o, p = place((orig, par), lay, DEV, BUFFERS[:2])
        if not tail:
            assert_class(lay, (o.t, p.t))
        st = R.lib().rs_encode_batch_dev(k, m, sb, n, ptr(o.t), o.t.stride(0), ptr(p.t), p.t.stride(0), flags, None)
        assert st == 0, R.lib().rs_last_error()
        ran.append(R.last_kernels())
        sync_frames(placed, BUFFERS[:2])
        return o.numpy(), p.numpy()

    try:
        check_encode(run, k, m, data, expected, pads=pads_for(lay)[:2])
    finally:
        print(f"\nFAMILY encode {lay.name} {k},{m} sb {sb} flags {flags} {env or {}}: {ran}")
    check_kernels(ran, lay.max_nv, want, forbid, padded_copies=tail)


def ecase(id, k, m, sb, want8, want4, env=None, flags=0):
    """-> one parameter set per layout class: (A8, want8) and (A4, want4)."""
    return [pytest.param(k, m, sb, name, [want], env, flags, id=f"{id}-{name}")
            for name, want in (("A8", want8), ("A4", want4)) if want]


NV2, NV4 = {"RS_AMD_NV": "2"}, {"RS_AMD_NV": "4"}
ENCODE_CASES = sum([
    ecase("reg-contig", 10, 4, 4096, "encode_reg_w4_nv2", "encode_reg_w4_nv1"),
    # split lanes: 8256 = 129 chunks, no multiple of 512, and a 1024-byte wave leaves 960 of 9216
    # bytes idle (<= 1/8: fit_nv keeps 2); 192: 832 of 1024 idle, one dword pair
    ecase("reg-split-8256", 10, 4, 8256, "encode_reg_w4_nv2", "encode_reg_w4_nv1"),
    ecase("reg-split-192", 10, 4, 192, "encode_reg_w4_nv1", "encode_reg_w4_nv1"),
    ecase("reg-w1", 2, 1, 4096, "encode_reg_w1_nv2", "encode_reg_w1_nv1"),
    ecase("reg-w8", 9, 8, 4096, "encode_reg_w8_nv2", "encode_reg_w8_nv1"),
    ecase("reg-w16", 16, 16, 4096, "encode_reg_w16_nv1", "encode_reg_w16_nv1"),  # 2 * 16 slots: one pair (clamp_nv)
    ecase("reg-w32", 33, 32, 4096, "encode_reg_w32_nv1", "encode_reg_w32_nv1"),
    ecase("ws64", 70, 40, 1024, "encode_ws64_nv2", "encode_ws64_nv1", NV2),
    ecase("generic-sb192", 70, 40, 192, "encode_generic_nv1", "encode_generic_nv1"),
    ecase("generic-c128", 65, 70, 192, "encode_generic_nv1", "encode_generic_nv1"),
    # RS(70,65): equal chunks and k > m, a low-rate code here (rs_use_high_rate)
    ecase("low-generic-rs70_65", 70, 65, 192, "encode_low_generic_nv1", "encode_low_generic_nv1"),
    ecase("low-reg", 3, 5, 4096, "encode_low_reg_w4_nv2", "encode_low_reg_w4_nv1"),
    ecase("low-generic", 40, 100, 192, "encode_low_generic_nv1", "encode_low_generic_nv1"),
    ecase("nv4-forced", 10, 4, 4096, "encode_reg_w4_nv2", "encode_reg_w4_nv1", NV4),
    ecase("flags3", 10, 4, 4096, "encode_reg_w4_nv2", "encode_reg_w4_nv1", flags=3),
], [])


@pytest.mark.parametrize("k,m,sb,name,want,env,flags", ENCODE_CASES)
def test_encode(monkeypatch, k, m, sb, name, want, env, flags):
    encode_case(monkeypatch, k, m, sb, lay_of(name), want, env, flags)


@pytest.mark.parametrize("which", BUFFERS[:2])
@pytest.mark.parametrize("cls,nv", [("ONE8", 2), ("ONE4", 1), ("STRIDE4", 1)])
def test_encode_one_buffer(monkeypatch, cls, nv, which):
    """One misaligned base or stride among the call's two buffers pulls the lane width down."""
    encode_case(monkeypatch, 10, 4, 4096, layout(cls, which), [f"encode_reg_w4_nv{nv}"])


def test_encode_tail(monkeypatch):
    """sb 70: k_tail_pack copies from and to the caller's rows; the encode itself runs on the
    library's aligned padded copies, so its kernel may be a hipRTC one."""
    encode_case(monkeypatch, 10, 4, 70, layout("A4"), ["k_tail_pack"], tail=True)


# ------------------------------------------------------------ rs_reconstruct_batch_dev
def laid_run(call, ran, lay, whole=True):
    """run() of check_reconstruct on the GPU with every array at the layout's offset."""
    def run(orig, rec, out):
        placed = o, r, t = place((orig, rec, out), lay, DEV)
        if whole:
            assert_class(lay, (o.t, r.t, t.t))
        call(o.t, r.t, t.t)
        ran.append(R.last_kernels())
        sync_frames(placed, BUFFERS)
        return o.numpy(), r.numpy(), t.numpy()
    return run


def reconstruct_case(monkeypatch, k, m, sb, lost, lost_rec, lay, want, env=None, n=3, flags=0, forbid=(),
                     null_original=False, knobs=True):
    if knobs:
        set_knobs(monkeypatch, env or {})
    shards = truth(k, m, sb, n, flags)
    present = np.ones(k + m, np.uint8)
    present[lost] = 0
    present[np.array(lost_rec, dtype=int) + k] = 0
    assert lost and int(present.sum()) >= k
    ran = []

    def call(o, r, t):
        st = R.lib().rs_reconstruct_batch_dev(k, m, sb, n, C.c_void_p(present.ctypes.data),
                                              None if null_original else ptr(o), o.stride(0), ptr(r), r.stride(0),
                                              ptr(t), t.stride(0), flags, None)
        assert st == 0, R.lib().rs_last_error()

    try:
        check_reconstruct(laid_run(call, ran, lay, sb % 64 == 0), k, m, shards, present, shards[:, sorted(lost)],
                          pads=pads_for(lay))
    finally:
        print(f"\nFAMILY batch_dev {lay.name} {k},{m} sb {sb} flags {flags} {env or {}}: {ran}")
    check_kernels(ran, lay.max_nv, want, forbid, padded_copies=sb % 64 != 0)


def rcase(id, k, m, sb, lost, lost_rec, want8, want4, env=None):
    return [pytest.param(k, m, sb, sorted(lost), sorted(lost_rec), name, want, env, id=f"{id}-{name}")
            for name, want in (("A8", want8), ("A4", want4)) if want]


FFT = {"RS_AMD_DECODE": "fft"}
LOW_BLOCKS = {"RS_AMD_LOW_BLOCK": "1", "RS_AMD_JIT": "0"}
LOW_TAIL = sorted(set(range(100)) - {12, 51, 94})  # 97 of RS(100,600)'s originals lost
# The loss patterns differ from those of test_gpu_missing_slots.py, so their plans are new in a
# run of the whole suite. "= k": exactly k shards present.
RECONSTRUCT_CASES = sum([
    rcase("decode_reg", 10, 4, 4096, [2, 6], [1, 3], ["decode_reg_w16_nv2"], ["decode_reg_w16_nv1"], FFT),  # = k
    rcase("decode_reg-sb192", 10, 4, 192, [2, 6], [1, 3], ["decode_reg_w16_nv1"], ["decode_reg_w16_nv1"], FFT),
    # no knob: a network on aligned buffers
    rcase("decode_matrix", 10, 4, 4096, [2, 5, 7], [3], ["decode_matrix_e3_nv2"], ["decode_matrix_e3_nv1"]),  # = k
    rcase("decode_mtile", 70, 40, 1024, every(3, 20, 2), every(2, 20, 1), ["decode_mtile16_nv2"], None,
          {"RS_AMD_DECODE": "matrix", "RS_AMD_NV": "2"}),  # = k
    rcase("decode_mtile", 70, 40, 1024, every(3, 20, 2), every(2, 20, 1), None, ["decode_mtile16_nv1"],
          {"RS_AMD_DECODE": "matrix"}),
    rcase("syndrome-tables", 70, 33, 1024, every(3, 20, 1), every(2, 13, 1), ["encode_ws64_nv1", "decode_mtile16_nv1"],
          ["encode_ws64_nv1", "decode_mtile16_nv1"], {"RS_AMD_DECODE": "syndrome"}),  # = k
    # wide codes, no knob: the fused FFT reconstruct on aligned buffers; here the full plan's
    # table kernels (as observed on the GPU)
    rcase("wide-rs33_17", 33, 17, 4096, [1, 6, 12, 18, 24, 30], [1, 5], ["decode_matrix_e6_nv2"],
          ["decode_matrix_e6_nv1"]),
    rcase("wide-rs200_55", 200, 55, 4096, every(6, 32, 1), [1, 4], ["encode_ws64_nv1", "decode_mtile16_nv1"],
          ["encode_ws64_nv1", "decode_mtile16_nv1"]),  # the syndrome path on the table kernels
    rcase("decode_generic", 100, 20, 192, [1, 30, 33, 62, 65, 94, 97, 98], [1, 4, 5, 8, 18], ["decode_generic_nv1"],
          ["decode_generic_nv1"], FFT),
    rcase("low-decode_reg", 3, 5, 4096, [0, 1], [1, 2, 4], ["decode_reg_w16_nv2"], ["decode_reg_w16_nv1"]),  # = k
    rcase("low-decode_generic", 40, 100, 192, every(4, 10, 1), every(1, 20, 1) + [25, 98], ["decode_generic_nv1"],
          ["decode_generic_nv1"]),
    rcase("low-blocks", 100, 600, 2048, LOW_TAIL, every(1, 500), ["low_blocks"], ["low_blocks"], LOW_BLOCKS),
], [])


@pytest.mark.parametrize("k,m,sb,lost,lost_rec,name,want,env", RECONSTRUCT_CASES)
def test_reconstruct(monkeypatch, k, m, sb, lost, lost_rec, name, want, env):
    reconstruct_case(monkeypatch, k, m, sb, lost, lost_rec, lay_of(name), want, env)


@pytest.mark.parametrize("which", BUFFERS)
@pytest.mark.parametrize("cls,nv", [("ONE8", 2), ("ONE4", 1), ("STRIDE4", 1)])
def test_reconstruct_one_buffer(monkeypatch, cls, nv, which):
    """One misaligned base or stride among the call's three buffers, no knob set: the matrix
    kernel at the narrower width, not the pattern's network."""
    reconstruct_case(monkeypatch, 10, 4, 4096, [3, 5, 8], [0], layout(cls, which), [f"decode_matrix_e3_nv{nv}"])


def test_reconstruct_tail(monkeypatch):
    reconstruct_case(monkeypatch, 10, 4, 70, [2, 8], [1, 3], layout("A4"), ["k_tail_pack"])


@pytest.mark.parametrize("null_original", [False, True], ids=["d_original", "d_original-NULL"])
def test_reconstruct_every_original_lost(monkeypatch, null_original):
    """RS(16,16), all 16 originals lost, all recovery rows present: the inverse FFT kernel on
    aligned buffers, the tiled matrix kernel here; d_original may be NULL when no original is
    present."""
    reconstruct_case(monkeypatch, 16, 16, 1024, list(range(16)), [], layout("A4"), ["decode_mtile16_nv1"],
                     null_original=null_original)


# ------------------------------------------------------------ rs_reconstruct_batch_dev_patterns
def patterns_case(monkeypatch, k, m, sb, max_e, lay, aligned_path, want, env=None):
    set_knobs(monkeypatch, dict({"RS_AMD_JIT_SYNC": "1"}, **(env or {})))
    n, flags = 7, 0
    path = R.patterns_kernel_name(k, m, sb, max_e, flags)  # what 16-byte alignment would run
    assert aligned_path in (None, path), path
    shards = truth(k, m, sb, n, flags)
    present, want_status = stripe_patterns(k, m, max_e)
    expected = [expected_rows(k, m, flags, present[s], shards[s])[:max_e] if want_status[s] != 2 else shards[s, :0]
                for s in range(n)]
    rows = np.random.default_rng(k + m).integers(1, 256, (n, k + m + 9), dtype=np.uint8)
    rows[:, :k + m] = present
    d_present = torch.from_numpy(rows).to(DEV)
    ran, statuses = [], []

    def call(o, r, t):
        status = torch.full((n + 1,), -1, dtype=torch.int32, device=DEV)
        st = R.lib().rs_reconstruct_batch_dev_patterns(k, m, sb, n, ptr(d_present), d_present.stride(0), max_e, ptr(o),
                                                       o.stride(0), ptr(r), r.stride(0), ptr(t), t.stride(0),
                                                       ptr(status), flags, None)
        assert st == 0, R.lib().rs_last_error()
        statuses.append(status)

    try:
        check_reconstruct(laid_run(call, ran, lay, sb % 64 == 0), k, m, shards, present, expected, max_e=max_e,
                          pads=pads_for(lay))
    finally:
        print(f"\nFAMILY patterns {lay.name} {k},{m} sb {sb} max_e {max_e} {env or {}} "
              f"(aligned: {path}): {ran}")
    for status in statuses:
        assert status.cpu().tolist() == want_status + [-1]  # 0, 2 and 14 as on aligned buffers
    assert (d_present.cpu().numpy() == rows).all()
    check_kernels(ran, lay.max_nv, want, padded_copies=sb % 64 != 0)


def pcase(id, k, m, sb, max_e, aligned_path, want, env=None, layouts=("A8", "A4")):
    out = []
    for name in layouts:
        nv = lay_of(name).max_nv
        out.append(pytest.param(k, m, sb, max_e, name, aligned_path, [w.format(nv=nv) for w in want], env,
                                id=f"{id}-{name}"))
    return out


PFFT = {"RS_AMD_PATTERNS": "fft"}
PATTERN_CASES = sum([
    pcase("pattern_matrix", 10, 4, 4096, 4, "psyn_k10_m4", ["k_pattern_images", "decode_matrix_e4_nv{nv}"],
          layouts=("A8", "A4", "ONE4-restored", "ONE8-original", "STRIDE4-recovery")),
    pcase("pattern_fft", 10, 4, 4096, 4, "pattern_fft", ["k_pattern_tables", "decode_reg_w16_nv{nv}"], PFFT),
    pcase("pattern_fft-rs33_17", 33, 17, 4096, 8, None, ["k_pattern_tables", "decode_generic_nv1"]),
    pcase("pattern_fft_low", 3, 5, 4096, 2, "pattern_fft_low", ["k_pattern_tables", "decode_reg_w16_nv{nv}"]),
    pcase("tail", 10, 4, 70, 2, None, ["k_tail_pack"]),
], [])


@pytest.mark.parametrize("k,m,sb,max_e,name,aligned_path,want,env", PATTERN_CASES)
def test_patterns(monkeypatch, k, m, sb, max_e, name, aligned_path, want, env):
    patterns_case(monkeypatch, k, m, sb, max_e, lay_of(name), aligned_path, want, env)


# ------------------------------------------------------------ plan-cache order
# One process, one pattern, aligned and misaligned calls in turn: each step checks bytes and
# kernels. RS_AMD_JIT_SYNC=1: no pending compile decides the path.
# An aligned step must not be left on the table kernels (TABLE).
def sequence(monkeypatch, k, m, sb, lost, lost_rec, env, steps):
    set_knobs(monkeypatch, dict({"RS_AMD_JIT_SYNC": "1"}, **env))
    for name, want in steps:
        lay = lay_of(name)
        reconstruct_case(monkeypatch, k, m, sb, lost, lost_rec, lay, want, env, knobs=False,
                         forbid=TABLE if lay.max_nv == 4 else ())


def test_plan_order_rs10_4(monkeypatch):
    net = ["rs_net_reconstruct_i10_o2"]
    sequence(monkeypatch, 10, 4, 4096, [5, 7], [0, 3], {},
             [("ALIGNED", net), ("A4", ["decode_matrix_e2_nv1"]), ("ALIGNED", net)])


# after the full plan is in the cache: the fused kernel, or the pattern's own network / fused kernel
HIPRTC_RS33_17 = [("rs_fft_decode_k33_m17", "rs_fft_pdecode_k33_m17", "rs_net_reconstruct_i33_o5")]


@pytest.mark.parametrize("env,lost", [({"RS_AMD_FDEC": "1"}, [2, 9, 16, 23, 31]), ({}, [3, 10, 17, 24, 32])],
                         ids=["fdec1", "no-knob"])
def test_plan_order_rs33_17_aligned_first(monkeypatch, env, lost):
    """The aligned call leaves the pattern's lite plan (the fused kernel's block only); the
    misaligned call replaces it with the full plan; the next aligned call must still find a
    hipRTC kernel to run."""
    again = ["rs_fft_decode_k33_m17"] if env else HIPRTC_RS33_17  # RS_AMD_FDEC=1: the fused kernel, always
    sequence(monkeypatch, 33, 17, 4096, lost, [0, 6], env,
             [("ALIGNED", ["rs_fft_decode_k33_m17"]), ("A8", ["decode_matrix_e5_nv2"]), ("ALIGNED", again)])


def test_plan_order_rs33_17_misaligned_first(monkeypatch):
    """A pattern whose first call is misaligned gets the full plan at once; the aligned call
    after it must run the fused or network kernel, not the plan's table kernels."""
    sequence(monkeypatch, 33, 17, 4096, [4, 11, 18, 25, 29], [2, 7], {},
             [("A4", ["decode_matrix_e5_nv1"]), ("ALIGNED", HIPRTC_RS33_17)])


def test_plan_order_encode_rs200_55(monkeypatch):
    for name, want in (("ALIGNED", "rs_fft_encode_k200_m55"), ("A4", "encode_ws64_nv1"),
                       ("ALIGNED", "rs_fft_encode_k200_m55")):
        encode_case(monkeypatch, 200, 55, 4096, lay_of(name), [want], {"RS_AMD_JIT_SYNC": "1"},
                    forbid=TABLE if name == "ALIGNED" else ())


# ------------------------------------------------------------ rejected alignments
def guard_buffers(shapes, which, how):
    """Guard-filled device arrays [rows, stride] for the named buffers; `which` at base + 2
    (how == "base") or with a stride = 2 mod 4 (how == "stride")."""
    out = {}
    for name, (rows, width) in shapes.items():
        bad = name == which
        arr = np.full((rows, width + 64 + (2 if bad and how == "stride" else 0)), GUARD, np.uint8)
        out[name] = Placed(arr, 2 if bad and how == "base" else 0, DEV)
    t = out[which].t
    assert t.data_ptr() % 4 == (2 if how == "base" else 0) and t.stride(0) % 4 == (2 if how == "stride" else 0)
    return out


def assert_untouched(bufs, extra=()):
    torch.cuda.synchronize()
    for name, p in bufs.items():
        flat = p.flat.cpu().numpy()
        inside = flat[p.offset:p.offset + p.size]
        assert (inside == GUARD).all(), f"{name} was written"
        assert (np.delete(flat, np.s_[p.offset:p.offset + p.size]) == FRAME).all(), f"{name}: frame written"
    for name, t, fill in extra:
        assert (t.cpu().numpy() == fill).all(), f"{name} was written"


def assert_rejected(st):
    err = R.lib().rs_last_error().decode()
    assert st == INVALID_ARGUMENT, (st, err)
    assert "align" in err, err


REJECT = dict(k=10, m=4, sb=4096, n=3, e=2)


@pytest.mark.parametrize("how", ["base", "stride"])
@pytest.mark.parametrize("which", BUFFERS[:2])
def test_rejected_encode(monkeypatch, which, how):
    set_knobs(monkeypatch, {})
    k, m, sb, n = (REJECT[x] for x in ("k", "m", "sb", "n"))
    b = guard_buffers({"original": (n, k * sb), "recovery": (n, m * sb)}, which, how)
    o, r = b["original"].t, b["recovery"].t
    st = R.lib().rs_encode_batch_dev(k, m, sb, n, ptr(o), o.stride(0), ptr(r), r.stride(0), 0, None)
    assert_rejected(st)
    assert_untouched(b)


@pytest.mark.parametrize("how", ["base", "stride"])
@pytest.mark.parametrize("which", BUFFERS)
def test_rejected_reconstruct(monkeypatch, which, how):
    set_knobs(monkeypatch, {})
    k, m, sb, n, e = (REJECT[x] for x in ("k", "m", "sb", "n", "e"))
    present = np.ones(k + m, np.uint8)
    present[[1, 6]] = 0
    b = guard_buffers({"original": (n, k * sb), "recovery": (n, m * sb), "restored": (n, e * sb)}, which, how)
    o, r, t = (b[x].t for x in BUFFERS)
    st = R.lib().rs_reconstruct_batch_dev(k, m, sb, n, C.c_void_p(present.ctypes.data), ptr(o), o.stride(0), ptr(r),
                                          r.stride(0), ptr(t), t.stride(0), 0, None)
    assert_rejected(st)
    assert_untouched(b)


@pytest.mark.parametrize("how", ["base", "stride"])
@pytest.mark.parametrize("which", BUFFERS)
def test_rejected_patterns(monkeypatch, which, how):
    set_knobs(monkeypatch, {})
    k, m, sb, n, e = (REJECT[x] for x in ("k", "m", "sb", "n", "e"))
    present = np.ones((n, k + m), np.uint8)
    present[:, [1, 6]] = 0
    d_present = torch.from_numpy(present).to(DEV)
    status = torch.full((n + 1,), -7, dtype=torch.int32, device=DEV)
    b = guard_buffers({"original": (n, k * sb), "recovery": (n, m * sb), "restored": (n, e * sb)}, which, how)
    o, r, t = (b[x].t for x in BUFFERS)
    st = R.lib().rs_reconstruct_batch_dev_patterns(k, m, sb, n, ptr(d_present), 0, e, ptr(o), o.stride(0), ptr(r),
                                                   r.stride(0), ptr(t), t.stride(0), ptr(status), 0, None)
    assert_rejected(st)
    assert_untouched(b, [("d_status", status, -7)])


@pytest.mark.parametrize("how", ["base", "stride"])
def test_rejected_verify(monkeypatch, how):
    """d_original at + 2, or its stride = 2 mod 4: the call fails before d_bad is zeroed (a failed
    verify must not leave "all clean" flags behind)."""
    set_knobs(monkeypatch, {})
    k, m, sb, n = (REJECT[x] for x in ("k", "m", "sb", "n"))
    b = guard_buffers({"original": (n, k * sb), "recovery": (n, m * sb)}, "original", how)
    o, r = b["original"].t, b["recovery"].t
    bad = torch.full((n + 1, m + 3), GUARD, dtype=torch.uint8, device=DEV)
    count = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    for bad_stride in (bad.stride(0), 0):  # strided and packed flag rows (the two memsets)
        st = R.lib().rs_verify_batch_dev(k, m, sb, n, ptr(o), o.stride(0), ptr(r), r.stride(0), ptr(bad), bad_stride,
                                         ptr(count), 0, None)
        assert_rejected(st)
        assert_untouched(b, [("d_bad", bad, GUARD), ("d_bad_count", count, -7)])


def test_verify_recovery_at_2_is_legal(monkeypatch):
    """d_recovery only feeds the compare, which takes any alignment: stored parity at base + 2
    with an odd stride residue, one corrupt shard flagged."""
    set_knobs(monkeypatch, {})
    k, m, sb, n = (REJECT[x] for x in ("k", "m", "sb", "n"))
    shards = truth(k, m, sb, n)
    stored = shards[:, k:].copy()
    stored[1, 2, sb - 1] ^= 0x10
    rng = np.random.default_rng(77)
    rec = rng.integers(1, 256, (n, m * sb + 66), dtype=np.uint8)
    rec[:, :m * sb] = stored.reshape(n, -1)
    orig = rng.integers(1, 256, (n, k * sb + 256), dtype=np.uint8)
    orig[:, :k * sb] = shards[:, :k].reshape(n, -1)
    o, r = Placed(orig, 0, DEV), Placed(rec, 2, DEV)
    assert r.t.data_ptr() % 4 == 2 and r.t.stride(0) % 4 == 2
    bad = torch.full((n + 1, m + 3), GUARD, dtype=torch.uint8, device=DEV)
    count = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    st = R.lib().rs_verify_batch_dev(k, m, sb, n, ptr(o.t), o.t.stride(0), ptr(r.t), r.t.stride(0), ptr(bad),
                                     bad.stride(0), ptr(count), 0, None)
    assert st == 0, R.lib().rs_last_error()
    kernels = R.last_kernels()
    sync_frames((o, r), BUFFERS[:2])
    want = np.full((n + 1, m + 3), GUARD, np.uint8)
    want[:n, :m] = 0
    want[1, 2] = 1
    assert (bad.cpu().numpy() == want).all(), bad
    assert int(count.item()) == 1
    assert (o.numpy() == orig).all() and (r.numpy() == rec).all()
    assert any(x.startswith("k_verify_compare") for x in kernels), kernels
