"""The encode checker and the layout classes (tests/layout_contract.py) on the CPU: check_encode
passes a backend that keeps the contract (the oracle's encode) and rejects, by the intended
check, backends that break it in each of the ways a kernel on a narrow layout could: a wrong
byte in the last lanes of the last row, a store into the parity stride padding, into the guard
stripe past the batch, or into the input."""
import numpy as np
import pytest

from layout_contract import BUFFERS, EncodeContractError, align_nv, check_encode, check_kernels, layout, pads_for
from slot_contract import GUARD, stripe_rows

CODES = {"rs10_4": (10, 4, 0, 192), "rs10_4_d1d2": (10, 4, 3, 192), "rs33_17": (33, 17, 0, 128)}
N = 3


def case(oracle, name):
    k, m, flags, sb = CODES[name]
    data = np.random.default_rng(k * 100 + m + flags).integers(0, 256, (N, k, sb), dtype=np.uint8)
    return k, m, flags, sb, data, oracle.encode_batch(k, m, data, quirks=flags)


def oracle_backend(oracle, k, m, sb, flags, tamper=None):
    """run() for check_encode on oracle.encode_batch; tamper(orig, par) then breaks the contract
    on the buffers about to be returned."""
    def run(orig, par):
        n = orig.shape[0]
        par[:n, :m * sb] = oracle.encode_batch(k, m, stripe_rows(orig, k, sb), quirks=flags).reshape(n, -1)
        if tamper:
            tamper(orig, par)
        return orig, par
    return run


@pytest.mark.parametrize("name", list(CODES))
@pytest.mark.parametrize("pads", [(0, 0), (256, 64), (260, 76), (264, 72)])
def test_oracle_keeps_the_contract(oracle, name, pads):
    k, m, flags, sb, data, expected = case(oracle, name)
    par = check_encode(oracle_backend(oracle, k, m, sb, flags), k, m, data, expected, pads=pads)
    assert par.shape == (N + 1, m * sb + pads[1])


def rejected(oracle, tamper, pads=(260, 76)):
    k, m, flags, sb, data, expected = case(oracle, "rs10_4")
    with pytest.raises(EncodeContractError) as err:
        check_encode(oracle_backend(oracle, k, m, sb, flags, tamper), k, m, data, expected, pads=pads)
    return err.value


def test_rejects_wrong_byte_in_last_lanes(oracle):
    """One wrong byte among the last 16 of the last parity row of the last stripe: check 1."""
    k, m, _, sb = CODES["rs10_4"]
    for back in (1, 9, 16):
        def tamper(orig, par, back=back):
            par[N - 1, m * sb - back] ^= 0x20
        err = rejected(oracle, tamper)
        assert err.checks == {1} and f"row {m - 1} byte {sb - back}" in str(err), err


@pytest.mark.parametrize("at", [0, 7, 75])
def test_rejects_stride_padding_written(oracle, at):
    """A store into the parity stride padding (first, inner and last byte of it): check 3."""
    k, m, _, sb = CODES["rs10_4"]

    def tamper(orig, par):
        par[1, m * sb + at] = GUARD ^ 0xFF

    assert rejected(oracle, tamper).checks == {3}


def test_rejects_guard_stripe_written(oracle):
    """A store into the stripe past the batch, in its rows or in its padding: check 4."""
    k, m, _, sb = CODES["rs10_4"]
    for at in (0, m * sb - 1, m * sb + 75):
        def tamper(orig, par, at=at):
            par[N, at] = 0
        assert rejected(oracle, tamper).checks == {4}


@pytest.mark.parametrize("where", ["shard", "padding"])
def test_rejects_input_written(oracle, where):
    """One bit of an input shard, or of the input's stride padding: check 2."""
    k, m, _, sb = CODES["rs10_4"]

    def tamper(orig, par):
        orig[2, 3 * sb + 5 if where == "shard" else k * sb + 259] ^= 1

    assert rejected(oracle, tamper).checks == {2}


def test_every_failed_check_is_named(oracle):
    k, m, _, sb = CODES["rs10_4"]

    def tamper(orig, par):
        par[0, 0] ^= 1
        par[0, m * sb] = 0
        par[N, 5] = 0
        orig[0, 0] ^= 1

    err = rejected(oracle, tamper)
    assert err.checks == {1, 2, 3, 4} and err.check == 1
    assert all(f"check {c}:" in str(err) for c in (1, 2, 3, 4))


def test_guard_value_in_padding_is_not_a_false_alarm(oracle):
    """The input padding is random and nonzero, so a kernel that reads it as data cannot pass by
    luck of zeros; the parity's padding is GUARD everywhere."""
    k, m, flags, sb, data, expected = case(oracle, "rs10_4")
    seen = {}

    def run(orig, par):
        seen["orig"], seen["par"] = orig.copy(), par.copy()
        return oracle_backend(oracle, k, m, sb, flags)(orig, par)

    check_encode(run, k, m, data, expected, pads=(260, 76))
    assert (seen["orig"][:, k * sb:] != 0).all() and (seen["par"] == GUARD).all()


def test_kernel_name_assertions():
    """What a call that ignored the alignment would report is rejected: a hipRTC kernel, a
    table kernel wider than the layout allows, or the named family missing."""
    check_kernels([["encode_reg_w4_nv2"]], 2, ["encode_reg_w4_nv2"])
    check_kernels([["k_pattern_tables", "decode_reg_w16_nv1"]], 1, ["k_pattern_tables", ("decode_reg", "decode_matrix")])
    check_kernels([["rs_net_encode_i10_o4_ab12"]], 4, ["rs_net_encode_"], forbid=["encode_"])
    check_kernels([["k_tail_pack", "rs_net_encode_i10_o4_ab12", "encode_reg_w4_nv4"]], 1, ["k_tail_pack"],
                  padded_copies=True)
    for ran, max_nv, want in [
            ([["rs_net_encode_i10_o4_ab12"]], 2, []),             # a network on an 8-byte layout
            ([["rs_fft_encode_k200_m55_1f"]], 1, []),
            ([["k_psyn_plan", "rs_psyn_reconstruct_k10_m4_c3"]], 1, []),
            ([["encode_reg_w4_nv4"]], 2, []),                      # align_nv answering 4
            ([["encode_reg_w4_nv2"]], 1, []),
            ([["encode_reg_w4_nv1"], ["encode_reg_w4_nv2"]], 1, []),  # the second of two calls
            ([["encode_reg_w4_nv1"]], 2, ["encode_reg_w4_nv2"]),  # the named kernel did not launch
            ([[]], 1, []),
            ([], 1, [])]:
        with pytest.raises(AssertionError):
            check_kernels(ran, max_nv, want)
    with pytest.raises(AssertionError):
        check_kernels([["decode_matrix_e3_nv4"]], 4, ["rs_net_"], forbid=["decode_"])


def test_layout_classes():
    """The classes give the max_nv they state, for rows of whole 64-byte chunks on 16-byte
    aligned allocations, under the library's rule (align_nv: OR of every pointer and stride)."""
    base = 0x7F0000001000
    rows = (10 * 4096, 4 * 4096, 2 * 4096)

    def nv(lay):
        pads = pads_for(lay)
        return align_nv([base + o for o in lay.offsets] + [r + p for r, p in zip(rows, pads)])

    assert nv(layout("ALIGNED")) == 4
    assert nv(layout("A8")) == 2 and layout("A8").max_nv == 2
    a4 = layout("A4")
    assert nv(a4) == 1 and a4.max_nv == 1 and set(a4.residues) == {4, 12}
    for which in BUFFERS:
        for cls, want in (("ONE8", 2), ("ONE4", 1), ("STRIDE4", 1)):
            lay = layout(cls, which)
            assert nv(lay) == want == lay.max_nv, lay
            changed = [i for i in range(3) if lay.offsets[i] or lay.residues[i]]
            assert changed == [BUFFERS.index(which)], lay  # one buffer only
    assert align_nv([base + 2]) == 0 and align_nv([base, 40962]) == 0
