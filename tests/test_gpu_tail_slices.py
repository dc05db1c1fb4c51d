"""Shard tails over more than one slice. Batches whose shard_bytes is no multiple of 64 run on
padded copies in slices of at most 1 GiB (kTailSliceBytes, rs_host.hpp), a constant that
RS_AMD_SCRATCH_CAP_MB does not move, so only a batch this large reaches the tail loops' second
slice: RS(10,4), 65538-byte shards (padded to 65600), 1200 stripes, about 0.8 GB of originals.

Each entry point's one-call result must equal, byte for byte, the same batch run as two calls of
600 stripes (each under the cap: one slice), and the stripes either side of the slice boundary
plus the first and the last must be what the CPU oracle encodes / the original bytes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from rs_amd import reedsol_amd as R  # noqa: E402  (after torch: share its HIP runtime)

DEV = torch.device("cuda:0")
K, M, SB, N, HALF = 10, 4, 65538, 1200, 600
PSB = (SB + 63) // 64 * 64
TAIL_SLICE_BYTES = 1 << 30


def slice_plan(rows):
    """(stripes per slice, slices) of a tail loop that pads `rows` shards per stripe: the greedy
    rule, max(1, min(n, cap / stripe bytes))."""
    per = max(1, min(N, TAIL_SLICE_BYTES // (rows * PSB)))
    return per, -(-N // per)


def boundary_stripes(rows):
    per, slices = slice_plan(rows)
    assert slices >= 2, (per, slices)
    assert HALF <= per, "the two-call form must be one slice per call"
    return sorted({0, per - 1, per, N - 1})


@pytest.fixture(scope="module")
def batch():
    """Originals from a fixed seed, and their parity by two one-slice encodes."""
    g = torch.Generator(device=DEV)
    g.manual_seed(0x7A115)
    d = torch.randint(0, 256, (N, K, SB), dtype=torch.uint8, device=DEV, generator=g)
    p = torch.zeros((N, M, SB), dtype=torch.uint8, device=DEV)
    R.encode_batch_dev(K, M, d[:HALF], p[:HALF])
    R.encode_batch_dev(K, M, d[HALF:], p[HALF:])
    torch.cuda.synchronize()
    return d, p


def encode_case(oracle, batch):
    d, p_halves = batch
    idx = boundary_stripes(K + M)
    assert idx == [0, 1168, 1169, N - 1]
    p = torch.zeros_like(p_halves)
    R.encode_batch_dev(K, M, d, p)
    torch.cuda.synchronize()
    assert torch.equal(p, p_halves)
    exp = oracle.encode_batch(K, M, d[idx].cpu().numpy())
    assert (p[idx].cpu().numpy() == exp).all()


def reconstruct_case(oracle, batch):
    d, p = batch
    lost = [0, 1]
    idx = boundary_stripes(K + M + len(lost))
    assert idx == [0, 1022, 1023, N - 1]
    present = [0 if i in lost else 1 for i in range(K + M)]
    out = torch.zeros((N, len(lost), SB), dtype=torch.uint8, device=DEV)
    R.reconstruct_batch_dev(K, M, present, d, p, out)
    halves = torch.zeros_like(out)
    R.reconstruct_batch_dev(K, M, present, d[:HALF], p[:HALF], halves[:HALF])
    R.reconstruct_batch_dev(K, M, present, d[HALF:], p[HALF:], halves[HALF:])
    torch.cuda.synchronize()
    assert torch.equal(out, halves)
    assert (out[idx].cpu().numpy() == d[idx][:, lost].cpu().numpy()).all()


def patterns_case(oracle, batch):
    d, p = batch
    max_e = 2
    idx = boundary_stripes(K + M + max_e)
    assert idx == [0, 1022, 1023, N - 1]
    rng = np.random.default_rng(1200)
    present = np.ones((N, K + M), np.uint8)
    lost = np.stack([np.sort(rng.choice(K, size=max_e, replace=False)) for _ in range(N)])
    np.put_along_axis(present, lost, 0, axis=1)
    pres = torch.from_numpy(present).to(DEV)

    def run(lo, hi, out, status):
        R.reconstruct_batch_dev_patterns(K, M, pres[lo:hi], d[lo:hi], p[lo:hi], out[lo:hi], status[lo:hi])

    out = torch.full((N, max_e, SB), 0xAB, dtype=torch.uint8, device=DEV)
    status = torch.full((N,), -1, dtype=torch.int32, device=DEV)
    run(0, N, out, status)
    halves, status_halves = torch.full_like(out, 0xAB), torch.full_like(status, -1)
    run(0, HALF, halves, status_halves)
    run(HALF, N, halves, status_halves)
    torch.cuda.synchronize()
    assert not status.any().item() and not status_halves.any().item()
    assert torch.equal(out, halves)
    got, orig = out[idx].cpu().numpy(), d[idx].cpu().numpy()
    for i, s in enumerate(idx):
        assert (got[i] == orig[i][lost[s]]).all(), s


CASES = {"encode": encode_case, "reconstruct": reconstruct_case, "patterns": patterns_case}


@pytest.mark.parametrize("entry", list(CASES))
def test_tail_two_slices(oracle, batch, entry):
    """rs_encode_batch_dev, rs_reconstruct_batch_dev (originals 0 and 1 lost) and
    rs_reconstruct_batch_dev_patterns (max_e = 2, two originals lost per stripe)."""
    CASES[entry](oracle, batch)
