"""bench.py's command line: a plain run times its steps and prints the result line only;
--full adds the legs after the timed region; --dump-outputs writes what the last timed
step computed, the same from run to run. Tiny shapes, in process."""
import json

import numpy as np
import pytest

import bench

SHAPE = ["--stripes", "6", "--shard-bytes", "4096"]  # RS(10,4), erase 0,1,2,3
N, K, M, E, SB = 6, 10, 4, 4, 4096


def _run(capsys, *extra):
    bench.main(["--gpus", "1", "--steps", "2", "--warmup", "1", *SHAPE, *extra])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_options_default_to_a_plain_run():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert bench.parse(["--full", "--dump-outputs", "d"]).full


def test_dump_sample_is_fixed():
    a, b = bench.dump_sample(1 << 34, 1000, 0), bench.dump_sample(1 << 34, 1000, 0)
    assert a.dtype == np.int64 and (a == b).all() and (np.diff(a) >= 0).all()
    assert 0 <= a[0] and a[-1] < 1 << 34 and a[-1] > 1 << 32
    assert (a != bench.dump_sample(1 << 34, 1000, 1)).any()


@pytest.mark.gpu
def test_plain_run_and_dump(tmp_path, capsys, oracle):
    import torch

    res = _run(capsys, "--dump-outputs", str(tmp_path / "a"))
    assert res["steps"] == 2 and res["warmup"] == 1 and res["full"] is False
    assert res["unit"] == "GiB/s" and res["higher_is_better"] is True and res["dtype"] == "u8"
    assert res["ms_per_step"] > 0 and res["value"] > 0 and "RS(10,4)" in res["metric"]
    # value and ms_per_step describe the same timed steps (both are rounded in the line)
    gib = 2 * K * SB * N / 2**30 / (res["ms_per_step"] * 1e-3)
    assert gib == pytest.approx(res["value"], rel=0.05, abs=0.011)
    assert res["verified"] is None and res["cpu_baseline"] is None and res["c4_gpu"] is None

    par, rest = np.load(tmp_path / "a" / "parity.npy"), np.load(tmp_path / "a" / "restored.npy")
    assert par.dtype == np.float32 and par.shape == (N, M, SB)
    assert rest.dtype == np.float32 and rest.shape == (N, E, SB)
    # the bench's inputs, from its seed: the dump is the parity and the erased shards of them
    g = torch.Generator(device="cuda:0")
    g.manual_seed(0x5EED0000)
    data = torch.randint(0, 256, (N, K, SB), dtype=torch.uint8, device="cuda:0", generator=g).cpu().numpy()
    assert (rest == data[:, :E]).all()
    assert (par == oracle.encode_batch(K, M, data, threads=2)).all()

    # same arguments, same outputs; a small budget dumps the seeded sample of the same arrays
    bench.DUMP_BUDGET_BYTES, saved = 4 * 2 * 1000, bench.DUMP_BUDGET_BYTES
    try:
        for d in "bc":
            _run(capsys, "--dump-outputs", str(tmp_path / d))
    finally:
        bench.DUMP_BUDGET_BYTES = saved
    for i, (name, whole) in enumerate((("parity", par), ("restored", rest))):
        b, c = np.load(tmp_path / "b" / f"{name}.npy"), np.load(tmp_path / "c" / f"{name}.npy")
        assert b.dtype == np.float32 and b.shape == (1000,) and (b == c).all()
        assert (b == whole.reshape(-1)[bench.dump_sample(whole.size, 1000, i)]).all()


@pytest.mark.gpu
def test_full_run_verifies(capsys):
    res = _run(capsys, "--full", "--cpu-seconds", "0", "--c4-reps", "0")
    assert res["full"] is True and res["verified"] is True
