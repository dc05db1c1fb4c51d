#!/usr/bin/env python3
"""Verify (scrub) against what a caller had to do before it, device-resident, per shape:
  (a) encode          rs_encode_batch_dev into a spare parity buffer
  (b) encode+compare  (a), then a per-shard `any` of spare != parity in torch
  (c) verify          rs_verify_batch_dev
  (d) locate_clean    rs_locate_batch_dev on the clean batch (k + 3m rows, as the verify)
  (e) locate_corrupt  rs_locate_batch_dev with one corrupt original in every stripe (every stripe
                      is a candidate: 2m more rows for the confirm, (k + 5m) / (k + 3m) of (c)'s traffic)
The legs alternate in one process; each timed window is warmed, ends in a device synchronise
and lasts at least --window seconds. The set is repeated --sets times; per leg the median and
the min-max spread of the per-call times are printed as one JSON line per shape.

    python tools/verify_bench.py [--shapes K,M,SHARD_BYTES,STRIPES;...] [--out FILE]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "reed-solomon-cc_amd"))
import reedsol_amd as R  # noqa: E402


def window(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def bench_shape(k, m, sb, n, sets, min_window, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(2025)
    data = torch.randint(0, 256, (n, k, sb), dtype=torch.uint8, device=dev, generator=g)
    parity = torch.empty((n, m, sb), dtype=torch.uint8, device=dev)
    spare = torch.empty((n, m, sb), dtype=torch.uint8, device=dev)
    bad = torch.empty((n, m), dtype=torch.uint8, device=dev)
    R.encode_batch_dev(k, m, data, parity)

    def leg_a():
        R.encode_batch_dev(k, m, data, spare)

    def leg_b():
        R.encode_batch_dev(k, m, data, spare)
        return (spare != parity).any(dim=2)

    def leg_c():
        return R.verify_batch_dev(k, m, data, parity, bad=bad)

    # the legs agree before anything is timed: clean parity, then one corrupted byte
    assert not leg_b().any().item() and not leg_c().any().item()
    kernels = R.last_kernels()
    parity[n - 1, m - 1, sb - 1] ^= 1
    assert torch.equal(leg_b().to(torch.uint8), leg_c()) and int(leg_c().sum().item()) == 1
    parity[n - 1, m - 1, sb - 1] ^= 1

    # locate: the clean batch, and a copy with one flipped bit in one original of every stripe
    located = torch.empty((n,), dtype=torch.int32, device=dev)
    counts = torch.zeros(4, dtype=torch.int64, device=dev)
    broken = data.clone()
    idx = torch.arange(n, device=dev)
    broken[idx, idx % k, (idx * 7919) % sb] ^= 1

    def leg_d():
        return R.locate_batch_dev(k, m, data, parity, located=located, counts=counts)

    def leg_e():
        return R.locate_batch_dev(k, m, broken, parity, located=located, counts=counts)

    assert bool((leg_d() == R.LOCATE_CLEAN).all().item()) and counts.tolist() == [n, 0, 0, 0]
    want = (idx % k).to(torch.int32) if m >= 2 else torch.full_like(located, R.LOCATE_UNLOCATED)
    assert torch.equal(leg_e(), want)
    locate_kernels = R.last_kernels()

    legs = {"encode": leg_a, "encode+compare": leg_b, "verify": leg_c, "locate_clean": leg_d,
            "locate_corrupt": leg_e}
    reps = {}
    for name, fn in legs.items():  # warm, and size the windows
        fn()
        reps[name] = max(2, math.ceil(min_window / (window(fn, 2) / 1e3)))
    times = {name: [] for name in legs}
    for _ in range(sets):
        for name, fn in legs.items():
            times[name].append(window(fn, reps[name]))
    res = {"shape": {"k": k, "m": m, "shard_bytes": sb, "stripes": n}, "verify_kernels": kernels,
           "verify_kernel_name": R.verify_kernel_name(k, m, sb), "sets": sets, "window_s": min_window, "legs": {}}
    for name, t in times.items():
        res["legs"][name] = {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4),
                             "max_ms": round(max(t), 4), "spread_ms": round(max(t) - min(t), 4),
                             "calls_per_window": reps[name]}
    b, c = res["legs"]["encode+compare"], res["legs"]["verify"]
    res["verify_beats_encode+compare_beyond_spreads"] = \
        b["median_ms"] - c["median_ms"] > b["spread_ms"] + c["spread_ms"]
    res["verify_over_encode"] = round(c["median_ms"] / res["legs"]["encode"]["median_ms"], 4)
    res["locate_kernels"] = locate_kernels
    res["locate_kernel_name"] = R.locate_kernel_name(k, m, sb)
    res["locate_clean_over_verify"] = round(res["legs"]["locate_clean"]["median_ms"] / c["median_ms"], 4)
    res["locate_corrupt_over_verify"] = round(res["legs"]["locate_corrupt"]["median_ms"] / c["median_ms"], 4)
    res["locate_corrupt_traffic_over_verify"] = round((k + 5 * m) / (k + 3 * m), 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="10,4,1048576,4096;200,55,262144,512",
                    help="K,M,SHARD_BYTES,STRIPES;... (default: the headline shape, then the c4 shape)")
    ap.add_argument("--sets", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="least seconds per timed window")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "verify_bench needs a GPU"
    dev = torch.device("cuda:0")
    for shape in args.shapes.split(";"):
        k, m, sb, n = (int(x) for x in shape.split(","))
        line = json.dumps(bench_shape(k, m, sb, n, args.sets, args.window, dev))
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
