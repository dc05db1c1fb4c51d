#!/usr/bin/env python3
"""The multi-shard locate next to verify and the single-shard locate, device-resident, per shape:
  verify            rs_verify_batch_dev (the yardstick: k + 3m rows per stripe)
  locate_clean      rs_locate_batch_dev on the clean batch
  locate_1          rs_locate_batch_dev, one corrupt original in every stripe
  multi_clean       rs_locate_multi_batch_dev (max_t 2) on the clean batch
  multi_1, multi_2  the same with one / two corrupt originals in every stripe
  multi4_4          max_t 4 with four corrupt originals in every stripe (codes with m >= 8)
Stripe s has bit 0 flipped at byte (7919 s + 62528 i) mod shard_bytes of original (s + i) mod k for
its i-th corrupt shard: different chunks, so the errors of a stripe are independent. Expected
traffic over verify's: clean 1, t corrupt shards (k + 3m + 2m (t + 1)) / (k + 3m).
The legs alternate in one process; each timed window is warmed, ends in a device synchronise and
lasts at least --window seconds. The set is repeated --sets times; per leg the median and the
min-max range of the per-call times are printed as one JSON line per shape.

    python tools/locate_multi_bench.py [--shapes K,M,SHARD_BYTES,STRIPES;...] [--out FILE]
    python tools/locate_multi_bench.py --only multi_1 --calls 5     (one leg alone, for a kernel trace)
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


def bench_shape(k, m, sb, n, sets, min_window, dev, only, calls):
    g = torch.Generator(device=dev)
    g.manual_seed(2025)
    data = torch.randint(0, 256, (n, k, sb), dtype=torch.uint8, device=dev, generator=g)
    parity = torch.empty((n, m, sb), dtype=torch.uint8, device=dev)
    R.encode_batch_dev(k, m, data, parity)
    idx = torch.arange(n, device=dev)
    bad = torch.empty((n, m), dtype=torch.uint8, device=dev)
    located = torch.empty((n,), dtype=torch.int32, device=dev)
    counts1 = torch.zeros(4, dtype=torch.int64, device=dev)
    count = torch.empty((n,), dtype=torch.int32, device=dev)

    def flip(t):
        """toggle the bits of t corrupt originals per stripe (its own inverse)"""
        for i in range(t):
            data[idx, (idx + i) % k, (idx * 7919 + 62528 * i) % sb] ^= 1

    def multi(max_t):
        loc = torch.empty((n, max_t), dtype=torch.int32, device=dev)
        counts = torch.zeros(max_t + 2, dtype=torch.int64, device=dev)

        def call():
            return R.locate_multi_batch_dev(k, m, data, parity, max_t, count=count, located=loc, counts=counts)
        return call, loc, counts

    multi2, loc2, counts2 = multi(2)
    # (corrupt originals per stripe, the call, rows of traffic per stripe)
    legs = {
        "verify": (0, lambda: R.verify_batch_dev(k, m, data, parity, bad=bad), k + 3 * m),
        "locate_clean": (0, lambda: R.locate_batch_dev(k, m, data, parity, located=located, counts=counts1), k + 3 * m),
        "locate_1": (1, lambda: R.locate_batch_dev(k, m, data, parity, located=located, counts=counts1), k + 5 * m),
        "multi_clean": (0, multi2, k + 3 * m),
        "multi_1": (1, multi2, k + 3 * m + 4 * m),
        "multi_2": (2, multi2, k + 3 * m + 6 * m),
    }
    if m >= 8:
        multi4, loc4, counts4 = multi(4)
        legs["multi4_4"] = (4, multi4, k + 3 * m + 10 * m)

    if only:  # a few calls of one leg and nothing else, for a kernel trace of that leg alone
        t, fn, _ = legs[only]
        flip(t)
        window(fn, calls)
        if only.startswith("multi"):
            assert bool((count == t).all().item()), only
        return {"shape": {"k": k, "m": m, "shard_bytes": sb, "stripes": n}, "only": only, "calls": calls,
                "kernels": R.last_kernels()}

    # the answers, before anything is timed
    assert not legs["verify"][1]().any().item()
    assert bool((legs["locate_clean"][1]() == R.LOCATE_CLEAN).all().item())
    assert bool((multi2() == 0).all().item()) and counts2.tolist() == [n, 0, 0, 0]
    kernels = {"multi_clean": R.last_kernels()}
    for name, t, loc, counts in [("multi_1", 1, loc2, counts2), ("multi_2", 2, loc2, counts2)] + \
            ([("multi4_4", 4, loc4, counts4)] if m >= 8 else []):
        flip(t)
        max_t = loc.shape[1]
        assert bool((legs[name][1]() == t).all().item()), name
        kernels[name] = R.last_kernels()
        want = torch.full((n, max_t), -1, dtype=torch.int32, device=dev)
        want[:, :t] = torch.sort(torch.stack([(idx + i) % k for i in range(t)], dim=1), dim=1).values.to(torch.int32)
        assert torch.equal(loc, want), name
        assert counts.tolist() == [n if c == t else 0 for c in range(max_t + 2)], name
        if t == 1:
            assert torch.equal(legs["locate_1"][1](), (idx % k).to(torch.int32))
        flip(t)

    reps = {}
    for name, (t, fn, _) in legs.items():  # warm, and size the windows
        flip(t)
        fn()
        reps[name] = max(2, math.ceil(min_window / (window(fn, 2) / 1e3)))
        flip(t)
    times = {name: [] for name in legs}
    for _ in range(sets):
        for name, (t, fn, _) in legs.items():
            flip(t)
            times[name].append(window(fn, reps[name]))
            flip(t)
    res = {"shape": {"k": k, "m": m, "shard_bytes": sb, "stripes": n}, "sets": sets, "window_s": min_window,
           "kernels": kernels, "kernel_name": R.locate_multi_kernel_name(k, m, sb, 2), "legs": {}}
    verify = statistics.median(times["verify"])
    for name, ts in times.items():
        res["legs"][name] = {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4),
                             "max_ms": round(max(ts), 4), "calls_per_window": reps[name],
                             "over_verify": round(statistics.median(ts) / verify, 4),
                             "traffic_over_verify": round(legs[name][2] / (k + 3 * m), 4)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="10,4,1048576,1024;200,55,262144,512", help="K,M,SHARD_BYTES,STRIPES;...")
    ap.add_argument("--sets", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="least seconds per timed window")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--only", default=None, help="run this leg alone, --calls times, untimed")
    ap.add_argument("--calls", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "locate_multi_bench needs a GPU"
    dev = torch.device("cuda:0")
    for shape in args.shapes.split(";"):
        k, m, sb, n = (int(x) for x in shape.split(","))
        line = json.dumps(bench_shape(k, m, sb, n, args.sets, args.window, dev, args.only, args.calls))
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
