#!/usr/bin/env python3
"""Rebuild (every lost shard of a stripe, recovery shards included) against what a caller had to do
before it, device-resident, per shape and loss pattern:
  (a) rebuild    rs_rebuild_batch_dev into [n][max_e][sb]: k + e_s rows on the fast form
  (b) composed   rs_reconstruct_batch_dev_patterns of the missing originals, a copy of them into
                 their places, rs_encode_batch_dev of every stripe into a full m-row parity buffer,
                 a copy of the rows that were lost out of it: the entry points that existed before
                 the rebuild, and the yardstick. The two copies go through torch indexing (a gather and a
                 scatter each), which is far from copy speed on 1 MiB rows, so the tool also times
  (c) composed_kernels  the two library calls of (b) alone, no copy: below anything a composed route
                 can reach, whatever it copies with
Loss patterns: `rotate` (one shard per stripe, stripe s loses shard s mod (k + m): a failed node
under rotated parity), `parity` (one recovery shard per stripe), `2+2` (two originals and two
recovery shards per stripe), `mixedN` (N shards per stripe spread over originals and recovery).
Before anything is timed both routes must give the true originals and the encode's parity, byte for
byte. The legs alternate in one process; each timed window is warmed, ends in a device synchronise
and lasts at least --window seconds. The set is repeated --sets times; per leg the median and the
min-max range of the per-call times are printed as one JSON line per shape and pattern.

    python tools/rebuild_bench.py [--cases K,M,SHARD_BYTES,STRIPES,PATTERN;...] [--out FILE]
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


def lost_shards(pattern, k, m, s):
    """the shards stripe s has lost, originals [0, k), recovery [k, k + m)"""
    if pattern == "rotate":
        return [s % (k + m)]
    if pattern == "parity":
        return [k + s % m]
    if pattern == "2+2":
        return [s % k, (s + 3) % k, k + s % m, k + (s + 1) % m]
    if pattern.startswith("mixed"):
        return sorted({(s * 7 + 29 * i) % (k + m) for i in range(int(pattern[5:]))})
    raise ValueError(pattern)


def bench_case(k, m, sb, n, pattern, sets, min_window, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(2025)
    truth = torch.randint(0, 256, (n, k, sb), dtype=torch.uint8, device=dev, generator=g)
    parity_true = torch.empty((n, m, sb), dtype=torch.uint8, device=dev)
    R.encode_batch_dev(k, m, truth, parity_true)
    lost = [lost_shards(pattern, k, m, s) for s in range(n)]
    max_e = max(len(x) for x in lost)
    max_eo = max(sum(1 for i in x if i < k) for x in lost)
    assert 0 < max_e <= m
    present = torch.ones((n, k + m), dtype=torch.uint8)
    # (stripe, shard, slot) of every lost original / recovery shard; a stripe's slots: originals first
    so, jo, sloto, sr, jr, slotr = [], [], [], [], [], []
    for s, x in enumerate(lost):
        present[s, x] = 0
        for slot, i in enumerate(sorted(x)):
            if i < k:
                so.append(s), jo.append(i), sloto.append(slot)
            else:
                sr.append(s), jr.append(i - k), slotr.append(slot)
    present = present.to(dev)
    so, jo, sloto, sr, jr, slotr = (torch.tensor(v, dtype=torch.long, device=dev) for v in (so, jo, sloto, sr, jr, slotr))
    data, parity = truth.clone(), parity_true.clone()
    data[so, jo] = 0  # what is lost is gone
    parity[sr, jr] = 0
    want = torch.zeros((n, max_e, sb), dtype=torch.uint8, device=dev)
    want[so, sloto] = truth[so, jo]
    want[sr, slotr] = parity_true[sr, jr]
    del truth, parity_true

    rebuilt = torch.zeros((n, max_e, sb), dtype=torch.uint8, device=dev)
    status = torch.empty((n,), dtype=torch.int32, device=dev)
    restored = torch.zeros((n, max(max_eo, 1), sb), dtype=torch.uint8, device=dev)
    full = torch.empty((n, m, sb), dtype=torch.uint8, device=dev)  # the composed route's m-row parity buffer
    picked = torch.zeros((n, max_e, sb), dtype=torch.uint8, device=dev)

    def leg_rebuild():
        R.rebuild_batch_dev(k, m, present, data, parity, rebuilt, status=status)

    def leg_composed():
        if max_eo:
            R.reconstruct_batch_dev_patterns(k, m, present, data, parity, restored[:, :max_eo], status=status)
            data[so, jo] = restored[so, sloto]  # the restored originals into their places
            picked[so, sloto] = restored[so, sloto]
        R.encode_batch_dev(k, m, data, full)
        picked[sr, slotr] = full[sr, jr]  # the rows that were lost

    def leg_composed_kernels():
        if max_eo:
            R.reconstruct_batch_dev_patterns(k, m, present, data, parity, restored[:, :max_eo], status=status)
        R.encode_batch_dev(k, m, data, full)

    kernels = {}
    for _ in range(2):  # the second call runs the steady-state kernels
        leg_rebuild()
        R.net_wait()
    kernels["rebuild"] = R.last_kernels()
    torch.cuda.synchronize()
    assert torch.equal(rebuilt, want) and not status.any().item(), "rebuild"
    leg_composed()
    R.net_wait()
    leg_composed()
    torch.cuda.synchronize()
    assert torch.equal(picked, want), "composed"
    del want

    legs = {"rebuild": leg_rebuild, "composed": leg_composed, "composed_kernels": leg_composed_kernels}
    reps = {}
    for name, fn in legs.items():  # warm, and size the windows
        fn()
        reps[name] = max(2, math.ceil(min_window / (window(fn, 2) / 1e3)))
    times = {name: [] for name in legs}
    for _ in range(sets):
        for name, fn in legs.items():
            times[name].append(window(fn, reps[name]))
    e_o, e_r = so.numel() / n, sr.numel() / n
    res = {"shape": {"k": k, "m": m, "shard_bytes": sb, "stripes": n}, "pattern": pattern,
           "lost_per_stripe": {"originals": round(e_o, 3), "recovery": round(e_r, 3)}, "max_e": max_e,
           "rebuild_kernel_name": R.rebuild_kernel_name(k, m, sb, max_e), "rebuild_kernels": kernels["rebuild"],
           "sets": sets, "window_s": min_window, "legs": {}}
    for name, t in times.items():
        res["legs"][name] = {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4),
                             "max_ms": round(max(t), 4), "calls_per_window": reps[name]}
    res["composed_over_rebuild"] = round(res["legs"]["composed"]["median_ms"] / res["legs"]["rebuild"]["median_ms"], 4)
    res["composed_kernels_over_rebuild"] = round(
        res["legs"]["composed_kernels"]["median_ms"] / res["legs"]["rebuild"]["median_ms"], 4)
    res["rebuild_range_below_composed"] = res["legs"]["rebuild"]["max_ms"] < res["legs"]["composed"]["min_ms"]
    res["rows_per_stripe_fast_form"] = round(k + e_o + e_r, 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="10,4,1048576,1024,rotate;10,4,1048576,1024,parity;10,4,1048576,1024,2+2;"
                                       "200,55,262144,512,mixed8", help="K,M,SHARD_BYTES,STRIPES,PATTERN;...")
    ap.add_argument("--sets", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="least seconds per timed window")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "rebuild_bench needs a GPU"
    dev = torch.device("cuda:0")
    for case in args.cases.split(";"):
        k, m, sb, n, pattern = case.split(",")
        line = json.dumps(bench_case(int(k), int(m), int(sb), int(n), pattern, args.sets, args.window, dev))
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
