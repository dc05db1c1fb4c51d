#!/usr/bin/env python3
"""Update (the small write) against what a caller had to do before it, device-resident, per shape:
  (a) encode        rs_encode_batch_dev of the whole stripe into the parity buffer: k + m rows
  (b) update_u1     rs_update_batch_dev, one changed original per stripe, old + new: 2 + 2m rows
  (c) update_u1_delta  the same in delta form (d_old == NULL): 1 + 2m rows
  (d) update_u4     four changed originals per stripe, old + new: 8 + 2m rows
  (e) update_u2     two changed originals per stripe, old + new: 4 + 2m rows (where the crossover
                    with the encode lies on a narrow code)
Before anything is timed, (b), (c), (d) and (e) applied to a copy of the old parity must equal (a) on
the new data, byte for byte. The legs alternate in one process; each timed window is warmed, ends
in a device synchronise and lasts at least --window seconds. The set is repeated --sets times; per
leg the median and the min-max range of the per-call times are printed as one JSON line per shape,
next to the leg's traffic ratio over the encode.

    python tools/update_bench.py [--shapes K,M,SHARD_BYTES,STRIPES;...] [--out FILE]
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
    assert k >= 8, "the u = 4 leg changes originals s, s + 3, s + 5, s + 7 (mod k)"
    g = torch.Generator(device=dev)
    g.manual_seed(2025)
    data = torch.randint(0, 256, (n, k, sb), dtype=torch.uint8, device=dev, generator=g)
    parity_old = torch.empty((n, m, sb), dtype=torch.uint8, device=dev)
    parity = torch.empty_like(parity_old)
    R.encode_batch_dev(k, m, data, parity_old)

    rows = torch.arange(n, device=dev)
    idx4 = torch.stack([(rows + d) % k for d in (0, 3, 5, 7)], dim=1).to(torch.int32).contiguous()
    idx1 = idx4[:, :1].contiguous()
    old4 = torch.stack([data[rows, idx4[:, i].long()] for i in range(4)], dim=1).contiguous()
    new4 = torch.randint(0, 256, (n, 4, sb), dtype=torch.uint8, device=dev, generator=g)
    old1, new1 = old4[:, :1].contiguous(), new4[:, :1].contiguous()
    idx2, old2, new2 = idx4[:, :2].contiguous(), old4[:, :2].contiguous(), new4[:, :2].contiguous()
    delta1 = old1 ^ new1
    status = torch.empty((n,), dtype=torch.int32, device=dev)

    def leg_a():
        R.encode_batch_dev(k, m, data, parity)

    def leg_b(p=parity):
        R.update_batch_dev(k, m, idx1, new1, p, old=old1, status=status)

    def leg_c(p=parity):
        R.update_batch_dev(k, m, idx1, delta1, p, status=status)

    def leg_d(p=parity):
        R.update_batch_dev(k, m, idx4, new4, p, old=old4, status=status)

    def leg_e(p=parity):
        R.update_batch_dev(k, m, idx2, new2, p, old=old2, status=status)

    # the legs agree before anything is timed: the update of the old parity is the encode of the new data
    kernels = {}
    work = torch.empty_like(parity_old)
    data[rows, idx4[:, 0].long()] = new4[:, 0]
    leg_a()
    for name, leg in (("update_u1", leg_b), ("update_u1_delta", leg_c)):
        work.copy_(parity_old)
        leg(work)
        kernels[name] = R.last_kernels()
        assert torch.equal(work, parity) and not status.any().item(), name
    for u, name, leg in ((2, "update_u2", leg_e), (4, "update_u4", leg_d)):
        for i in range(1, u):
            data[rows, idx4[:, i].long()] = new4[:, i]
        leg_a()
        work.copy_(parity_old)
        leg(work)
        kernels[name] = R.last_kernels()
        assert torch.equal(work, parity) and not status.any().item(), name
    del work, parity_old

    legs = {"encode": leg_a, "update_u1": leg_b, "update_u1_delta": leg_c, "update_u4": leg_d, "update_u2": leg_e}
    reps = {}
    for name, fn in legs.items():  # warm, and size the windows
        fn()
        reps[name] = max(2, math.ceil(min_window / (window(fn, 2) / 1e3)))
    times = {name: [] for name in legs}
    for _ in range(sets):
        for name, fn in legs.items():
            times[name].append(window(fn, reps[name]))
    traffic = {"encode": 1.0, "update_u1": (2 + 2 * m) / (k + m), "update_u1_delta": (1 + 2 * m) / (k + m),
               "update_u4": (8 + 2 * m) / (k + m), "update_u2": (4 + 2 * m) / (k + m)}
    res = {"shape": {"k": k, "m": m, "shard_bytes": sb, "stripes": n},
           "encode_kernel_name": R.encode_kernel_name(k, m, sb), "update_kernels": kernels, "sets": sets,
           "window_s": min_window, "legs": {}}
    enc = statistics.median(times["encode"])
    for name, t in times.items():
        res["legs"][name] = {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4),
                             "max_ms": round(max(t), 4), "calls_per_window": reps[name],
                             "over_encode": round(statistics.median(t) / enc, 4),
                             "traffic_over_encode": round(traffic[name], 4)}
    for name in ("update_u1", "update_u1_delta", "update_u4", "update_u2"):  # the whole range below the encode's
        res[name + "_range_below_encode"] = res["legs"][name]["max_ms"] < res["legs"]["encode"]["min_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="200,55,262144,512;10,4,1048576,1024", help="K,M,SHARD_BYTES,STRIPES;...")
    ap.add_argument("--sets", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="least seconds per timed window")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "update_bench needs a GPU"
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
