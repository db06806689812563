"""Timing of the TGV prox (tomo_tgv: two launches per iteration, docs/kernels/tgv.md) on synthetic data.

usage: python tools/tgv_bench.py [--shapes 512x512x512,1024x1024x1024,4096x4096] [--reps 5] [--short 4] [--long 14] [--out FILE]

Per shape: the placed scratch arena is reserved first, every shape is warmed up, then `reps` pairs of calls with `short`
and `long` iterations are timed with device events; the time of one iteration is the median over the pairs of
(t_long - t_short) / (long - short), which leaves the set-up of a call (two copies and one fill of the arena) out.
Prints one JSON line per shape: ms per iteration, the algorithmic traffic (44 floats = 176 B per voxel and iteration in
3D, 28 floats = 112 B in 2D), the rate it amounts to and its ratio to the plain-copy rate measured on this hardware
(6.2 TB/s, profiles/archive/r4b_hbm_copy_probe.txt).  Kernel times: run the same command under
`rocprofv3 --kernel-trace --stats` in a run of its own."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_RATE_GBPS = 6200.0
BYTES_PER_VOXEL = {3: 176, 2: 112}


def algorithmic_bytes(shape):
    n = 1
    for v in shape:
        n *= v
    return n * BYTES_PER_VOXEL[len(shape)]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="512x512x512,1024x1024x1024,4096x4096")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--short", type=int, default=4)
    ap.add_argument("--long", type=int, default=14)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args(argv)
    if not 0 < args.short < args.long or args.reps < 1:
        ap.error("need 0 < --short < --long and --reps >= 1")
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    for s in shapes:
        if len(s) not in (2, 3) or min(s) < 1:
            ap.error(f"bad shape {s}")

    import numpy as np
    import torch
    from tomobar_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("tgv_bench needs a GPU (there is no CPU path)")
    tau = np.float32(np.float32(1.0) / np.sqrt(np.float32(12.0)))
    lines = []
    for shape in shapes:
        gen = torch.Generator(device="cuda").manual_seed(3)
        # a noisy ramp scaled like the tests' phantom: both projections are active on part of the voxels
        x = torch.rand(shape, device="cuda", generator=gen) * 4.0
        x += torch.arange(shape[-1], device="cuda", dtype=torch.float32) * 1.2
        out = torch.empty_like(x)
        ops.reserve_tv_scratch(shape, "cuda:0", "TGV")

        def run(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.tgv(x, out, 5.0, 1.0, 2.0, tau, tau, iters)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        run(args.short)   # warm-up: code objects, the arena
        per_iter, calls = [], []
        for _ in range(args.reps):
            ts, tl = run(args.short), run(args.long)
            per_iter.append((tl - ts) / (args.long - args.short))
            calls.append(tl)
        ms = statistics.median(per_iter)
        nbytes = algorithmic_bytes(shape)
        rate = nbytes / (ms * 1e-3) / 1e9
        line = {"op": "tgv", "shape": list(shape), "ms_per_iteration": round(ms, 4),
                "ms_per_iteration_min_max": [round(min(per_iter), 4), round(max(per_iter), 4)],
                f"ms_per_call_{args.long}_iterations": round(statistics.median(calls), 3),
                "algorithmic_bytes_per_iteration": nbytes, "algorithmic_GBps": round(rate, 1),
                "ratio_to_copy_rate_6200_GBps": round(rate / COPY_RATE_GBPS, 3),
                "finite": bool(torch.isfinite(out).all()), "placement": ops.placement_last()}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del x, out
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
