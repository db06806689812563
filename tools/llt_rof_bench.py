"""Timing of the LLT_ROF regulariser (tomo_llt_rof: one launch per iteration, both stages fused, docs/kernels/llt_rof.md) on
synthetic data, with Diff4th, NDF (Huber) and ROF_TV -- the same algorithmic traffic, 12 B per voxel -- timed beside it on
the same arrays in the same process.

usage: python tools/llt_rof_bench.py [--shapes 512x512x512,1024x1024x1024,4096x4096] [--reps 5] [--short 4] [--long 14] [--out FILE]

Per shape: the placed scratch arena is reserved first, every operator is warmed up, then `reps` pairs of calls with `short`
and `long` iterations are timed with device events; the time of one iteration is the median over the pairs of
(t_long - t_short) / (long - short), which leaves the set-up of a call out.  Prints one JSON line per shape and operator:
ms per iteration, the algorithmic traffic per iteration, the rate it amounts to and its ratio to the plain-copy rate
measured on this hardware (6.2 TB/s, profiles/archive/r4b_hbm_copy_probe.txt); the LLT_ROF line also carries its time as a
ratio to the siblings'.  `--out profiles/llt_rof_bench.jsonl` keeps the lines.  Kernel times: run the same command under
`rocprofv3 --kernel-trace --stats` in a run of its own."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_RATE_GBPS = 6200.0
BYTES_PER_VOXEL = 12                   # all four operators: U and f read, U' written


def algorithmic_bytes(shape, per_voxel=BYTES_PER_VOXEL):
    n = 1
    for v in shape:
        n *= v
    return n * per_voxel


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="512x512x512,1024x1024x1024,4096x4096")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--short", type=int, default=4)
    ap.add_argument("--long", type=int, default=14)
    ap.add_argument("--no-siblings", action="store_true", help="skip Diff4th, NDF and ROF_TV")
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
        raise SystemExit("llt_rof_bench needs a GPU (there is no CPU path)")
    lam_rof, lam_llt, tau = np.float32(0.3), np.float32(0.1), np.float32(0.02)   # set A of tests/_llt_rof_oracle.py
    # the siblings' parameters are those of tools/diff4th_bench.py
    lam, sigma, d4_tau = np.float32(1.0), np.float32(2.0), np.float32(0.005)
    lines = []
    for shape in shapes:
        gen = torch.Generator(device="cuda").manual_seed(3)
        # a noisy ramp scaled like the tests' phantom (the input of tools/diff4th_bench.py)
        x = torch.rand(shape, device="cuda", generator=gen) * 4.0
        x += torch.arange(shape[-1], device="cuda", dtype=torch.float32) * 1.2
        out = torch.empty_like(x)
        if not args.no_siblings:
            ops.reserve_tv_scratch(shape, "cuda:0", "ROF_TV")   # the largest of the four arenas: nothing is re-placed in between
        ops.reserve_tv_scratch(shape, "cuda:0", "LLT_ROF")

        runs = [("llt_rof", BYTES_PER_VOXEL, lambda n: ops.llt_rof(x, out, lam_rof, lam_llt, tau, n))]
        if not args.no_siblings:
            runs.append(("diff4th", BYTES_PER_VOXEL, lambda n: ops.diff4th(x, out, lam, sigma, d4_tau, n)))
            runs.append(("ndf_Huber", BYTES_PER_VOXEL, lambda n: ops.ndf(x, out, lam, sigma, np.float32(0.05), "Huber", n)))
            runs.append(("rof_tv", BYTES_PER_VOXEL, lambda n: ops.roftv(x, out, np.float32(0.05), np.float32(0.005), n, False)))
        first = len(lines)
        for name, per_voxel, call in runs:
            def run(iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call(iters)
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
            nbytes = algorithmic_bytes(shape, per_voxel)
            rate = nbytes / (ms * 1e-3) / 1e9
            line = {"op": name, "shape": list(shape), "ms_per_iteration": round(ms, 4),
                    "ms_per_iteration_min_max": [round(min(per_iter), 4), round(max(per_iter), 4)],
                    f"ms_per_call_{args.long}_iterations": round(statistics.median(calls), 3),
                    "algorithmic_bytes_per_iteration": nbytes, "algorithmic_GBps": round(rate, 1),
                    "ratio_to_copy_rate_6200_GBps": round(rate / COPY_RATE_GBPS, 3),
                    "finite": bool(torch.isfinite(out).all()), "placement": ops.placement_last()}
            print(json.dumps(line), flush=True)
            lines.append(line)
        ms_of = {ln["op"]: ln["ms_per_iteration"] for ln in lines[first:]}
        for other in ("diff4th", "ndf_Huber", "rof_tv"):
            if other in ms_of:
                lines[first][f"time_ratio_to_{other}"] = round(ms_of["llt_rof"] / ms_of[other], 3)
        if len(ms_of) > 1:
            print(json.dumps({"op": "llt_rof_ratios", "shape": list(shape),
                              **{k: v for k, v in lines[first].items() if k.startswith("time_ratio_to_")}}), flush=True)
        del x, out
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
