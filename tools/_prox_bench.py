"""What tools/tgv_bench.py, ndf_bench.py, diff4th_bench.py and llt_rof_bench.py share: the command line, the synthetic
input, the timing and the JSON lines.  Each of the four scripts states its own options, parameters and run list.

Per shape: the script reserves the placed scratch arena first, every operator is warmed up, then `reps` pairs of calls with
`short` and `long` iterations are timed with device events; the time of one iteration is the median over the pairs of
(t_long - t_short) / (long - short), which leaves the set-up of a call out.  One JSON line per shape and operator: ms per
iteration, the algorithmic traffic per iteration, the rate it amounts to and its ratio to the plain-copy rate measured on
this hardware (6.2 TB/s, profiles/archive/r4b_hbm_copy_probe.txt)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_RATE_GBPS = 6200.0
BYTES_PER_VOXEL = 12                   # ROF_TV, NDF, Diff4th, LLT_ROF: U and f read, U' written
TGV_BYTES_PER_VOXEL = {3: 176, 2: 112}


def algorithmic_bytes(shape, per_voxel=BYTES_PER_VOXEL):
    n = 1
    for v in shape:
        n *= v
    return n * per_voxel


def main(tool, runs_of, argv=None, options=(), ratios_of=None):
    """``options``: (flag, help) switches of the script beside the shared ones.  ``runs_of(args, shape, x, out)`` reserves
    the arenas and returns (runs, extra): runs = [(op, bytes per voxel, call(iterations))], extra = further fields of every
    line of the shape.  ``ratios_of``: the ops the first run's time is given as a ratio to, on its line in `--out` and on a
    line "<first op>_ratios" of its own."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="512x512x512,1024x1024x1024,4096x4096")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--short", type=int, default=4)
    ap.add_argument("--long", type=int, default=14)
    for flag, text in options:
        ap.add_argument(flag, action="store_true", help=text)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args(argv)
    if not 0 < args.short < args.long or args.reps < 1:
        ap.error("need 0 < --short < --long and --reps >= 1")
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    for s in shapes:
        if len(s) not in (2, 3) or min(s) < 1:
            ap.error(f"bad shape {s}")

    import torch
    from tomobar_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit(f"{tool} needs a GPU (there is no CPU path)")
    lines = []
    for shape in shapes:
        gen = torch.Generator(device="cuda").manual_seed(3)
        # a noisy ramp scaled like the tests' phantom: differences and gradients on both sides of the scripts' thresholds
        x = torch.rand(shape, device="cuda", generator=gen) * 4.0
        x += torch.arange(shape[-1], device="cuda", dtype=torch.float32) * 1.2
        out = torch.empty_like(x)
        runs, extra = runs_of(args, shape, x, out)
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
                    "ratio_to_copy_rate_6200_GBps": round(rate / COPY_RATE_GBPS, 3), **extra,
                    "finite": bool(torch.isfinite(out).all()), "placement": ops.placement_last()}
            print(json.dumps(line), flush=True)
            lines.append(line)
        if ratios_of:
            ms_of = {ln["op"]: ln["ms_per_iteration"] for ln in lines[first:]}
            mine = runs[0][0]
            for other in ratios_of:
                if other in ms_of:
                    lines[first][f"time_ratio_to_{other}"] = round(ms_of[mine] / ms_of[other], 3)
            if len(ms_of) > 1:
                print(json.dumps({"op": f"{mine}_ratios", "shape": list(shape),
                                  **{k: v for k, v in lines[first].items() if k.startswith("time_ratio_to_")}}), flush=True)
        del x, out
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")
