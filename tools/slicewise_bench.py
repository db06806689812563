"""Timing of the slice-wise PD_TV / ROF_TV (tomo_pdtv_slices / tomo_roftv_slices, docs/kernels/slicewise.md) on synthetic
data: for every shape and operator the batched call, the loop of today's 2D function over the slices (what a user had to
write before) and today's 3D call on the same array (coupled along z: another result, the same amount of data).

usage: python tools/slicewise_bench.py [--shapes 256x1024x1024,1024x1024x1024] [--iterations 30] [--reps 5] [--out FILE]

One process.  Per shape the TV scratch arena is reserved for its largest user first (so no placement search falls into a
timed window) and every call is warmed up; a timed window is ONE call between two device events (the shortest, the 3D
call at 256 x 1024^2, is tens of milliseconds), `reps` windows per call, taken in turns (batched, loop, 3D, and round again)
so that a drift of the machine hits all three alike; the figure is the median window.  Prints -- and with --out appends
to FILE -- one JSON line per shape and operator: the three medians with their spread, the ratios, and the algorithmic
traffic of the batched form (PD_TV: 28 B per pixel and pass with float32 duals, 20 B with binary16 duals, less the duals
the first pass does not read and the last does not write; ROF_TV: 12 B per pixel and iteration) with the rate that amounts
to.  Kernel times: run the same command under `rocprofv3 --kernel-trace --stats` in a run of its own."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

OPERATORS = ("PD_TV", "PD_TV_f16", "ROF_TV")


def pd_passes(iterations):
    """launches of a PD_TV run of `iterations` (three per pass, 4 = 2 + 2)"""
    n, left = 0, iterations
    while left > 0:
        left -= 3 if (left >= 3 and left != 4) else 2 if left >= 2 else 1
        n += 1
    return n


def algorithmic_bytes_per_pixel(op, iterations):
    if op == "ROF_TV":
        return 12.0 * iterations
    dual = 4.0 if op == "PD_TV" else 2.0
    passes = pd_passes(iterations)
    # every pass reads U and the input and writes U; all but the first read two duals, all but the last write two
    return 12.0 * passes + 2 * dual * (passes - 1) * 2


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x1024x1024,1024x1024x1024")
    ap.add_argument("--operators", default=",".join(OPERATORS))
    ap.add_argument("--iterations", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args(argv)
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    operators = args.operators.split(",")
    if args.reps < 1 or args.iterations < 1 or any(len(s) != 3 or min(s) < 2 for s in shapes) or set(operators) - set(OPERATORS):
        ap.error("bad --reps, --iterations, --operators or --shapes")

    import numpy as np
    import torch
    from tomobar_amd import ops
    from tomobar_amd.regularisersCuPy import PD_TV_cupy, ROF_TV_cupy
    if not torch.cuda.is_available():
        raise SystemExit("slicewise_bench needs a GPU (there is no CPU path)")

    def window(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for shape in shapes:
        nz = shape[0]
        gen = torch.Generator(device="cuda").manual_seed(3)
        x = torch.rand(shape, device="cuda", generator=gen) * 0.2
        x += torch.linspace(0.0, 1.0, nz, device="cuda").view(nz, 1, 1)
        out = torch.empty_like(x)
        ops.reserve_tv_scratch(shape, "cuda:0", "PD_TV", False)   # the largest: two U and six dual arrays
        for op in operators:
            half = op == "PD_TV_f16"
            if op == "ROF_TV":
                def fn(a, o, slicewise=False):
                    return ROF_TV_cupy(a, 0.05, args.iterations, 0.005, 0, False, out=o, slicewise=slicewise)
            else:
                def fn(a, o, slicewise=False, half=half):
                    return PD_TV_cupy(a, 0.05, args.iterations, 0, 0, 8.0, 0, half, out=o, slicewise=slicewise)

            def loop(fn=fn):
                for k in range(nz):
                    fn(x[k], out[k])

            calls = {"batched": lambda fn=fn: fn(x, out, slicewise=True), "loop_2d": loop, "coupled_3d": lambda fn=fn: fn(x, out)}
            for call in calls.values():
                window(call)
            times = {name: [] for name in calls}
            for _ in range(args.reps):
                for name, call in calls.items():
                    times[name].append(window(call))
            # the batched call and the loop compute the same thing
            calls["batched"]()
            got = out.clone()
            calls["loop_2d"]()
            same = bool(torch.equal(got, out))
            med = {name: statistics.median(ts) for name, ts in times.items()}
            bpp = algorithmic_bytes_per_pixel(op, args.iterations)
            line = {"op": op, "shape": list(shape), "iterations": args.iterations, "windows": args.reps,
                    "ms": {name: round(med[name], 3) for name in calls},
                    "ms_min_max": {name: [round(min(ts), 3), round(max(ts), 3)] for name, ts in times.items()},
                    "loop_over_batched": round(med["loop_2d"] / med["batched"], 3),
                    "batched_over_coupled_3d": round(med["batched"] / med["coupled_3d"], 3),
                    "batched_algorithmic_bytes_per_pixel": bpp,
                    "batched_algorithmic_GBps": round(float(np.prod(shape)) * bpp / (med["batched"] * 1e-3) / 1e9, 1),
                    "batched_equals_loop": same, "finite": bool(torch.isfinite(out).all()), "placement": ops.placement_last()}
            print(json.dumps(line), flush=True)
            if args.out:
                with open(args.out, "a") as fh:
                    fh.write(json.dumps(line) + "\n")
        del x, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
