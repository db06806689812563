"""Timing of the wavelet shrinkage (tomo_wavelet_shrink: six launches per call, docs/kernels/wavelets.md) on synthetic data,
beside the copy rate measured in the same process on the same arrays, and of PD_TV_WAVELETS against PD_TV through
prox_regul at the headline's 30 inner iterations.

usage: python tools/wavelet_bench.py [--shapes 1024x1024x1024,256x2048x2048] [--reps 7] [--calls 4] [--inner 30] [--out FILE]

Per shape: the scratch arena is reserved first and everything is warmed up; a timed window is `calls` back-to-back calls
between two device events (a window of a single call at these sizes is a few milliseconds), `reps` windows per operation,
taken in turns (copy, shrink, shrink with mix, PD_TV, PD_TV_WAVELETS, and round again) so that a drift of the machine hits all of them
alike; the figure is the median window over `calls`.  Prints one JSON line per shape and operation: ms per call with its
spread, the algorithmic traffic (copy: 8 B per voxel; shrinkage: 21 B per voxel, 25 B with `mix` -- forward 10.5, inverse
10.5 / 14.5, docs/kernels/wavelets.md), the rate that amounts to and its ratio to the copy rate of this run.  Kernel times:
run the same command under `rocprofv3 --kernel-trace --stats` in a run of its own."""
import argparse
import json
import os
import statistics
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BYTES = {"copy": 8.0, "wavelet_shrink": 21.0, "wavelet_shrink_mix": 25.0}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1024x1024x1024,256x2048x2048")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--inner", type=int, default=30, help="inner iterations of the PD_TV comparison")
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--no-prox", action="store_true", help="skip the PD_TV / PD_TV_WAVELETS comparison")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args(argv)
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    if args.reps < 1 or args.calls < 1 or any(len(s) not in (2, 3) or min(s) < 1 for s in shapes):
        ap.error("bad --reps, --calls or --shapes")

    import numpy as np
    import torch
    from tomobar_amd import ops
    from tomobar_amd.regularisersCuPy import prox_regul, reserve_prox_scratch
    if not torch.cuda.is_available():
        raise SystemExit("wavelet_bench needs a GPU (there is no CPU path)")
    me = types.SimpleNamespace(nonneg_regul=0, Atools=types.SimpleNamespace(device_index=0), slab=None)
    t = np.float32(args.threshold)
    lines = []
    for shape in shapes:
        gen = torch.Generator(device="cuda").manual_seed(3)
        x = torch.rand(shape, device="cuda", generator=gen) * 4.0
        x += torch.arange(shape[-1], device="cuda", dtype=torch.float32) * 1.2
        out, mix = torch.empty_like(x), torch.rand(shape, device="cuda", generator=gen)
        reg = {"method": "PD_TV", "regul_param": 0.05, "iterations": args.inner, "methodTV": 0, "PD_LipschitzConstant": 8.0,
               "regul_param2": float(t)}
        reg_w = dict(reg, method="PD_TV_WAVELETS")
        ops_of = {"copy": lambda: out.copy_(x),
                  "wavelet_shrink": lambda: ops.wavelet_shrink(x, t, out=out),
                  "wavelet_shrink_mix": lambda: ops.wavelet_shrink(x, t, out=out, mix=mix)}
        if not args.no_prox:
            reserve_prox_scratch(me, shape, reg_w)
            ops_of["PD_TV"] = lambda: prox_regul(me, x, reg, out=out)
            ops_of["PD_TV_WAVELETS"] = lambda: prox_regul(me, x, reg_w, out=out)
        else:
            ops.reserve_wavelet_scratch(shape, "cuda:0")

        def window(call):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                call()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / args.calls

        for call in ops_of.values():
            window(call)
        times = {name: [] for name in ops_of}
        for _ in range(args.reps):
            for name, call in ops_of.items():
                times[name].append(window(call))
        nvox = int(np.prod(shape))
        copy_rate = nvox * BYTES["copy"] / (statistics.median(times["copy"]) * 1e-3) / 1e9
        for name, ts in times.items():
            ms = statistics.median(ts)
            line = {"op": name, "shape": list(shape), "ms_per_call": round(ms, 4), "ms_per_call_min_max": [round(min(ts), 4), round(max(ts), 4)],
                    "windows": args.reps, "calls_per_window": args.calls}
            if name in BYTES:
                rate = nvox * BYTES[name] / (ms * 1e-3) / 1e9
                line.update(algorithmic_bytes_per_voxel=BYTES[name], algorithmic_GBps=round(rate, 1),
                            copy_GBps_this_run=round(copy_rate, 1), ratio_to_copy_rate_this_run=round(rate / copy_rate, 3))
            else:
                line.update(inner_iterations=args.inner, threshold=float(t))
            if name == "PD_TV_WAVELETS":
                line.update(time_ratio_to_PD_TV=round(ms / statistics.median(times["PD_TV"]), 4),
                            ms_more_than_PD_TV=round(ms - statistics.median(times["PD_TV"]), 4))
            line.update(finite=bool(torch.isfinite(out).all()), placement=ops.placement_last())
            print(json.dumps(line), flush=True)
            lines.append(line)
        del x, out, mix
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
