"""Timing of non-local TV (docs/kernels/nltv.md) on synthetic data: tomo_patch_select (one launch per call) and one
iteration of tomo_nltv (one launch per iteration), with one iteration of ROF_TV timed beside it on the same array.

usage: python tools/nltv_bench.py [--shapes 512x512x512,64x1024x1024,4096x4096] [--search 7] [--patch 2] [--neighbours 15]
                                  [--reps 5] [--short 4] [--long 14] [--no-rof] [--out profiles/nltv_bench.jsonl]

Per shape: the tables are built once (that call is the warm-up of patch_select), then `reps` calls of patch_select are timed
with device events, the figure is the median.  The iterations are timed as tools/_prox_bench.py times them: `reps` pairs of
calls with `short` and `long` iterations, the time of one iteration is the median of (t_long - t_short) / (long - short),
which leaves the set-up of a call out.  One JSON line per shape and operation.  patch_select is compute-bound: its line gives
the pixel-candidate pairs per second ((2 search + 1)^2 - 1 candidates per pixel).  The iteration is traffic-bound: its line
gives the algorithmic traffic (8 * neighbours + 12 B per voxel: the three tables, U and f read, U' written; the gather of
the neighbours is served by the cache and not counted), the rate it amounts to and its ratio to the plain-copy rate measured
on this hardware (6.2 TB/s, profiles/archive/r4b_hbm_copy_probe.txt).  The tables take 8 * neighbours bytes per voxel of
device memory (129 GB at 1024^3 with 15 neighbours), which is what bounds the 3D shapes this script can hold.  Kernel times:
run the same command under `rocprofv3 --kernel-trace --stats` in a run of its own."""
import argparse
import json
import statistics

import _prox_bench as B


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="512x512x512,64x1024x1024,4096x4096")
    ap.add_argument("--search", type=int, default=7)
    ap.add_argument("--patch", type=int, default=2)
    ap.add_argument("--neighbours", type=int, default=15)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--short", type=int, default=4)
    ap.add_argument("--long", type=int, default=14)
    ap.add_argument("--no-rof", action="store_true", help="skip the ROF_TV comparison")
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
        raise SystemExit("nltv_bench needs a GPU (there is no CPU path)")
    S, P, K = args.search, args.patch, args.neighbours
    h, lam = np.float32(2.0), np.float32(0.5)
    lines = []

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for shape in shapes:
        gen = torch.Generator(device="cuda").manual_seed(3)
        # the noisy ramp of tools/_prox_bench.py
        x = torch.rand(shape, device="cuda", generator=gen) * 4.0
        x += torch.arange(shape[-1], device="cuda", dtype=torch.float32) * 1.2
        out = torch.empty_like(x)
        nvox = int(np.prod(shape))
        common = {"shape": list(shape), "search": S, "patch": P, "neighbours": K, "table_bytes": 8 * K * nvox}
        ops.reserve_tv_scratch(shape, "cuda:0", "ROF_TV")   # the larger of the two arenas: nothing is re-placed in between
        ops.reserve_nltv_scratch(shape, "cuda:0")

        tables = ops.patch_select(x, S, P, K, h)
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            ts.append(timed(lambda: ops.patch_select(x, S, P, K, h)))
            torch.cuda.synchronize()
        ms = statistics.median(ts)
        pairs = nvox * ((2 * S + 1) ** 2 - 1)
        line = {"op": "patch_select", **common, "ms_per_call": round(ms, 3), "ms_per_call_min_max": [round(min(ts), 3), round(max(ts), 3)],
                "calls": args.reps, "pixel_candidate_pairs": pairs, "Gpairs_per_s": round(pairs / (ms * 1e-3) / 1e9, 2),
                "ns_per_voxel": round(ms * 1e6 / nvox, 3), "weights_finite": bool(torch.isfinite(tables[2]).all())}
        print(json.dumps(line), flush=True)
        lines.append(line)

        runs = [("nltv", 8 * K + 12, lambda n: ops.nltv(x, out, *tables, lam, n))]
        if not args.no_rof:
            runs.append(("roftv", B.BYTES_PER_VOXEL, lambda n: ops.roftv(x, out, np.float32(0.05), np.float32(0.005), n, False)))
        first = len(lines)
        for name, per_voxel, call in runs:
            timed(lambda: call(args.short))   # warm-up: code objects, the arena
            per_iter, calls = [], []
            for _ in range(args.reps):
                t_short, t_long = timed(lambda: call(args.short)), timed(lambda: call(args.long))
                per_iter.append((t_long - t_short) / (args.long - args.short))
                calls.append(t_long)
            ms = statistics.median(per_iter)
            nbytes = B.algorithmic_bytes(shape, per_voxel)
            rate = nbytes / (ms * 1e-3) / 1e9
            line = {"op": name, **common, "ms_per_iteration": round(ms, 4),
                    "ms_per_iteration_min_max": [round(min(per_iter), 4), round(max(per_iter), 4)],
                    f"ms_per_call_{args.long}_iterations": round(statistics.median(calls), 3),
                    "algorithmic_bytes_per_voxel": per_voxel, "algorithmic_bytes_per_iteration": nbytes,
                    "algorithmic_GBps": round(rate, 1), "ratio_to_copy_rate_6200_GBps": round(rate / B.COPY_RATE_GBPS, 3),
                    "finite": bool(torch.isfinite(out).all()), "placement": ops.placement_last()}
            print(json.dumps(line), flush=True)
            lines.append(line)
        ms_of = {ln["op"]: ln["ms_per_iteration"] for ln in lines[first:]}
        if "roftv" in ms_of:
            lines[first]["time_ratio_to_roftv"] = round(ms_of["nltv"] / ms_of["roftv"], 3)
            print(json.dumps({"op": "nltv_ratios", "shape": list(shape),
                              **{k: v for k, v in lines[first].items() if k.startswith("time_ratio_to_")}}), flush=True)
        del x, out, tables
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
