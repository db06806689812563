"""Timing of the Diff4th regulariser (tomo_diff4th: one launch per iteration, both stages fused, docs/kernels/diff4th.md) on
synthetic data, with NDF -- the same algorithmic traffic, 12 B per voxel -- and TGV -- the operator Diff4th is the cheap
alternative to, 176 B per voxel (2D: 112) -- timed beside it on the same arrays.

usage: python tools/diff4th_bench.py [--shapes 512x512x512,1024x1024x1024,4096x4096] [--reps 5] [--short 4] [--long 14] [--out FILE]

Per shape: the placed scratch arena is reserved first (TGV's, the largest), every operator is warmed up, then `reps` pairs
of calls with `short` and `long` iterations are timed with device events; the time of one iteration is the median over the
pairs of (t_long - t_short) / (long - short), which leaves the set-up of a call out.  Prints one JSON line per shape and
operator: ms per iteration, the operator's algorithmic traffic per iteration, the rate it amounts to and its ratio to the
plain-copy rate measured on this hardware (6.2 TB/s, profiles/archive/r4b_hbm_copy_probe.txt); the Diff4th line also
carries its time as a ratio to NDF's and TGV's.  `--out profiles/diff4th_bench.jsonl` keeps the lines.  Kernel times: run
the same command under `rocprofv3 --kernel-trace --stats` in a run of its own."""
import numpy as np

import _prox_bench as B


def runs_of(args, shape, x, out):
    from tomobar_amd import ops
    # tau (1 + 16 nd^2 lam) = 0.73 in 3D: inside the stability bound; sigma of the size of the synthetic gradient
    lam, sigma, tau = np.float32(1.0), np.float32(2.0), np.float32(0.005)
    tgv_tau = np.float32(np.float32(1.0) / np.sqrt(np.float32(12.0)))
    if not args.no_tgv:
        ops.reserve_tv_scratch(shape, "cuda:0", "TGV")   # the largest of the arenas: nothing is re-placed in between
    ops.reserve_tv_scratch(shape, "cuda:0", "Diff4th")
    gx = 0.5 * (x[..., 2:] - x[..., :-2])
    active = float((gx * gx > float(sigma) ** 2).float().mean())
    runs = [("diff4th", B.BYTES_PER_VOXEL, lambda n: ops.diff4th(x, out, lam, sigma, tau, n))]
    if not args.no_ndf:
        runs.append(("ndf_Huber", B.BYTES_PER_VOXEL, lambda n: ops.ndf(x, out, lam, sigma, np.float32(0.05), "Huber", n)))
    if not args.no_tgv:
        runs.append(("tgv", B.TGV_BYTES_PER_VOXEL[len(shape)], lambda n: ops.tgv(x, out, 5.0, 1.0, 2.0, tgv_tau, tgv_tau, n)))
    return runs, {"x_gradient_squared_above_sigma_squared": round(active, 3)}


if __name__ == "__main__":
    B.main("diff4th_bench", runs_of, ratios_of=("ndf_Huber", "tgv"),
           options=[("--no-ndf", "skip the NDF comparison"), ("--no-tgv", "skip the TGV comparison")])
