"""Timing of the NDF regulariser (tomo_ndf: one launch per iteration, docs/kernels/ndf.md) on synthetic data, per penalty,
with ROF_TV -- the same algorithmic traffic -- timed beside it on the same arrays.

usage: python tools/ndf_bench.py [--shapes 512x512x512,1024x1024x1024,4096x4096] [--reps 5] [--short 4] [--long 14] [--out FILE]

Per shape: the placed scratch arena is reserved first, every operator is warmed up, then `reps` pairs of calls with `short`
and `long` iterations are timed with device events; the time of one iteration is the median over the pairs of
(t_long - t_short) / (long - short), which leaves the set-up of a call out.  Prints one JSON line per shape and operator:
ms per iteration, the algorithmic traffic (3 floats = 12 B per voxel and iteration: U and f read, U' written), the rate it
amounts to and its ratio to the plain-copy rate measured on this hardware (6.2 TB/s,
profiles/archive/r4b_hbm_copy_probe.txt).  Kernel times: run the same command under `rocprofv3 --kernel-trace --stats` in
a run of its own."""
import numpy as np

import _prox_bench as B

PENALTIES = ("Huber", "PM", "Tukey")


def runs_of(args, shape, x, out):
    from tomobar_amd import ops
    lam, sigma, tau = np.float32(1.0), np.float32(2.0), np.float32(0.05)
    ops.reserve_tv_scratch(shape, "cuda:0", "ROF_TV")   # the larger of the two arenas: nothing is re-placed in between
    ops.reserve_tv_scratch(shape, "cuda:0", "NDF")
    above = float(((x[..., 1:] - x[..., :-1]).abs() > float(sigma)).float().mean())
    runs = [(f"ndf_{p}", B.BYTES_PER_VOXEL, (lambda n, p=p: ops.ndf(x, out, lam, sigma, tau, p, n))) for p in PENALTIES]
    if not args.no_rof:
        runs.append(("roftv", B.BYTES_PER_VOXEL, lambda n: ops.roftv(x, out, np.float32(0.05), np.float32(0.005), n, False)))
    return runs, {"x_differences_above_sigma": round(above, 3)}


if __name__ == "__main__":
    B.main("ndf_bench", runs_of, options=[("--no-rof", "skip the ROF_TV comparison")])
