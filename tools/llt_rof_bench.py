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
import numpy as np

import _prox_bench as B


def runs_of(args, shape, x, out):
    from tomobar_amd import ops
    lam_rof, lam_llt, tau = np.float32(0.3), np.float32(0.1), np.float32(0.02)   # set A of tests/_llt_rof_oracle.py
    # the siblings' parameters are those of tools/diff4th_bench.py
    lam, sigma, d4_tau = np.float32(1.0), np.float32(2.0), np.float32(0.005)
    if not args.no_siblings:
        ops.reserve_tv_scratch(shape, "cuda:0", "ROF_TV")   # the largest of the four arenas: nothing is re-placed in between
    ops.reserve_tv_scratch(shape, "cuda:0", "LLT_ROF")
    runs = [("llt_rof", B.BYTES_PER_VOXEL, lambda n: ops.llt_rof(x, out, lam_rof, lam_llt, tau, n))]
    if not args.no_siblings:
        runs.append(("diff4th", B.BYTES_PER_VOXEL, lambda n: ops.diff4th(x, out, lam, sigma, d4_tau, n)))
        runs.append(("ndf_Huber", B.BYTES_PER_VOXEL, lambda n: ops.ndf(x, out, lam, sigma, np.float32(0.05), "Huber", n)))
        runs.append(("rof_tv", B.BYTES_PER_VOXEL, lambda n: ops.roftv(x, out, np.float32(0.05), np.float32(0.005), n, False)))
    return runs, {}


if __name__ == "__main__":
    B.main("llt_rof_bench", runs_of, ratios_of=("diff4th", "ndf_Huber", "rof_tv"),
           options=[("--no-siblings", "skip Diff4th, NDF and ROF_TV")])
