"""Timing of the TGV prox (tomo_tgv: two launches per iteration, docs/kernels/tgv.md) on synthetic data.

usage: python tools/tgv_bench.py [--shapes 512x512x512,1024x1024x1024,4096x4096] [--reps 5] [--short 4] [--long 14] [--out FILE]

Per shape: the placed scratch arena is reserved first, every shape is warmed up, then `reps` pairs of calls with `short`
and `long` iterations are timed with device events; the time of one iteration is the median over the pairs of
(t_long - t_short) / (long - short), which leaves the set-up of a call (two copies and one fill of the arena) out.
Prints one JSON line per shape: ms per iteration, the algorithmic traffic (44 floats = 176 B per voxel and iteration in
3D, 28 floats = 112 B in 2D), the rate it amounts to and its ratio to the plain-copy rate measured on this hardware
(6.2 TB/s, profiles/archive/r4b_hbm_copy_probe.txt).  Kernel times: run the same command under
`rocprofv3 --kernel-trace --stats` in a run of its own."""
import numpy as np

import _prox_bench as B


def runs_of(args, shape, x, out):
    from tomobar_amd import ops
    tau = np.float32(np.float32(1.0) / np.sqrt(np.float32(12.0)))
    ops.reserve_tv_scratch(shape, "cuda:0", "TGV")
    return [("tgv", B.TGV_BYTES_PER_VOXEL[len(shape)], lambda n: ops.tgv(x, out, 5.0, 1.0, 2.0, tau, tau, n))], {}


if __name__ == "__main__":
    B.main("tgv_bench", runs_of)
