"""What early stopping costs: times tomo_rel_change (with and without the snapshot refresh) and a 60-iteration PD_TV /
ROF_TV call with the tolerance off and on-but-never-met, at 1024^3 and 256 x 2048^2 (docs/kernels/convergence.md).

    python tools/conv_bench.py [--shapes 1024,1024,1024 256,2048,2048] [--reps 5] [--nontemporal]

--nontemporal repeats the tomo_rel_change timings with non-temporal loads / stores (dev flavour, probe bit 64): the A/B
that decides which form ships.  Prints one JSON line per measurement."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tomobar_amd import _lib, ops  # noqa: E402


def timed(fn, reps):
    """median wall time in ms of `fn` (every call ends synchronised), after one warm-up call"""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), [round(m, 3) for m in ms]


def rel_change_rows(shape, reps, label):
    n = int(np.prod(shape))
    x = torch.rand(n, device="cuda")
    ref = torch.rand(n, device="cuda")
    for keep, nbytes in ((None, 8), (ref, 12)):
        ms, all_ms = timed(lambda: ops.rel_change(x, ref, keep), reps)
        print(json.dumps({"what": "tomo_rel_change", "form": label, "shape": list(shape), "keep": keep is not None,
                          "bytes_per_voxel": nbytes, "ms": round(ms, 3), "GBps": round(n * nbytes / ms / 1e6, 1), "all_ms": all_ms}))
    del x, ref
    torch.cuda.empty_cache()


def tv_rows(shape, reps, iterations=60):
    x = torch.rand(shape, device="cuda")
    out = torch.empty_like(x)
    s = (np.float32(1.0 / (8.0 * 0.005)), np.float32(0.005), np.float32(0.1), np.float32(1.0))
    never = 1e-30   # on, never met: every check runs, the loop never stops
    for name, off, on in (("PD_TV", lambda: ops.pdtv(x, out, *s, iterations, 0, 0, False),
                           lambda: ops.pdtv_tol(x, out, *s, iterations, 0, 0, False, never)),
                          ("ROF_TV", lambda: ops.roftv(x, out, np.float32(0.05), np.float32(0.005), iterations, False),
                           lambda: ops.roftv_tol(x, out, np.float32(0.05), np.float32(0.005), iterations, False, never))):
        t_off, a_off = timed(off, reps)
        t_on, a_on = timed(on, reps)
        print(json.dumps({"what": name, "shape": list(shape), "iterations": iterations, "checks": 9, "ms_off": round(t_off, 2),
                          "ms_on_never_met": round(t_on, 2), "overhead_pct": round(100.0 * (t_on / t_off - 1.0), 2),
                          "ms_per_check": round((t_on - t_off) / 9, 3), "all_ms_off": a_off, "all_ms_on": a_on}))
    del x, out
    ops_release()


def ops_release():
    torch.cuda.synchronize()
    _lib.check(_lib.lib().tomo_release_scratch(0))
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["1024,1024,1024", "256,2048,2048"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nontemporal", action="store_true")
    ap.add_argument("--skip-tv", action="store_true")
    args = ap.parse_args()
    for spec in args.shapes:
        shape = tuple(int(v) for v in spec.split(","))
        rel_change_rows(shape, args.reps, "plain")
        if args.nontemporal:
            with _lib.use_flavour("dev"):
                ops.set_variant("probe", 64)
                try:
                    rel_change_rows(shape, args.reps, "nontemporal")
                finally:
                    ops.set_variant("probe", 0)
                rel_change_rows(shape, args.reps, "plain (dev flavour)")
        if not args.skip_tv:
            tv_rows(shape, args.reps)


if __name__ == "__main__":
    main()
