"""Matched against shipped back projector on the same arrays in one process (docs/kernels/bp_matched.md).

Median of 5 calls (after one warm-up call each, the four entry points taken in turn) of tomo_bp3d_matched and
tomo_bp3d_matched_fista against tomo_bp3d and tomo_bp3d_fista, planar input, at 1024^3 x 75 angles and 512^3 x 60 angles;
device events around each call.  One JSON line per shape, appended to profiles/bp_matched_bench.jsonl.

usage: python tools/bp_matched_bench.py [--out FILE] [--shapes n:angles[,n:angles...]]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tomobar_amd.projector import HipTools3D  # noqa: E402

REPEATS = 5


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def bench(n, na):
    H = HipTools3D(n, 0, n, np.linspace(0, np.pi, na, endpoint=False), 0.0, n, "gpu", 0, None)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    sino = torch.randn(H.sino_shape(None), device="cuda", generator=gen)
    x_t = torch.rand(H.vol_shape(), device="cuda", generator=gen)
    out = torch.empty_like(x_t)

    def plain(adjoint):
        return lambda: H.backward(sino, None, out=out, adjoint=adjoint)

    def fista(adjoint):
        def run():
            H.adjoint = adjoint
            H.grad_step(sino, x_t, out, 1e-3, True, None)
        return run

    calls = {"bp3d": plain("unmatched"), "bp3d_matched": plain("matched"),
             "bp3d_fista": fista("unmatched"), "bp3d_matched_fista": fista("matched")}
    paths, times = {}, {k: [] for k in calls}
    for k, fn in calls.items():          # warm-up: code objects, the relay arena of the shipped projector
        fn()
        paths[k] = H.kernel_path("bp")
    torch.cuda.synchronize()
    for _ in range(REPEATS):             # the four in turn, so that a drift of the clock hits all alike
        for k, fn in calls.items():
            times[k].append(timed(fn))
    H.adjoint = "unmatched"
    med = {k: statistics.median(v) for k, v in times.items()}
    return {"n": n, "nz": n, "nu": n, "angles": na, "repeats": REPEATS, "device": torch.cuda.get_device_name(0),
            "median_ms": {k: round(v, 4) for k, v in med.items()},
            "min_ms": {k: round(min(v), 4) for k, v in times.items()},
            "max_ms": {k: round(max(v), 4) for k, v in times.items()},
            "ratio_plain": round(med["bp3d_matched"] / med["bp3d"], 3),
            "ratio_fista": round(med["bp3d_matched_fista"] / med["bp3d_fista"], 3),
            "kernel_path": paths}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bp_matched_bench.jsonl"))
    ap.add_argument("--shapes", default="1024:75,512:60")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bp_matched_bench needs a GPU: nothing is measured without one")
    for item in args.shapes.split(","):
        n, na = (int(v) for v in item.split(":"))
        line = json.dumps(bench(n, na))
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
