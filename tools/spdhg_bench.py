"""Timing of RecToolsIRCuPy.SPDHG (docs/kernels/spdhg.md: a subset update is one forward projection of a subset, the
sinogram dual, one matched back projection and the streaming primal; a TV update is the TV dual and the TV primal) on
synthetic data.

usage: python tools/spdhg_bench.py [--shapes 512:360,1024:900] [--subsets 12] [--reps 5] [--short 1] [--long 3] [--out FILE]
       python tools/spdhg_bench.py --kernel-db RESULTS.db [--out FILE]

Per shape n:angles (an n^3 volume, n detector columns), LS + TV with non-negativity: one warm-up call, then `reps` pairs of
calls with `short` and `long` epochs timed with device events; the time of one epoch is the median over the pairs of
(t_long - t_short) / (long - short), which leaves the set-up of a call out.  The same pairs without the regulariser (every
block update is a subset update) give the time of a subset update; the TV update is what the epochs with TV take beyond
their subset updates, over the TV updates the draws of those epochs hold (last_run["block_updates"]).  The Lipschitz
constant is given, so the power method is not part of a call.  One JSON line per shape, appended to
profiles/spdhg_bench.jsonl.

The split over the launches comes from a run of its own under the profiler,
    rocprofv3 --kernel-trace --stats -d DIR -o spdhg -- python tools/spdhg_bench.py --shapes 1024:900 --reps 1 --out /dev/null
whose database the second form reads: per launch group the calls, the mean time and the share of the kernel time, and for
the four new launches the rate over their algorithmic bytes (sinogram dual 20 B per sample, streaming primal 20 B per
voxel, TV dual 40 and TV primal 28 B per voxel in 3D) against the plain-copy rate measured on this hardware (6.2 TB/s,
profiles/archive/r4b_hbm_copy_probe.txt); give --shapes and --subsets with the ONE shape the profiled run used."""
import argparse
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE_GBPS = 6200.0
NEW = ("sino_dual", "primal", "tv_dual", "tv_primal")
# regular expressions on the kernel names of csrc/pdhg_kernels.hip, which PDHG's launches share: the functor names the launch,
# the dual march's third template argument says whether it also writes e (SPDHG) or not (PDHG)
GROUPS = (("StochSino", "sino_dual"), ("StochPrimal", "primal"), (r"tv_dual_march<\d, \w+, true,", "tv_dual"),
          ("StochTvUpdate", "tv_primal"), ("bp_", "bp"), ("fp_", "fp"),
          ("transpose64", "fp"))   # the in-plane transpose in front of the forward projector


def bench(n, na, args):
    import numpy as np
    import torch
    from tomobar_amd.methodsIR_CuPy import RecToolsIRCuPy
    rt = RecToolsIRCuPy(n, 0, n, 0.0, np.linspace(0, np.pi, na, endpoint=False), n, 0, args.subsets, adjoint="matched")
    gen = torch.Generator(device="cuda").manual_seed(3)
    sino = torch.rand((n, na, n), device="cuda", generator=gen) * (0.5 * n)
    reg = {"method": "PD_TV", "regul_param": 0.5, "methodTV": 0}
    out = [None]

    def run(epochs, tv):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out[0] = rt.SPDHG({"projection_data": sino, "data_fidelity": "LS"},
                          {"iterations": epochs, "lipschitz_const": float(n) * na / args.subsets, "nonnegativity": True,
                           "recon_mask_radius": None}, dict(reg) if tv else None)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), rt.last_run["block_updates"]

    def pairs(tv):
        run(args.short, tv)   # warm-up: code objects, the placed block
        per_epoch, calls, counts = [], [], None
        for _ in range(args.reps):
            (ts, cs), (tl, cl) = run(args.short, tv), run(args.long, tv)
            per_epoch.append((tl - ts) / (args.long - args.short))
            calls.append(tl)
            counts = (cl[0] - cs[0], cl[1] - cs[1])   # the block updates of the epochs the difference times
        return per_epoch, calls, counts

    plain, _, plain_counts = pairs(False)
    with_tv, calls, counts = pairs(True)
    span = args.long - args.short
    ms_subset = statistics.median(plain) * span / plain_counts[0]
    ms_epoch = statistics.median(with_tv)
    ms_tv = (ms_epoch * span - counts[0] * ms_subset) / counts[1]
    from tomobar_amd import ops
    return {"op": "spdhg", "fidelity": "LS", "n": n, "nz": n, "nu": n, "angles": na, "subsets": args.subsets, "reps": args.reps,
            "device": torch.cuda.get_device_name(0), "ms_per_epoch": round(ms_epoch, 3),
            "ms_per_epoch_min_max": [round(min(with_tv), 3), round(max(with_tv), 3)],
            "block_updates_of_the_timed_epochs": {"subset": counts[0], "tv": counts[1], "epochs": span},
            "ms_per_subset_update": round(ms_subset, 3), "ms_per_tv_update": round(ms_tv, 3),
            "ms_per_epoch_without_tv": round(statistics.median(plain), 3),
            f"ms_per_call_{args.long}_epochs": round(statistics.median(calls), 2),
            "kernel_path": {"fp": rt.Atools.kernel_path("fp"), "bp": rt.Atools.kernel_path("bp")},
            "finite": bool(torch.isfinite(out[0]).all()), "placement": ops.placement_last()}


def split(db_path, n, na, subsets):
    """the launch groups of a profiled run: calls, mean ms per launch, share of the kernel time; the time of a subset and of
    a TV update from their launches; rates of the four new launches"""
    import sqlite3
    rows = sqlite3.connect(db_path).execute("select name, count(*), sum(duration) from kernels group by name").fetchall()
    agg = {}
    for name, calls, total in rows:
        group = next((g for key, g in GROUPS if re.search(key, name)), "other")
        c, t = agg.get(group, (0, 0.0))
        agg[group] = (c + calls, t + total / 1e6)
    whole = sum(t for _, t in agg.values()) or 1.0
    total = lambda *gs: sum(agg.get(g, (0, 0.0))[1] for g in gs)  # noqa: E731
    n_subset, n_tv = agg.get("primal", (0, 0.0))[0], agg.get("tv_primal", (0, 0.0))[0]
    line = {"op": "spdhg_split", "n": n, "angles": na, "subsets": subsets, "subset_updates": n_subset, "tv_updates": n_tv,
            "groups": {g: {"calls": c, "mean_ms": round(t / c, 4), "share": round(t / whole, 4)} for g, (c, t) in sorted(agg.items())}}
    if n_subset:
        line["ms_per_subset_update"] = round(total("fp", "sino_dual", "bp", "primal") / n_subset, 3)
    if n_tv:
        line["ms_per_tv_update"] = round(total("tv_dual", "tv_primal") / n_tv, 3)
    line["share_of_the_four_new_launches"] = round(total(*NEW) / whole, 4)
    nbytes = {"sino_dual": 20 * n * n * (na / subsets), "primal": 20 * n ** 3, "tv_dual": 40 * n ** 3, "tv_primal": 28 * n ** 3}
    for g, b in nbytes.items():
        if g in agg:
            rate = b / (agg[g][1] / agg[g][0] * 1e-3) / 1e9
            line["groups"][g].update(algorithmic_GBps=round(rate, 1), ratio_to_copy_rate_6200_GBps=round(rate / COPY_RATE_GBPS, 3))
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="512:360,1024:900")
    ap.add_argument("--subsets", type=int, default=12)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--short", type=int, default=1)
    ap.add_argument("--long", type=int, default=3)
    ap.add_argument("--kernel-db", default=None, help="summarise the kernels table of a rocprofv3 --kernel-trace --stats run instead")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spdhg_bench.jsonl"))
    args = ap.parse_args()
    if not 0 < args.short < args.long or args.reps < 1 or args.subsets < 1:
        ap.error("need 0 < --short < --long, --reps >= 1 and --subsets >= 1")
    shapes = [tuple(int(v) for v in item.split(":")) for item in args.shapes.split(",")]
    lines = []
    if args.kernel_db:
        if len(shapes) != 1:
            ap.error("--kernel-db needs --shapes with the one shape the profiled run used")
        lines.append(split(args.kernel_db, *shapes[0], args.subsets))
        print(json.dumps(lines[-1]), flush=True)
    else:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("spdhg_bench needs a GPU (there is no CPU path)")
        for n, na in shapes:
            lines.append(bench(n, na, args))
            print(json.dumps(lines[-1]), flush=True)
            torch.cuda.empty_cache()
    with open(args.out, "a") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
