"""Timing of RecToolsIRCuPy.PDHG (docs/kernels/pdhg.md: per iteration one forward projection, the sinogram dual, one matched
back projection, the TV dual and the primal) on synthetic data.

usage: python tools/pdhg_bench.py [--shapes 512:360,1024:900] [--fidelity LS] [--regulariser tv|tgv] [--preconditioner diagonal]
                                  [--power-method] [--reps 5] [--short 4] [--long 14] [--out FILE]
       python tools/pdhg_bench.py --kernel-db RESULTS.db [--regulariser tv|tgv] [--preconditioner diagonal] [--out FILE]
       python tools/pdhg_bench.py --stripe [--stripe-shapes 1024:900:1024,1:1800:2560] [--fidelity LS] [--rounds 3] [--reps 20]

--stripe times the fused launch of the stripe variable (tomo_pdhg_sino_dual_stripe: step 2 on r + s-bar and the sums of y along
the angles, 16.06 B per sample) against the plain sinogram dual (tomo_pdhg_sino_dual, 16 B) on the same arrays of nz:angles:nu
samples, alternately: `rounds` rounds of `reps` plain launches, then `reps` fused ones, each timed with device events; per round
the medians and their ratio, and the plain launch's own spread between the rounds, which is what a ratio can be read against.
Its lines go to profiles/pdhg_stripe_bench.jsonl.

--regulariser tgv times PD_TGV, the second-order TGV term in the dual (two marches of 88 + 88 B per voxel in 3D, 92 B for the
primal with a step per voxel, in place of the TV pair); its lines go to profiles/pdhg_tgv_bench.jsonl.

--preconditioner diagonal times the diagonally preconditioned driver (steps from A 1 and A^T 1 at the set-up of every call,
20 B per sample and 32 B per voxel in the split); --power-method leaves lipschitz_const out of the scalar run, so that
`ms_set_up_per_call` -- a short call minus its iterations -- shows what the power method costs.

Per shape n:angles (an n^3 volume, n detector columns): one warm-up call, then `reps` pairs of calls with `short` and `long`
iterations timed with device events; the time of one iteration is the median over the pairs of
(t_long - t_short) / (long - short), which leaves the set-up of a call out.  The Lipschitz constant is given, so the power
method is not part of a call.  One JSON line per shape, appended to profiles/pdhg_bench.jsonl.

The split over the five launches comes from a run of its own under the profiler,
    rocprofv3 --kernel-trace --stats -d DIR -o pdhg -- python tools/pdhg_bench.py --shapes 1024:900 --reps 1 --out /dev/null
whose database the second form reads: per launch group the calls, the mean time and the share of the kernel time, and for
the three new launches the rate over their algorithmic bytes (TV dual + primal: 28 + 28 B per voxel in 3D; the sinogram
dual: 16 B per sample) against the plain-copy rate measured on this hardware (6.2 TB/s,
profiles/archive/r4b_hbm_copy_probe.txt); give --shapes with the ONE shape the profiled run used."""
import argparse
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE_GBPS = 6200.0
# regular expressions on the kernel names of csrc/pdhg_kernels.hip, which SPDHG's launches share: the functor names the launch,
# the dual march's third template argument says whether it also writes e (SPDHG) or not (PDHG)
GROUPS = (("pdhg_tgv_dual_march", "tgv_dual"), ("pdhg_tgv_primal_march", "tgv_primal"),   # in front of the functor names they carry
          ("PdhgSino", "sino_dual"), (r"tv_dual_march<\d, \w+, false,", "tv_dual"), ("PdhgUpdate", "primal"),
          ("PdhgDiagUpdate", "primal"), ("DiagSteps", "diag_steps"), ("bp_", "bp"),
          ("fp_", "fp"), ("transpose64", "fp"))   # the in-plane transpose in front of the forward projector
# algorithmic bytes per voxel / per sample of (TV dual, primal, sinogram dual): the diagonal launches read one more array
BYTES = {None: (28, 28, 16), "diagonal": (28, 32, 20)}
# the same for (TGV dual, TGV primal, sinogram dual)
TGV_BYTES = {None: (88, 88, 16), "diagonal": (88, 92, 20)}
REGULARISERS = {"tv": {"method": "PD_TV", "regul_param": 0.5, "methodTV": 0},
                "tgv": {"method": "PD_TGV", "regul_param": 0.5, "TGV_alpha1": 1.0, "TGV_alpha2": 2.0}}


def bench(n, na, args):
    import numpy as np
    import torch
    from tomobar_amd.methodsIR_CuPy import RecToolsIRCuPy
    rt = RecToolsIRCuPy(n, 0, n, 0.0, np.linspace(0, np.pi, na, endpoint=False), n, 0, None, adjoint="matched")
    gen = torch.Generator(device="cuda").manual_seed(3)
    sino = torch.rand((n, na, n), device="cuda", generator=gen) * (0.5 * n)
    reg = REGULARISERS[args.regulariser]
    out = [None]

    algo = {"nonnegativity": True, "recon_mask_radius": None}
    if args.preconditioner is not None:      # its steps come from A 1 and A^T 1: two projections at set-up, no operator norm
        algo["PDHG_preconditioner"] = args.preconditioner
    elif not args.power_method:
        algo["lipschitz_const"] = float(n) * na

    def run(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out[0] = rt.PDHG({"projection_data": sino, "data_fidelity": args.fidelity}, dict(algo, iterations=iters), dict(reg))
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    run(args.short)   # warm-up: code objects, the placed block
    per_iter, calls, set_up = [], [], []
    for _ in range(args.reps):
        ts, tl = run(args.short), run(args.long)
        per_iter.append((tl - ts) / (args.long - args.short))
        calls.append(tl)
        set_up.append(ts - args.short * per_iter[-1])   # what a call costs beside its iterations
    from tomobar_amd import ops
    return {"op": "pdhg", "fidelity": args.fidelity, "regulariser": reg["method"], "preconditioner": args.preconditioner,
            "steps_from": "A1 and AT1" if args.preconditioner else ("power method" if args.power_method else "given"),
            "n": n, "nz": n, "nu": n, "angles": na, "reps": args.reps,
            "device": torch.cuda.get_device_name(0), "ms_per_iteration": round(statistics.median(per_iter), 3),
            "ms_per_iteration_min_max": [round(min(per_iter), 3), round(max(per_iter), 3)],
            f"ms_per_call_{args.long}_iterations": round(statistics.median(calls), 2),
            "ms_set_up_per_call": round(statistics.median(set_up), 2),
            "kernel_path": {"fp": rt.Atools.kernel_path("fp"), "bp": rt.Atools.kernel_path("bp")},
            "finite": bool(torch.isfinite(out[0]).all()), "placement": ops.placement_last()}


def stripe_bench(nz, na, nu, args):
    """the fused launch against the plain sinogram dual on the same y, r, b: alternately, `rounds` times"""
    import torch
    from tomobar_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(4)
    y, r, b = (torch.rand((nz, na, nu), device="cuda", generator=gen) for _ in range(3))
    sbar = torch.rand((nz, nu), device="cuda", generator=gen)
    s = torch.zeros((nz, nu), device="cuda")
    part = torch.empty((ops.pdhg_stripe_segments(na), nz, nu), device="cuda")
    sigma = 0.25
    launches = {"plain": lambda: ops.pdhg_sino_dual(y.view(-1), r.view(-1), b.view(-1), args.fidelity, sigma),
                "fused": lambda: ops.pdhg_sino_dual_stripe(y, r, b, sbar, part, args.fidelity, sigma),
                "update": lambda: ops.pdhg_stripe_update(s, sbar, part, na, 0.01, 0.5)}

    def median_ms(fn):
        times = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        return statistics.median(times)

    for fn in launches.values():   # warm-up: code objects
        fn()
    torch.cuda.synchronize()
    rounds = [{name: round(median_ms(fn), 4) for name, fn in launches.items()} for _ in range(args.rounds)]
    plain = [q["plain"] for q in rounds]
    fused = [q["fused"] for q in rounds]
    samples = nz * na * nu
    byte_ratio = (16.0 * samples + 4.0 * nz * nu * (1 + part.shape[0])) / (16.0 * samples)
    best = min(fused)
    return {"op": "pdhg_stripe", "fidelity": args.fidelity, "nz": nz, "angles": na, "nu": nu, "rounds": rounds, "reps": args.reps,
            "device": torch.cuda.get_device_name(0), "ms_fused_min_max": [min(fused), max(fused)],
            "ms_plain_min_max": [min(plain), max(plain)], "ratio_per_round": [round(f / p, 4) for f, p in zip(fused, plain)],
            "plain_spread_between_rounds": round(max(plain) / min(plain) - 1.0, 4), "byte_ratio": round(byte_ratio, 4),
            "fused_algorithmic_GBps": round(16.0 * samples * byte_ratio / (best * 1e-3) / 1e9, 1),
            "fused_ratio_to_copy_rate_6200_GBps": round(16.0 * samples * byte_ratio / (best * 1e-3) / 1e9 / COPY_RATE_GBPS, 3),
            "finite": bool(torch.isfinite(part).all())}


def split(db_path, n, na, preconditioner=None, regulariser="tv"):
    """the launch groups of a profiled run: calls, mean ms per launch, ms per iteration, share of the kernel time; rates of
    the three new launches"""
    import sqlite3
    rows = sqlite3.connect(db_path).execute("select name, count(*), sum(duration) from kernels group by name").fetchall()
    agg = {}
    for name, calls, total in rows:
        group = next((g for key, g in GROUPS if re.search(key, name)), "other")
        c, t = agg.get(group, (0, 0.0))
        agg[group] = (c + calls, t + total / 1e6)
    whole = sum(t for _, t in agg.values()) or 1.0
    dual, primal = ("tgv_dual", "tgv_primal") if regulariser == "tgv" else ("tv_dual", "primal")
    iterations = agg.get(primal, (1, 0.0))[0]   # one primal launch per iteration
    line = {"op": "pdhg_split", "regulariser": REGULARISERS[regulariser]["method"], "preconditioner": preconditioner, "n": n, "angles": na, "iterations": iterations,
            "groups": {g: {"calls": c, "mean_ms": round(t / c, 4), "ms_per_iteration": round(t / iterations, 3),
                           "share": round(t / whole, 4)} for g, (c, t) in sorted(agg.items())}}
    new = sum(agg.get(g, (0, 0.0))[1] for g in ("sino_dual", dual, primal))
    line["share_of_the_three_new_launches"] = round(new / whole, 4)
    per_dual, per_primal, per_sample = (TGV_BYTES if regulariser == "tgv" else BYTES)[preconditioner]
    nbytes = {dual: per_dual * n ** 3, primal: per_primal * n ** 3, "sino_dual": per_sample * n * n * na}
    for g, b in nbytes.items():
        if g in agg:
            rate = b / (agg[g][1] / agg[g][0] * 1e-3) / 1e9
            line["groups"][g].update(algorithmic_GBps=round(rate, 1), ratio_to_copy_rate_6200_GBps=round(rate / COPY_RATE_GBPS, 3))
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="512:360,1024:900")
    ap.add_argument("--fidelity", default="LS", choices=("LS", "L1", "KL"))
    ap.add_argument("--regulariser", default="tv", choices=tuple(REGULARISERS), help="PD_TV (the default) or PD_TGV in the dual")
    ap.add_argument("--preconditioner", default=None, choices=("diagonal",), help="_algorithm_['PDHG_preconditioner']")
    ap.add_argument("--power-method", action="store_true", help="scalar steps without a given lipschitz_const: every call runs the power method")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--short", type=int, default=4)
    ap.add_argument("--long", type=int, default=14)
    ap.add_argument("--kernel-db", default=None, help="summarise the kernels table of a rocprofv3 --kernel-trace --stats run instead")
    ap.add_argument("--stripe", action="store_true", help="time the stripe variable's fused launch against the plain sinogram dual")
    ap.add_argument("--stripe-shapes", default="1024:900:1024,1:1800:2560", help="nz:angles:nu of --stripe")
    ap.add_argument("--rounds", type=int, default=3, help="rounds of --stripe")
    ap.add_argument("--out", default=None, help="default: profiles/pdhg_bench.jsonl, profiles/pdhg_tgv_bench.jsonl with --regulariser tgv, "
                                                "profiles/pdhg_stripe_bench.jsonl with --stripe")
    args = ap.parse_args()
    if args.out is None:
        name = "pdhg_stripe_bench.jsonl" if args.stripe else "pdhg_tgv_bench.jsonl" if args.regulariser == "tgv" else "pdhg_bench.jsonl"
        args.out = os.path.join(ROOT, "profiles", name)
    if not 0 < args.short < args.long or args.reps < 1:
        ap.error("need 0 < --short < --long and --reps >= 1")
    shapes = [tuple(int(v) for v in item.split(":")) for item in args.shapes.split(",")]
    lines = []
    if args.stripe:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("pdhg_bench needs a GPU (there is no CPU path)")
        if args.rounds < 2:
            ap.error("--stripe needs --rounds >= 2: the plain launch's spread between rounds is part of the result")
        for item in args.stripe_shapes.split(","):
            lines.append(stripe_bench(*(int(v) for v in item.split(":")), args))
            print(json.dumps(lines[-1]), flush=True)
            torch.cuda.empty_cache()
    elif args.kernel_db:
        if len(shapes) != 1:
            ap.error("--kernel-db needs --shapes with the one shape the profiled run used")
        lines.append(split(args.kernel_db, *shapes[0], args.preconditioner, args.regulariser))
        print(json.dumps(lines[-1]), flush=True)
    else:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("pdhg_bench needs a GPU (there is no CPU path)")
        for n, na in shapes:
            lines.append(bench(n, na, args))
            print(json.dumps(lines[-1]), flush=True)
            torch.cuda.empty_cache()
    with open(args.out, "a") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
