"""Generate tests/golden/fp_plan_paths.json -- the forward projector's kernel choice, pinned per geometry (GPU).

For every case below, every subset it lists and every fp variant it names, the fixture records the kernel path string
(`tomo_ctx_kernel_path("fp")`) of a forward projection and of an LS residual, and the SHA-256 of both outputs on a seeded
float32 volume and sinogram.  Variant 0 runs the shipped library, the others libtomo_mi355x_dev.so.  The cases cover
every form of the selection: whole-row with merged axes (1-5 passes, every rows-per-chunk count, with and without lane
multipliers), whole-row per sign class on detectors wider than 1024, the dense 16-angle form and just below its
workgroup floor, 256-pixel pipelined tiles with 1-5 passes, the synchronous fallback and the march.
tests/test_gpu_fp_plan.py reads CASES and record() from this file.

    python tests/golden/make_fp_plan_paths.py
"""
import hashlib
import json
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "fp_plan_paths.json")

FULL = (0.1, math.pi + 0.1, False)   # np.linspace(a0, a1, na, endpoint) -- the parity tests' angle set

# name, nz, n, nu, na, angles, cor ("vec": per-angle), OS number, LERP8, fp variants
CASES = [
    ("wide1_mult", 8, 800, 800, 25, FULL, 0.0, 1, False, (0, 2, 4)),
    ("wide1_640", 4, 600, 640, 30, FULL, 0.0, 1, False, (0,)),
    ("wide2_kc4", 4, 256, 256, 40, FULL, 0.0, 1, False, (0, 3)),
    ("wide2_kc2_mult", 2, 1300, 1024, 16, FULL, 0.0, 1, False, (0, 4)),
    ("wide3_kc2_lerp8", 8, 300, 128, 20, FULL, 0.0, 1, True, (0,)),
    ("wide3_kc1_mult", 1, 9000, 1024, 8, (-0.21, 0.21, True), 0.0, 1, False, (0,)),
    ("wide4", 4, 1000, 200, 10, FULL, 0.0, 1, False, (0,)),
    ("wide5_and_tiles", 4, 1200, 256, 20, FULL, 0.0, 1, False, (0, 2)),
    ("sign_classes_2560_os", 2, 2560, 2560, 24, FULL, 0.0, 3, False, (0, 4)),
    ("sign_classes_2560_vec", 4, 1600, 2560, 30, FULL, "vec", 1, False, (0,)),
    ("dense", 16, 512, 512, 6144, (-0.6, 0.6, False), 0.0, 1, False, (0, 3, 4)),
    ("dense_below_floor", 16, 512, 512, 6000, (-0.6, 0.6, False), 0.0, 1, False, (0, 3)),
    ("tiles_1pass", 4, 200, 100, 20, FULL, 0.0, 1, False, (0, 1, 2)),
    ("tiles_2pass", 4, 400, 100, 20, FULL, 0.0, 1, False, (0,)),
    ("tiles_3_4pass", 4, 900, 100, 20, FULL, 0.0, 1, False, (0,)),
    ("tiles_4_5pass_lerp8", 4, 1200, 100, 20, FULL, 0.0, 1, True, (0,)),
    ("tiles_sync", 4, 2000, 100, 20, FULL, 0.0, 1, False, (0, 2)),
    ("march", 1, 4100, 4100, 4, (-0.77, 0.77, True), 0.0, 1, False, (0,)),
    ("os_tiles", 18, 70, 64, 31, FULL, -2.5, 4, False, (0, 2)),
    ("os_vec_wide_lerp8", 5, 780, 900, 18, FULL, "vec", 3, True, (0, 3, 4)),
]


def subsets(case):
    os_n = case[7]
    return [None] if os_n == 1 else [None, 0, os_n - 1]


def key(case, variant, s):
    return f"{case[0]}/v{variant}/s{'all' if s is None else s}"


def _sha(t):
    import torch
    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()


def record(case, variant):
    """{key: {"fp": path, "fp_sha256": ..., "res": path, "res_sha256": ...}} for one case and variant, run under the
    library flavour that carries the variant."""
    import torch
    from tomobar_amd import _lib, ops
    from tomobar_amd.projector import HipTools3D
    name, nz, n, nu, na, (a0, a1, endpoint), cor, os_n, lerp8, _ = case
    angles = np.linspace(a0, a1, na, endpoint=endpoint)
    if cor == "vec":
        cor = np.linspace(-1.5, 2.0, na)
    out = {}
    with _lib.use_flavour("shipped" if variant == 0 else "dev"):
        ops.set_variant("fp", variant)
        try:
            H = HipTools3D(nu, 0, nz, angles, cor, n, "gpu", 0, os_n if os_n > 1 else None, lerp8=lerp8)
            rng = np.random.default_rng(5)
            vol = torch.from_numpy(rng.standard_normal((nz, n, n), dtype=np.float32)).cuda()
            b = torch.from_numpy(rng.standard_normal((nz, na, nu), dtype=np.float32)).cuda()
            for s in subsets(case):
                fp = H.forward(vol, s)
                r = {"fp": H.kernel_path("fp"), "fp_sha256": _sha(fp)}
                del fp
                res = torch.empty(H.sino_shape(s), dtype=torch.float32, device="cuda")
                H.residual(vol, b, None, "LS", s, res)
                r.update({"res": H.kernel_path("fp"), "res_sha256": _sha(res)})
                out[key(case, variant, s)] = r
            del H, vol, b, res
            torch.cuda.empty_cache()
        finally:
            ops.set_variant("fp", 0)
    return out


def main():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    dst = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    table = {}
    for case in CASES:
        for v in case[-1]:
            rec = record(case, v)
            for k, r in rec.items():
                print(k, r["fp"], flush=True)
            table.update(rec)
    with open(dst, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
