"""Generate tests/golden/tv_dispatch_digests.json -- the outputs of the TV operators, pinned per dispatch arm (GPU).

For every (operator, variant, dual type) below the fixture records the SHA-256 of the output of every call that reaches a
different arm of the host dispatch in tomobar_amd/csrc/tv_kernels.hip: both TV types with and without the nonnegativity
clip (the data holds negative values, so the no-clip arms must pass them through), 2D images and 3D volumes, iteration
counts that are cut into every launch sequence (first = last launch, 3, 2 + 2, 3 + 2, 3 + 2 + 2, trailing single
iterations), 3D volumes of one and two planes (fewer iterations per launch than the variant's own), an in-place call and
a call that a tolerance stops early.  Variants 0 and 22 run the shipped library, the others libtomo_mi355x_dev.so.
Only the public Python surface is used, so the file runs unchanged on an older checkout: that is how the fixture is
recorded before a change to the dispatch and compared after it.  tests/test_gpu_tv_dispatch.py reads CASES and record().

    python tests/golden/make_tv_dispatch_digests.py
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "tv_dispatch_digests.json")

SHIPPED = {"pdtv": (0, 22), "roftv": (0,)}
# operator, variant, binary16 duals / D fields (the workgroup-shape builds 31 / 32 exist for float32 duals only)
CASES = ([("pdtv", v, h) for v in (0, 22, 1, 2, 3, 21) for h in (False, True)] + [("pdtv", 31, False), ("pdtv", 32, False)]
         + [("roftv", v, h) for v in (0, 1, 2, 3, 4) for h in (False, True)])

# shapes of TV_SHAPES in tests/test_gpu_parity.py: one tile and several tiles per plane; (12, 1, 70) is squeezed to 2D
SHAPES_3D = [(6, 9, 13), (20, 70, 150)]
SHAPES_2D = [(24, 19), (12, 1, 70)]
SHAPES_THIN = [(1, 20, 17), (2, 20, 17)]   # run as nd = 3 through ops.pdtv
PD_ITERS = (0, 1, 2, 3, 4, 5, 7, 11)
ROF_ITERS = (0, 1, 2, 5)
REG, LIPSCHITZ = 0.04, 8.0
ROF_REG, ROF_TAU = 0.05, 0.005


def key(case):
    op, variant, half = case
    return f"{op}/v{variant}/{'f16' if half else 'f32'}"


def _data(shape):
    rng = np.random.default_rng(5)
    x = rng.random(shape) * 0.3 + (np.indices(shape)[-1] > shape[-1] // 2)
    return (x - 0.6).astype(np.float32)   # negative values: the no-clip arms must keep them


def _sha(t):
    import torch
    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()


def _shape_name(shape):
    return "x".join(str(s) for s in shape)


def _record_pdtv(half):
    import torch
    from tomobar_amd import ops
    from tomobar_amd.regularisersCuPy import PD_TV_cupy, last_prox
    out = {}
    for shape in SHAPES_3D + SHAPES_2D:
        x = torch.from_numpy(_data(shape)).cuda()
        for mtv in (0, 1):
            for nn in (0, 1):
                for it in PD_ITERS:
                    got = PD_TV_cupy(x, REG, it, mtv, nn, LIPSCHITZ, 0, half)
                    out[f"{_shape_name(shape)}/tv{mtv}/nn{nn}/it{it}"] = _sha(got)
    # the scalar set-up of PD_TV_cupy
    tau = np.float32(REG * 0.1)
    sigma = np.float32(1.0 / (LIPSCHITZ * tau))
    lt = np.float32(tau / REG)
    for shape in SHAPES_THIN:
        x = torch.from_numpy(_data(shape)).cuda()
        for mtv in (0, 1):
            for nn in (0, 1):
                for it in PD_ITERS:
                    got = ops.pdtv(x, torch.empty_like(x), sigma, tau, lt, np.float32(1.0), it, mtv, nn, half)
                    out[f"thin{_shape_name(shape)}/tv{mtv}/nn{nn}/it{it}"] = _sha(got)
    for shape in (SHAPES_3D[1], SHAPES_2D[0]):
        for it in (4, 7):
            x = torch.from_numpy(_data(shape)).cuda()
            PD_TV_cupy(x, REG, it, 0, 1, LIPSCHITZ, 0, half, out=x)
            out[f"{_shape_name(shape)}/inplace/it{it}"] = _sha(x)
        x = torch.from_numpy(_data(shape)).cuda()
        got = PD_TV_cupy(x, REG, 60, 0, 1, LIPSCHITZ, 0, half, tolerance=2e-2)
        done = last_prox()[0]
        assert 0 < done < 60, done   # the case is there for the early exit
        out[f"{_shape_name(shape)}/tol/done{done}"] = _sha(got)
    return out


def _record_roftv(half):
    import torch
    from tomobar_amd.regularisersCuPy import ROF_TV_cupy
    out = {}
    for shape in SHAPES_3D + SHAPES_2D:
        for it in ROF_ITERS:
            x = torch.from_numpy(_data(shape)).cuda()
            got = ROF_TV_cupy(x, ROF_REG, it, ROF_TAU, 0, half)
            out[f"{_shape_name(shape)}/it{it}"] = _sha(got)
            ROF_TV_cupy(x, ROF_REG, it, ROF_TAU, 0, half, out=x)
            out[f"{_shape_name(shape)}/inplace/it{it}"] = _sha(x)
    return out


def record(case):
    """{call: sha256 of its output} for one (operator, variant, dual type), run under the library flavour that carries
    the variant."""
    from tomobar_amd import _lib, ops
    op, variant, half = case
    with _lib.use_flavour("shipped" if variant in SHIPPED[op] else "dev"):
        ops.set_variant(op, variant)
        try:
            return _record_pdtv(half) if op == "pdtv" else _record_roftv(half)
        finally:
            ops.set_variant(op, 0)


def main():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    dst = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    table = {}
    for case in CASES:
        table[key(case)] = record(case)
        print(key(case), len(table[key(case)]), flush=True)
    with open(dst, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
