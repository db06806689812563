"""MI355X: the fused epilogues of BOTH back projectors (csrc/bp_common.h: bp_value behind bp_epilogue* of proj_kernels.hip /
bp_brick.inl and mb_epilogue* of bp_matched.hip) against ONE numpy-float32 restatement, and the folded 32 x 32 momentum /
transpose kernel.  The gradient the restatement starts from is the same kernel's plain epilogue (`backward`), which
accumulates in the same order, so every comparison is array_equal.

Shapes: the kernels own 32 x 16 x 16 voxel bricks.  17 x 64 x 64 has whole bricks (the dwordx4 hand-over through LDS) and a
ragged z-brick; the same with every volume array one float off 16-byte alignment stores whole bricks through the scalar
path; 5 x 37 x 37 has ragged bricks only."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _guarded import guarded  # noqa: E402

NA = 9
F32 = np.float32
LINV, BETA, TAU, RHO, ALPHA = F32(1 / 300.0), F32(0.37), F32(0.002), F32(1.7), F32(1.6)
OMA = F32(1.0 - 1.6)


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def restate(form, g, i0, i1=None, i2=None, nonneg=False, relax_on=False):
    """The three fused forms, one float32 rounding per operation (methodsIR_CuPy.py:463-475,545-557):
         "fista"      i0 = X_t                    -> X
         "fista_mom"  i0 = X_t, i1 = X_old        -> X, new X_t
         "admm"       i0 = z, i1 = u, i2 = x      -> z, z + u"""
    assert g.dtype == i0.dtype == np.float32
    if form in ("fista", "fista_mom"):
        x = i0 - LINV * g
        if nonneg:
            x = np.where(x < 0, F32(0), x)
        return (x,) if form == "fista" else (x, x + BETA * (x - i1))
    ga = RHO * ((i0 - i2) + i1)
    z = i0 - TAU * (g + ga)
    if nonneg:
        z = np.where(z < 0, F32(0), z)
    if relax_on:
        z = OMA * i0 + ALPHA * z
    return z, z + i1


def on_device(arr, misaligned, made):
    """A device copy of `arr` inside guard bands (tests/_guarded.py); misaligned: 4 bytes off 16-byte alignment (shift=1).
    The guarded object joins `made`, whose bands the test checks at its end."""
    g = guarded(arr, shift=1 if misaligned else 0)
    assert (g.view.data_ptr() % 16 != 0) == misaligned
    made.append(g)
    return g.view


def quad_interleaved(r):
    """[nz][na][nu] -> the private residual layout [ceil(nz/4)][na][nu][4], zero padding slices."""
    nz, na, nu = r.shape
    nq = (nz + 3) // 4
    pad = np.zeros((4 * nq, na, nu), np.float32)
    pad[:nz] = r
    return np.ascontiguousarray(pad.reshape(nq, 4, na, nu).transpose(0, 2, 3, 1))


# nz, n, nu, every volume array misaligned
SHAPES = {"whole+ragged-z": (17, 64, 71, False), "whole-misaligned": (17, 64, 71, True), "ragged-only": (5, 37, 45, False)}
# ... per back projector, in the planar residual layout; the voxel-driven one reads the quad-interleaved residual too (the
# matched one does not), so its first shape runs under both layouts
CASES = [pytest.param(adj, *shape, "planar", id=f"{adj}-{name}") for adj in ("unmatched", "matched") for name, shape in SHAPES.items()]
CASES.append(pytest.param("unmatched", *SHAPES["whole+ragged-z"], "zquad", id="unmatched-whole+ragged-z-zquad-residual"))


@pytest.mark.parametrize("adjoint,nz,n,nu,misaligned,layout", CASES)
def test_fused_epilogues_equal_one_restatement(adjoint, nz, n, nu, misaligned, layout):
    from tomobar_amd.projector import HipTools3D
    H = HipTools3D(nu, 0, nz, np.linspace(0.1, np.pi + 0.1, NA, endpoint=False), 0.4, n, "gpu", 0, None, adjoint=adjoint)
    rng = np.random.default_rng(21)
    r = rng.standard_normal((nz, NA, nu)).astype(np.float32)
    x, xo, u = (rng.standard_normal((nz, n, n)).astype(np.float32) * F32(s) for s in (0.05, 0.05, 0.01))
    g = host(H.backward(torch.from_numpy(r).cuda()))     # the same kernel's plain epilogue: the same accumulation
    assert H.kernel_path("bp").startswith("matched" if adjoint == "matched" else "brick")
    assert np.abs(g).max() > 0
    H.set_residual_layout(layout)
    assert H.residual_layout() == layout
    res = torch.from_numpy(quad_interleaved(r) if layout == "zquad" else r).cuda()
    made = []
    dev = lambda a: on_device(a, misaligned, made)
    blank = lambda: on_device(np.full((nz, n, n), np.nan, np.float32), misaligned, made)
    try:
        for nonneg in (False, True):
            (X,) = restate("fista", g, x, nonneg=nonneg)
            assert (X < 0).any() != nonneg and (X > 0).any()
            out = blank()
            H.grad_step(res, dev(x), out, LINV, nonneg, None)
            assert np.array_equal(host(out), X)
            X, Xt = restate("fista_mom", g, x, xo, nonneg=nonneg)
            xt_d, xo_d = dev(x), dev(xo)
            H.grad_step_momentum(res, xt_d, xo_d, LINV, BETA, nonneg, None)
            assert np.array_equal(host(xo_d), X)
            assert np.array_equal(host(xt_d), Xt)
            for relax_on in (False, True):
                Z, ZU = restate("admm", g, x, u, xo, nonneg=nonneg, relax_on=relax_on)
                z_d, zu_d = dev(x), blank()
                H.admm_z_update(res, z_d, dev(xo), dev(u), zu_d, TAU, RHO, relax_on, OMA, ALPHA, nonneg, None)
                assert np.array_equal(host(z_d), Z), (nonneg, relax_on)
                assert np.array_equal(host(zu_d), ZU), (nonneg, relax_on)
        assert H.kernel_path("bp").startswith("matched" if adjoint == "matched" else "brick")
        for k, g in enumerate(made):
            g.check((adjoint, layout, "volume array", k))
    finally:
        H.set_residual_layout("planar")


@pytest.mark.parametrize("n", [30, 33])   # not multiples of 4: the 32 x 32 dword kernel; inside one tile, into a second
def test_folded_momentum_transpose_kernel(n):
    """momentum_transpose_kernel<true> writes X_t and the transposed token; <false> is the forward projector's own transpose.
    8 angles over [0, pi): some step along x, so the forward projection reads the transposed copy."""
    from tomobar_amd.projector import HipTools3D
    nz, beta = 2, F32(0.7391357421875)
    H = HipTools3D(n + 5, 0, nz, np.linspace(0.0, np.pi, 8, endpoint=False), 0.0, n, "gpu", 0, None)
    rng = np.random.default_rng(22)
    x, xold = (rng.standard_normal((nz, n, n)).astype(np.float32) for _ in range(2))
    xt = torch.full((nz, n, n), float("nan"), device="cuda")
    H.momentum(torch.from_numpy(x).cuda(), torch.from_numpy(xold).cuda(), xt, beta)
    assert np.array_equal(host(xt), x + beta * (x - xold))
    with_token = host(H.forward(xt))            # uses the token momentum left
    fresh = host(H.forward(xt.clone()))         # another volume: a fresh transpose by the MOMENTUM = false instantiation
    assert np.abs(fresh).max() > 0
    assert np.array_equal(with_token, fresh)
