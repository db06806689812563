"""MI355X: the matched back projector (tomobar_amd/csrc/bp_matched.hip, docs/kernels/bp_matched.md) against the numpy
restatement of its specification (tests/_matched_bp_oracle.py), bit for bit, from the C-ABI up to the drivers.

The kernel works on bricks of BX x BY x BZ = 32 x 16 x 16 voxels and stages the sinogram in batches of AB = 8 angles;
the edge shapes below are derived from these four numbers."""
import numpy as np
import pytest

import _matched_bp_oracle as M

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

BX, BY, BZ, AB = 32, 16, 16, 8
EXTRA_ANGLES = np.linspace(0.17, 6.1, 2 * AB + 1)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def angle_set(na):
    """`na` angles: the special ones first (0, the tie pi/4, pi/2, 3pi/4, pi, -0.3, 5.5), then a spread over (0, 2pi); a
    single angle is the tie."""
    if na == 1:
        return np.array([np.pi / 4])
    return np.concatenate([np.asarray(M.SPECIAL_ANGLES), EXTRA_ANGLES])[:na]


def make_pair(nz, n, nu, angles, cor, os_n=1, adjoint="matched"):
    from tomobar_amd.projector import HipTools3D
    P = M.MatchedProjector(nz, n, nu, angles, cor, os_n)
    H = HipTools3D(nu, 0, nz, angles, cor, n, "gpu", 0, os_n if os_n > 1 else None, adjoint=adjoint)
    return P, H


# (n, nz, nu - n, cor, angles per subset / na, OS): every value the kernel treats differently appears at least once --
#   n one below / on / one above BY and BX, and 2 BX + 1 (a second, partial brick in x; five in y);
#   nz 1, 3, 4, 5 (around a z-quad) and BZ + 1 (a second, ragged z-brick);
#   nu = n - 5, n, n + 7 (taps falling off either detector end); CoR 0, 0.4, -2.75 and a per-angle vector;
#   subset sizes 1, AB - 1, AB, AB + 1, 2 AB + 1 (no batch, a short one, a whole one, a tail of one, two and a tail);
#   OS_number 3 with 10 angles: subsets of 4, 3 and 3 angles after the one-element trim.
PLAIN_CASES = [
    (BY - 1, 1, 0, 0.0, 1, 1),
    (BY, 3, -5, 0.4, AB - 1, 1),
    (BY + 1, 4, 7, -2.75, AB, 1),
    (BX - 1, 5, -5, "vec", AB + 1, 1),
    (BX, BZ + 1, 0, 0.4, 2 * AB + 1, 1),
    (BX + 1, 3, 7, 0.0, AB, 1),
    (2 * BX + 1, 5, -5, -2.75, AB + 1, 1),
    (2 * BX + 1, BZ + 1, 7, "vec", 2 * AB + 1, 1),
    (BX + 1, 4, 0, 0.4, 10, 3),
    (3, 1, 7, -2.75, AB - 1, 1),
]


@pytest.mark.parametrize("case", PLAIN_CASES, ids=lambda c: "n{}-nz{}-du{}-cor{}-na{}-os{}".format(*c))
def test_backward_is_the_restatement_bit_for_bit(case):
    n, nz, du, cor, na, os_n = case
    nu = n + du
    angles = angle_set(na)
    if isinstance(cor, str):
        cor = np.linspace(-1.5, 2.0, na)
    P, H = make_pair(nz, n, nu, angles, cor, os_n)
    assert H.adjoint == "matched"
    rng = np.random.default_rng(11)
    for s in ([None] if os_n == 1 else list(range(os_n))):
        nsel = H.subset_size(s)
        assert nsel == (na if s is None else len(P.subsets[s]))
        noise = rng.standard_normal((nz, nsel, nu)).astype(np.float32)
        got = host(H.backward(dev(noise), s))
        assert H.kernel_path("bp").startswith("matched")
        assert np.array_equal(got, P.bp(noise, s)), (case, s, float(np.abs(got - P.bp(noise, s)).max()))
        assert np.array_equal(host(H._backprojCuPy(dev(noise)) if s is None else H._backprojOSCuPy(dev(noise), s)), got)
        # one detector pixel of one angle lit in every slice: the result IS the weights themselves.  The pixel the central
        # voxel's first tap falls on (lit voxels exist whenever it is on the detector), and the two end pixels
        tab = M.table_of(P, s)
        mid = int(M.taps32(n, nu, tab, nsel - 1)[0][n // 2, n // 2])
        for a, iu in ((nsel - 1, min(max(mid, 0), nu - 1)), (0, 0), (nsel // 2, nu - 1)):
            one = np.zeros((nz, nsel, nu), np.float32)
            one[:, a, iu] = 1.0
            want = P.bp(one, s)
            assert want.max() > 0 or iu != mid
            assert np.array_equal(host(H.backward(dev(one), s)), want), (case, s, a, iu)


FUSED_GEOMS = [
    # nz, n, nu, na, cor, os
    (BZ + 1, 2 * BX, 2 * BX + 7, 19, 0.4, 2),   # whole bricks (dwordx4 epilogue through LDS) and a ragged z-brick (scalar epilogue)
    (5, 37, 45, AB + 1, -2.75, 1),              # odd sizes: the scalar epilogue alone
]


@pytest.mark.parametrize("g", FUSED_GEOMS)
def test_fused_gradient_steps(g):
    """The three fused forms: the restated gradient pushed through the oracle's epilogue arithmetic (numpy float32, one
    rounding per operation, as tests/test_gpu_parity.py::test_fused_residual_and_gradient_steps does for the shipped one);
    both nonneg settings, relaxation on and off, and x_out aliasing x_t."""
    nz, n, nu, na, cor, os_n = g
    P, H = make_pair(nz, n, nu, angle_set(na), cor, os_n)
    rng = np.random.default_rng(3)
    x = rng.random((nz, n, n)).astype(np.float32) * 0.05
    xo = rng.random((nz, n, n)).astype(np.float32) * 0.05
    u = rng.standard_normal((nz, n, n)).astype(np.float32) * 0.01
    linv, beta = np.float32(1 / 300.0), np.float32(0.37)
    tau, rho, al = np.float32(0.002), np.float32(1.7), 1.6
    for s in ([None] if os_n == 1 else list(range(os_n))):
        r = rng.standard_normal((nz, H.subset_size(s), nu)).astype(np.float32)
        grad = P.bp(r, s)
        for nonneg in (False, True):
            X = x - linv * grad
            if nonneg:
                X = np.maximum(X, 0)
            out = torch.empty_like(dev(x))
            H.grad_step(dev(r), dev(x), out, linv, nonneg, s)
            assert H.kernel_path("bp").startswith("matched")
            assert np.array_equal(host(out), X)
            alias = dev(x)
            H.grad_step(dev(r), alias, alias, linv, nonneg, s)       # x_out aliases x_t
            assert np.array_equal(host(alias), X)
            xt_d, xo_d = dev(x), dev(xo)
            H.grad_step_momentum(dev(r), xt_d, xo_d, linv, beta, nonneg, s)
            assert np.array_equal(host(xo_d), X)
            assert np.array_equal(host(xt_d), X + beta * (X - xo))
            for relax_on in (False, True):
                z = x.copy()
                zn = z - tau * (grad + rho * (z - xo + u))
                if nonneg:
                    zn = np.maximum(zn, 0)
                if relax_on:
                    zn = np.float32(1.0 - al) * z + np.float32(al) * zn
                z_d, zu_d = dev(x), torch.empty_like(dev(x))
                H.admm_z_update(dev(r), z_d, dev(xo), dev(u), zu_d, tau, rho, relax_on, np.float32(1.0 - al), np.float32(al), nonneg, s)
                assert np.array_equal(host(z_d), zn)
                assert np.array_equal(host(zu_d), zn + u)


def test_adjoint_gap_on_the_shipped_forward_projector():
    """<Ax, y> against <x, A^T y> with tomo_fp3d and the new kernel at 48 x 48 x 5, nu = 52, 23 angles, white noise:
    normalised gap <= 2e-6; the unmatched `backward` on the same arrays >= 2e-5."""
    nz, n, nu, na = 5, 48, 52, 23
    P, H = make_pair(nz, n, nu, np.linspace(0.0, np.pi, na, endpoint=False), 0.4)
    rng = np.random.default_rng(8)
    x = rng.standard_normal((nz, n, n)).astype(np.float32)
    y = rng.standard_normal((nz, na, nu)).astype(np.float32)
    ax = host(H.forward(dev(x)))
    gm = M.normalised_gap(ax, y, x, host(H.backward(dev(y))))
    H.adjoint = "unmatched"
    gu = M.normalised_gap(ax, y, x, host(H.backward(dev(y))))
    assert H.kernel_path("bp").startswith("brick")
    print(f"normalised gap on the GPU pair: matched {gm:.3e}, unmatched {gu:.3e}")
    assert gm <= 2e-6, gm
    assert gu >= 2e-5, gu


def test_slice_independence():
    """The operator is per slice: planes 2 .. 6 of a 9-plane sinogram back project to planes 2 .. 6 of the whole result."""
    n, nu, na = 40, 44, 11
    angles = angle_set(na)
    _, H9 = make_pair(9, n, nu, angles, 0.4)
    _, H5 = make_pair(5, n, nu, angles, 0.4)
    y = np.random.default_rng(9).standard_normal((9, na, nu)).astype(np.float32)
    assert np.array_equal(host(H5.backward(dev(y[2:7]))), host(H9.backward(dev(y)))[2:7])


def test_default_objects_are_untouched(oracle):
    """With the keyword absent `backward` is the oracle's (voxel-driven) back projection, as before; the switch can be set
    and set back on a live object, and its refusals hold there too."""
    from tomobar_amd.projector import HipTools3D
    nz, n, nu, na = 5, 37, 45, 19
    angles = angle_set(na)
    P = oracle.Projector(nz, n, nu, angles, 1.25)
    H = HipTools3D(nu, 0, nz, angles, 1.25, n, "gpu", 0, None)
    assert H.adjoint == "unmatched"
    y = np.random.default_rng(10).standard_normal((nz, na, nu)).astype(np.float32)
    assert np.array_equal(host(H.backward(dev(y))), P.bp(y))
    assert H.kernel_path("bp").startswith("brick")
    H.adjoint = "matched"
    assert np.array_equal(host(H.backward(dev(y))), M.bp32(y, n, M.angle_table(angles, 1.25)))
    assert np.array_equal(host(H.backward(dev(y), adjoint="unmatched")), P.bp(y))
    H.set_residual_layout("zquad")                      # keeps the planar layout while the adjoint is matched
    assert H.residual_layout() == "planar" and H.residual_buffer(None).dim() == 3
    with pytest.raises(ValueError, match="adjoint"):
        H.adjoint = "exact"
    assert H.adjoint == "matched"
    H.adjoint = "unmatched"
    assert np.array_equal(host(H.backward(dev(y))), P.bp(y))
    H.set_residual_layout("zquad")
    assert H.residual_layout() == "zquad"
    H.adjoint = "matched"                               # ... and setting it brings a quad-interleaved context back
    assert H.residual_layout() == "planar"
    H8 = HipTools3D(nu, 0, nz, angles, 1.25, n, "gpu", 0, None, lerp8=True)
    with pytest.raises(ValueError, match="lerp8"):
        H8.adjoint = "matched"
    assert H8.adjoint == "unmatched"
    # the C-ABI refuses on its own: a lerp8 context, and a context in the quad-interleaved layout
    from tomobar_amd import _lib, ops
    v, yd = torch.empty((nz, n, n), device="cuda"), dev(y)
    assert H8._lib.tomo_bp3d_matched(H8._ctx, -1, ops.ptr(yd), ops.ptr(v), ops.stream_ptr(v)) == _lib.E_INVALID
    assert b"LERP8" in H8._lib.tomo_last_error()
    H.adjoint = "unmatched"
    H.set_residual_layout("zquad")
    assert H._lib.tomo_bp3d_matched(H._ctx, -1, ops.ptr(yd), ops.ptr(v), ops.stream_ptr(v)) == _lib.E_INVALID
    assert b"planar" in H._lib.tomo_last_error()
    H.set_residual_layout("planar")


def test_fbp_keeps_the_voxel_driven_back_projector():
    from tomobar_amd.methodsDIR_CuPy import RecToolsDIRCuPy
    nz, n, na = 3, 40, 30
    angles = np.linspace(0, np.pi, na, endpoint=False)
    data = torch.from_numpy(np.random.default_rng(12).random((na, nz, n)).astype(np.float32)).cuda()
    out = {}
    for adj in ("unmatched", "matched"):
        rt = RecToolsDIRCuPy(n, 0, nz, 0.0, angles, n, device_projector=0, adjoint=adj)
        assert rt.adjoint == adj
        out[adj] = host(rt.FBP(data.clone(), data_axes_labels_order=["angles", "detY", "detX"]))
        assert rt.Atools.kernel_path("bp").startswith("brick")
        sino = data.transpose(0, 1).contiguous()
        bp = host(rt.BACKPROJ(sino))
        assert rt.Atools.kernel_path("bp").startswith("matched" if adj == "matched" else "brick")
        out["bp_" + adj] = bp
    assert np.array_equal(out["matched"], out["unmatched"])
    tab = M.angle_table(angles, 0.0)
    y = host(data.transpose(0, 1).contiguous())
    assert np.array_equal(out["bp_matched"], M.bp32(y, n, tab))
    assert np.array_equal(out["bp_unmatched"], M.bp32(y, n, tab, matched=False))


# ------------------------------------------------------------------------------------------ drivers
NZ, N, NA, LC = 3, 24, 16, 900.0
LABELS = ["detY", "angles", "detX"]


@pytest.fixture(scope="module")
def problem(oracle):
    """24 x 24 x 3 voxels, 16 angles: positive data (OSEM divides by it) projected from a seeded block phantom."""
    angles = np.linspace(0, np.pi, NA, endpoint=False)
    vol = np.zeros((NZ, N, N), np.float32)
    vol[:, 6:17, 8:19] = 1.0
    vol[1:, 9:13, 10:15] = 2.0
    P = oracle.Projector(NZ, N, N, angles)
    sino = (P.fp(vol) + np.float32(0.25)).astype(np.float32)
    sino.setflags(write=False)
    return dict(angles=angles, sino=sino)


def make_rt(problem, os_n=None, cor=0.0):
    from tomobar_amd.methodsIR_CuPy import RecToolsIRCuPy
    rt = RecToolsIRCuPy(N, 0, NZ, cor, problem["angles"], N, 0, os_n, adjoint="matched")
    assert rt.adjoint == "matched" and rt.Atools.adjoint == "matched"
    return rt, M.MatchedProjector(NZ, N, N, problem["angles"], cor, os_n or 1)


def data_dict(problem):
    return {"projection_data": torch.from_numpy(problem["sino"].copy()).cuda(), "data_axes_labels_order": list(LABELS)}


def test_landweber_sirt_cgls(problem):
    """The reference's loops (methodsIR_CuPy.py:128-309) retyped on the oracle forward projector and the restated A^T.
    Landweber and SIRT are element-wise around the two operators: bit-identical.  CGLS keeps the 1e-4 of
    tests/test_gpu_recon.py::test_simple_iterative_methods_vs_oracle: its step sizes come from inner products whose
    reduction order on the GPU (float64 partial sums per workgroup) is not numpy's."""
    sino = problem["sino"]
    rt, P = make_rt(problem)
    x = np.zeros((NZ, N, N), np.float32)
    for _ in range(5):
        x = x - np.float32(1e-3) * P.bp(P.fp(x) - sino)
    got = host(rt.Landweber(data_dict(problem), {"iterations": 5, "tau_step_lanweber": 1e-3, "recon_mask_radius": None}))
    assert rt.Atools.kernel_path("bp").startswith("matched")
    assert np.array_equal(got, x), float(np.abs(got - x).max())

    with np.errstate(divide="ignore"):
        R = np.nan_to_num(np.float32(1) / P.fp(np.ones((NZ, N, N), np.float32)), nan=1.0, posinf=1.0, neginf=1.0)
        Cm = np.nan_to_num(np.float32(1) / P.bp(np.ones_like(sino)), nan=1.0, posinf=1.0, neginf=1.0)
    x = np.ones((NZ, N, N), np.float32)
    for _ in range(5):
        x = x + Cm * P.bp(R * (sino - P.fp(x)))
    got = host(rt.SIRT(data_dict(problem), {"iterations": 5, "recon_mask_radius": None}))
    assert np.array_equal(got, x), float(np.abs(got - x).max())

    x = np.zeros(NZ * N * N, np.float32)
    d = P.bp(sino).ravel()
    normr2 = np.inner(d, d)
    r = sino.ravel().copy()
    for _ in range(5):
        Ad = P.fp(d.reshape(NZ, N, N)).ravel()
        alpha = normr2 / np.inner(Ad, Ad)
        x = x + alpha * d
        r = r - alpha * Ad
        s = P.bp(r.reshape(sino.shape)).ravel()
        normr2_new = np.inner(s, s)
        d = s + (normr2_new / normr2) * d
        normr2 = normr2_new
    got = host(rt.CGLS(data_dict(problem), {"iterations": 5, "recon_mask_radius": None})).ravel()
    err = float(np.linalg.norm(got.astype(np.float64) - x) / np.linalg.norm(x.astype(np.float64)))
    print(f"CGLS(5), matched: rel-L2 vs the retyped loop {err:.3e}")
    assert err < 1e-4, err


@pytest.mark.parametrize("os_n", [None, 2])
def test_power_method(problem, os_n):
    """RecToolsIRCuPy.powermethod retyped (seeded start vector, 15 iterations, float64 sum of squares rounded to float32,
    multiplication by the float32 reciprocal): with a matched pair it returns the largest eigenvalue of A^T A."""
    rt, P = make_rt(problem, os_n)
    rt.power_seed = 5
    got = rt.powermethod({"projection_data": None})
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    x1 = host(torch.randn((NZ, N, N), dtype=torch.float32, device="cuda", generator=gen))
    sub = 0 if os_n else None
    y = P.fp(x1, sub)
    for _ in range(15):
        x1 = P.bp(y, sub)
        s = np.float32(np.sqrt(np.sum(x1.astype(np.float64) ** 2)))
        x1 = (np.float32(1.0) / s) * x1
        y = P.fp(x1, sub)
    assert got == float(s), (got, float(s))


def test_fista_os_pdtv_exact(problem, oracle):
    rt, P = make_rt(problem, 2)
    reg = {"method": "PD_TV", "regul_param": 0.002, "iterations": 9, "methodTV": 0, "PD_LipschitzConstant": 12.0}
    want = oracle.fista(P, problem["sino"], 3, LC, True, reg)
    got = host(rt.FISTA(data_dict(problem), {"iterations": 3, "lipschitz_const": LC, "nonnegativity": True, "recon_mask_radius": None},
                        {"method": "PD_TV", "regul_param": 0.002, "iterations": 9, "exact_roundings": True}))
    assert rt.Atools.kernel_path("bp").startswith("matched") and rt.Atools.residual_layout() == "planar"
    assert np.array_equal(got, want), float(np.abs(got - want).max())
    # ... and without a proximal step: the fused gradient + momentum epilogue
    want = oracle.fista(P, problem["sino"], 3, LC, False, None)
    got = host(rt.FISTA(data_dict(problem), {"iterations": 3, "lipschitz_const": LC, "recon_mask_radius": None}))
    assert np.array_equal(got, want), float(np.abs(got - want).max())


def test_admm_roftv_with_relaxation(problem, oracle):
    """Three outer iterations, so that the over-relaxation (from the third on) runs."""
    rt, P = make_rt(problem)
    reg = {"method": "ROF_TV", "regul_param": 0.004, "iterations": 8, "time_marching_step": 0.002}
    want = oracle.admm(P, problem["sino"], 3, LC, rho=2.0, relax=1.5, nonnegativity=True, reg=dict(reg))
    got = host(rt.ADMM(data_dict(problem), {"iterations": 3, "lipschitz_const": LC, "ADMM_rho_const": 2.0, "ADMM_relax_par": 1.5,
                                            "nonnegativity": True, "recon_mask_radius": None}, dict(reg)))
    assert rt.Atools.kernel_path("bp").startswith("matched")
    assert np.array_equal(got, want), float(np.abs(got - want).max())


def test_osem(problem, oracle):
    rt, P = make_rt(problem, 2)
    want = oracle.osem(P, problem["sino"], 3)
    got = host(rt.OSEM(data_dict(problem), {"iterations": 3, "recon_mask_radius": None}))
    assert rt.Atools.kernel_path("bp").startswith("matched")
    assert np.array_equal(got, want), float(np.abs(got - want).max())


def test_fista_with_a_vertical_cor_component(problem, oracle):
    """R(-shift) sits in front of either back projector: nothing new for the matched one."""
    cor = np.stack([np.linspace(-0.5, 0.75, NA), np.linspace(-0.6, 0.4, NA)], axis=1)
    rt, P = make_rt(problem, 2, cor)
    assert rt.Atools.has_vertical_shift and P.vshift is not None
    want = oracle.fista(P, problem["sino"], 2, LC, True, None)
    got = host(rt.FISTA(data_dict(problem), {"iterations": 2, "lipschitz_const": LC, "nonnegativity": True, "recon_mask_radius": None}))
    assert rt.Atools.kernel_path("bp").startswith("matched")
    assert np.array_equal(got, want), float(np.abs(got - want).max())
