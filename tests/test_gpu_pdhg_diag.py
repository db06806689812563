"""MI355X tests of PDHG with the diagonal preconditioner: the step builder, the two launches that read their step from an
array and the driver against the float32 numpy restatement tests/_pdhg_diag_oracle.py, bit for bit (formula-level parity,
unpinned; docs/kernels/pdhg.md), on the inputs of tests/_pdhg_cases.py.  Every array a launch sees lies between guard bands."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from _gpu_compare import host, same_bits  # noqa: E402
from _guarded import guarded  # noqa: E402
import _pdhg_cases as K  # noqa: E402
import _pdhg_diag_oracle as D  # noqa: E402
import _pdhg_oracle as P  # noqa: E402

F = np.float32


# ------------------------------------------------------------------------------------------------ the steps and step 2
SINO_EXTENTS = [(1,), (3,), (63,), (64,), (65,), (4099,), (5, 23, 48)]
NUMER = F(0.95)


def _sino_inputs(shape):
    rng = np.random.default_rng(41)
    y = (2.0 * rng.standard_normal(shape)).astype(np.float32)      # reaches beyond +-1: the L1 clip
    r = rng.uniform(-1.0, 9.0, shape).astype(np.float32)
    b = rng.uniform(-2.0, 8.0, shape).astype(np.float32)           # negative entries: the KL clamp
    return y, r, b


def _row_sums(shape):
    """what the step builder reads: zeros on about a sixth of the samples (the guard), elsewhere the sums that give steps
    of 1e-3 ... 1e3, log-uniform"""
    rng = np.random.default_rng(42)
    sums = (NUMER / 10.0 ** rng.uniform(-3.0, 3.0, shape)).astype(np.float32)
    sums[rng.random(shape) < 1.0 / 6.0] = 0.0
    return sums


@pytest.mark.parametrize("shape", SINO_EXTENTS, ids=lambda s: "x".join(map(str, s)))
def test_step_builder_equals_the_oracle(shape):
    from tomobar_amd import ops
    sums = _row_sums(shape)
    big = sums.size > 8
    for numer, add in ((NUMER, F(0)), (F(0.95) / F(4), F(6))):
        want = D.diag_steps(sums, numer, add)
        assert want.dtype == np.float32 and np.isfinite(want).all()
        if big and add == 0:   # conditions on the input: the guard acts, and the steps span five decades
            assert (want == numer * F(1024)).any() and want.min() < 1e-2 and want[want < 900].max() > 1e2
        sg, og = guarded(sums), guarded(shape)
        assert ops.pdhg_diag_steps(og.view, sg.view, numer, add) is og.view
        same_bits(host(og.view), want, (shape, float(add), "out of place"))
        assert sg.intact() and og.intact() and sg.unchanged()
        assert ops.pdhg_diag_steps(sg.view, sg.view, numer, add) is sg.view      # out == in
        same_bits(host(sg.view), want, (shape, float(add), "in place"))
        assert sg.intact()


@pytest.mark.parametrize("fidelity", P.FIDELITIES)
@pytest.mark.parametrize("shape", SINO_EXTENTS, ids=lambda s: "x".join(map(str, s)))
def test_sino_dual_diag_equals_the_oracle(shape, fidelity):
    from tomobar_amd import ops
    y, r, b = _sino_inputs(shape)
    sigma = D.diag_steps(_row_sums(shape), NUMER)
    want = D.sino_dual(y, r, b, fidelity, sigma)
    assert want.dtype == np.float32
    if y.size > 8:
        assert (sigma == NUMER * F(1024)).any() and (sigma < 1e-2).any()
        if fidelity == "L1":
            assert (want == 1).any() and (want == -1).any() and (np.abs(want) < 1).any()
    yg, rg, bg, sg = guarded(y), guarded(r), guarded(b), guarded(sigma)
    assert ops.pdhg_sino_dual_diag(yg.view, rg.view, bg.view, sg.view, fidelity) is yg.view
    same_bits(host(yg.view), want, (shape, fidelity))
    assert all(g.intact() for g in (yg, rg, bg, sg)) and rg.unchanged() and bg.unchanged() and sg.unchanged()
    # two applications: the dual is really updated in place
    ops.pdhg_sino_dual_diag(yg.view, rg.view, bg.view, sg.view, fidelity)
    same_bits(host(yg.view), D.sino_dual(want, r, b, fidelity, sigma), (shape, fidelity, "second application"))
    assert all(g.intact() for g in (yg, rg, bg, sg)) and sg.unchanged()


@pytest.mark.parametrize("shifts", [(1, 1, 1, 1), (0, 0, 0, 1), (0, 3, 0, 0)], ids=["all", "sigma only", "r only"])
@pytest.mark.parametrize("fidelity", P.FIDELITIES)
def test_streams_on_arrays_that_are_not_16_byte_aligned(fidelity, shifts):
    """the scalar form: arrays that start 4 k bytes past a 16-byte boundary -- all four, or the step array alone"""
    from tomobar_amd import ops
    y, r, b = _sino_inputs((4100,))
    sums = _row_sums((4100,))
    sigma = D.diag_steps(sums, NUMER)
    yg, rg, bg, sg = (guarded(a, shift=k) for a, k in zip((y, r, b, sigma), shifts))
    assert [g.view.data_ptr() % 16 for g in (yg, rg, bg, sg)] == [4 * k for k in shifts]
    ops.pdhg_sino_dual_diag(yg.view, rg.view, bg.view, sg.view, fidelity)
    same_bits(host(yg.view), D.sino_dual(y, r, b, fidelity, sigma), (fidelity, shifts))
    assert all(g.intact() for g in (yg, rg, bg, sg)) and rg.unchanged() and bg.unchanged() and sg.unchanged()
    ug, og = guarded(sums, shift=shifts[3]), guarded((4100,), shift=shifts[0])
    ops.pdhg_diag_steps(og.view, ug.view, NUMER)
    same_bits(host(og.view), sigma, ("steps", shifts))
    assert ug.intact() and og.intact() and ug.unchanged()


def test_streams_refuse_what_they_cannot_run():
    from tomobar_amd import _lib, ops
    y, r, b, s = (torch.full((8,), float(k), device="cuda") for k in range(4))
    keep = [t.clone() for t in (y, r, b, s)]
    with pytest.raises(ValueError, match="LS, L1 and KL"):
        ops.pdhg_sino_dual_diag(y, r, b, s, "PWLS")
    with pytest.raises(ValueError):
        ops.pdhg_sino_dual_diag(y, r, b, s[:4], "LS")
    for args in ((y, y, b, s), (y, r, y, s), (y, r, b, y)):
        with pytest.raises(ValueError, match="alias"):
            ops.pdhg_sino_dual_diag(*args, "LS")
    lib = _lib.lib()
    nul = C.c_void_p(0)
    p = [C.c_void_p(t.data_ptr()) for t in (y, r, b, s)]
    for args in ((nul, p[1], p[2], p[3]), (p[0], p[1], p[2], nul)):
        with pytest.raises(ValueError, match="NULL"):
            _lib.check(lib.tomo_pdhg_sino_dual_diag(*args, 8, 0, None))
    with pytest.raises(ValueError, match="data term"):
        _lib.check(lib.tomo_pdhg_sino_dual_diag(*p, 8, 7, None))
    with pytest.raises(ValueError, match="numerator"):
        ops.pdhg_diag_steps(y, s, 0.0)
    with pytest.raises(ValueError, match="NULL"):
        _lib.check(lib.tomo_pdhg_diag_steps(nul, p[3], 8, 0.95, 0.0, None))
    with pytest.raises(ValueError):
        ops.pdhg_diag_steps(y, s[:4], 0.95)
    torch.cuda.synchronize()
    assert all(torch.equal(t, k) for t, k in zip((y, r, b, s), keep)), "a refused call launched"


# ------------------------------------------------------------------------------------------------ steps 4 and 5
T_NUMER = F(0.95)


def _tau_field(shape, tv):
    """a seeded field spanning 0.05 ... 0.5, and in the first corner the step of a voxel no ray meets (C = 0)"""
    nd = 3 if shape[0] > 1 else 2
    tau = np.random.default_rng(10).uniform(0.05, 0.5, shape).astype(np.float32)
    corner = D.diag_steps(np.zeros((1,), np.float32), T_NUMER, F(2 * nd) if tv else F(0))[0]
    tau.flat[-2:] = 0.05, 0.5
    tau[:1, :2, :2] = corner
    assert corner == (T_NUMER / F(2 * nd) if tv else T_NUMER * F(1024))
    return tau


@pytest.mark.parametrize("shape", K.MARCH_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_primal_diag_equals_the_oracle(shape):
    from tomobar_amd import ops
    g_host = K.march_g(shape)
    gg, tg = guarded(g_host), guarded(_tau_field(shape, True))
    nd = 3 if shape[0] > 1 else 2
    for kind in ("noise", "terraces"):
        x0 = K.march_input(kind, shape)
        lam = K.MARCH_LAMBDA[kind]
        for methodTV in (0, 1):
            for nonneg in (0, 1):
                want = D.march_steps(x0, g_host, K.MARCH_SIGMA, tg.host(), lam, methodTV, nonneg, K.MARCH_COUNTS)
                xg, bg = guarded(x0), guarded(x0)
                x, xbar = xg.view, bg.view
                qs = [guarded(np.zeros(shape, np.float32)) for _ in range(nd)]
                q = [b.view for b in qs]
                for n in range(1, max(K.MARCH_COUNTS) + 1):
                    ops.pdhg_tv_dual(xbar, q, K.MARCH_SIGMA, lam, methodTV)
                    ops.pdhg_primal_diag(x, xbar, gg.view, q, tg.view, nonneg)
                    if n in K.MARCH_COUNTS:
                        what = (shape, kind, methodTV, nonneg, n)
                        wx, wb, wq = want[n]
                        same_bits(host(x), wx, what + ("x",))
                        same_bits(host(xbar), wb, what + ("x-bar",))
                        for d in range(nd):
                            same_bits(host(q[d]), wq[d], what + (f"q{d + 1}",))
                assert all(b.intact() for b in [xg, bg, gg, tg] + qs), (shape, kind, "a guard was written")
                assert gg.unchanged() and tg.unchanged(), "g or tau was written"
    # without the TV block: div q = 0, and the corner takes the guarded step 0.95 * 1024
    tg = guarded(_tau_field(shape, False))
    x0 = K.march_input("noise", shape) - np.float32(0.4)
    for nonneg in (0, 1):
        want = D.march_steps(x0, g_host, K.MARCH_SIGMA, tg.host(), None, 0, nonneg, (3,))[3]
        assert np.isfinite(want[0]).all()
        xg, bg = guarded(x0), guarded(x0)
        x, xbar = xg.view, bg.view
        for _ in range(3):
            ops.pdhg_primal_diag(x, xbar, gg.view, [], tg.view, nonneg)
        same_bits(host(x), want[0], (shape, "no TV", nonneg, "x"))
        same_bits(host(xbar), want[1], (shape, "no TV", nonneg, "x-bar"))
        assert xg.intact() and bg.intact() and gg.intact() and tg.intact() and gg.unchanged() and tg.unchanged()


def test_primal_diag_refuses_what_it_cannot_run():
    from tomobar_amd import _lib, ops
    x, xbar, g, tau, q1, q2, q3 = (torch.full((3, 4, 5), float(k), device="cuda") for k in range(7))
    keep = [t.clone() for t in (x, xbar)]
    for args in ((x, x, g, [q1, q2, q3], tau), (x, xbar, g, [q1, q2, q3], x), (x, xbar, g, [q1, q2, q3], xbar),
                 (x, xbar, g, [q1, q2, q3], g), (x, xbar, g, [q1, q2, x], tau)):
        with pytest.raises(ValueError, match="alias"):
            ops.pdhg_primal_diag(*args)
    with pytest.raises(ValueError, match="shape"):
        ops.pdhg_primal_diag(x, xbar, g, [], tau[:2])
    with pytest.raises(ValueError, match="3 dual fields"):
        ops.pdhg_primal_diag(x, xbar, g, [q1, q2], tau)
    p = [C.c_void_p(t.data_ptr()) for t in (x, xbar, g, tau, q1, q2, q3)]
    p[3] = C.c_void_p(0)
    with pytest.raises(ValueError, match="NULL"):
        _lib.check(_lib.lib().tomo_pdhg_primal_diag(0, *p, 5, 4, 3, 3, 0, None))
    torch.cuda.synchronize()
    assert all(torch.equal(t, k) for t, k in zip((x, xbar), keep)), "a refused call launched"


def test_tau_is_one_more_work_array_behind_the_others():
    from tomobar_amd import _lib, ops
    shape = (5, 13, 37)
    xbar, g, q, tau, lease = ops.pdhg_work_arrays(shape, "cuda:0", True, tau=True)
    arrs = [xbar, g] + q + [tau]
    assert len(q) == 3 and all(tuple(a.shape) == shape and a.dtype == torch.float32 and a.is_contiguous() for a in arrs)
    step = (5 * 13 * 37 * 4 + 255) // 256 * 256 + ops.ARRAY_SKEW
    assert [a.data_ptr() - xbar.data_ptr() for a in arrs] == [k * step for k in range(6)] and xbar.data_ptr() % 256 == 0
    assert _lib.lib().tomo_pdhg_diag_scratch_bytes(37, 13, 5, 3) == 6 * step
    assert _lib.lib().tomo_pdhg_scratch_bytes(37, 13, 5, 3) == 5 * step
    assert ops.lease_is_current(lease)
    assert len(ops.pdhg_work_arrays(shape, "cuda:0", True)) == 4          # the default call is what it was
    xbar2, g2, q2, tau2, _ = ops.pdhg_work_arrays(shape, "cuda:0", False, tau=True)
    assert q2 == [] and tau2.data_ptr() - xbar2.data_ptr() == 2 * step


# ------------------------------------------------------------------------------------------------ the driver
LABELS = ["detY", "angles", "detX"]
ITERS = 12


def _tools(nz):
    from tomobar_amd.methodsIR_CuPy import RecToolsIRCuPy
    return RecToolsIRCuPy(K.N, 0, nz if nz > 1 else None, 0.0, K.ANGLES, K.N, 0, None, adjoint="matched")


def _reg(kw):
    return None if kw["lam"] is None else {"method": "PD_TV", "regul_param": kw["lam"], "methodTV": kw.get("methodTV", 0)}


# name -> (the case of _pdhg_cases.CASES, planes, PDHG_ratio)
DRIVER_CASES = {"LS+TV": ("LS+TV", K.NZ, 1.0), "L1+TV": ("L1+TV", K.NZ, 1.0), "KL+TV": ("KL+TV", K.NZ, 1.0), "LS": ("LS", K.NZ, 1.0),
                "2D KL+TV": ("KL+TV", 1, 1.0), "L1+TV ratio 4": ("L1+TV", K.NZ, 4.0)}


@pytest.mark.parametrize("name", list(DRIVER_CASES))
def test_driver_equals_the_oracle_loop(name, monkeypatch):
    from tomobar_amd import ops
    case, nz, ratio = DRIVER_CASES[name]
    kw, positive = K.CASES[case]
    b = K.sinogram(nz, positive=positive)
    state = {}
    want = D.pdhg(K.matched(nz), b, ITERS, ratio=ratio, state=state, **kw)
    assert np.abs(want).max() > 0 and want.dtype == np.float32

    seen = {}
    real = ops.pdhg_sino_dual_diag

    def recording(y, r, b_dev, sigma, fidelity):
        seen.update(y=y, sigma=sigma)
        return real(y, r, b_dev, sigma, fidelity)

    monkeypatch.setattr(ops, "pdhg_sino_dual_diag", recording)
    rt = _tools(nz)
    data = guarded(np.asarray(b))
    algo = {"iterations": ITERS, "PDHG_preconditioner": "diagonal", "PDHG_ratio": ratio, "nonnegativity": kw.get("nonneg", False),
            "recon_mask_radius": None}
    got = rt.PDHG({"projection_data": data.view, "data_axes_labels_order": list(LABELS), "data_fidelity": kw["fidelity"]}, algo,
                  _reg(kw))
    assert isinstance(got, torch.Tensor) and tuple(got.shape) == (nz, K.N, K.N)
    assert "lipschitz_const" not in algo and rt.Atools.kernel_path("bp").startswith("matched")
    run = rt.last_run
    assert (run["method"], run["iterations_done"], run["converged"], run["preconditioner"]) == ("PDHG", ITERS, False, "diagonal")
    same_bits(host(got), want, (name, "x"))
    assert data.intact() and data.unchanged(), "the caller's projection data must not be written"
    # the rest of the state: the steps and y through the launch the driver made, x-bar, q and tau through the placed block
    same_bits(host(seen["sigma"]), state["sigma"], (name, "sigma"))
    same_bits(host(seen["y"]), state["y"], (name, "y"))
    tv = kw["lam"] is not None
    xbar, _, q, tau, _ = ops.pdhg_work_arrays((nz, K.N, K.N), "cuda:0", tv, tau=True)
    same_bits(host(xbar), state["xbar"], (name, "x-bar"))
    same_bits(host(tau), state["tau"], (name, "tau"))
    assert len(q) == len(state["q"])
    for d, field in enumerate(q):
        same_bits(host(field), state["q"][d], (name, f"q{d + 1}"))


def test_without_the_key_the_driver_is_the_scalar_one():
    """the default path did not move: the run tests/test_gpu_pdhg.py pins, on this geometry"""
    kw, positive = K.CASES["LS+TV"]
    b = K.sinogram(positive=positive)
    want = P.pdhg(K.matched(), b, K.lipschitz(), ITERS, **kw)
    for extra in ({}, {"PDHG_preconditioner": None}):
        rt = _tools(K.NZ)
        algo = dict({"iterations": ITERS, "lipschitz_const": K.lipschitz(), "recon_mask_radius": None}, **extra)
        got = rt.PDHG({"projection_data": torch.from_numpy(np.array(b)).cuda(), "data_axes_labels_order": list(LABELS)}, algo, _reg(kw))
        same_bits(host(got), want, ("scalar steps", tuple(extra)))
        assert rt.last_run["preconditioner"] is None and algo["PDHG_preconditioner"] is None


def test_refusals_on_a_real_object():
    rt = _tools(K.NZ)
    data = {"projection_data": torch.from_numpy(np.array(K.sinogram())).cuda(), "data_axes_labels_order": list(LABELS)}
    with pytest.raises(ValueError, match="PDHG_preconditioner"):
        rt.PDHG(dict(data), {"iterations": 2, "PDHG_preconditioner": "jacobi"})
    from tomobar_amd.methodsIR_CuPy import RecToolsIRCuPy
    sp = RecToolsIRCuPy(K.N, 0, K.NZ, 0.0, K.ANGLES, K.N, 0, 4, adjoint="matched")
    with pytest.raises(ValueError, match="PDHG only"):
        sp.SPDHG(dict(data), {"iterations": 2, "lipschitz_const": 100.0, "PDHG_preconditioner": "diagonal"})
    # the object still reconstructs afterwards
    out = rt.PDHG(dict(data), {"iterations": 2, "PDHG_preconditioner": "diagonal"}, {"method": "PD_TV", "regul_param": 0.5})
    assert np.isfinite(host(out)).all()
