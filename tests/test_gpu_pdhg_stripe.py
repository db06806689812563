"""MI355X tests of PDHG's stripe variable (``_data_["stripe_lambda"]``; docs/kernels/pdhg.md): the two stripe launches of
include/tomo_mi355x.h and the driver against the float32 numpy restatement tests/_pdhg_stripe_oracle.py, bit for bit (there
is no reference implementation: formula-level parity, unpinned), on the inputs of tests/_pdhg_stripe_cases.py and the
geometries of tests/_pdhg_driver_geometries.py; one case past 2^31 samples.  Both entry points run on a side stream behind a
delay in tests/test_gpu_streams.py (case "pdhg_stripe"): this file creates no stream."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _cupy_standin  # noqa: E402
from _gpu_compare import host, same_bits  # noqa: E402
from _guarded import guarded  # noqa: E402
import _large_index as LI  # noqa: E402
import _pdhg_driver_geometries as GEO  # noqa: E402
import _pdhg_oracle as P  # noqa: E402
import _pdhg_stripe_cases as SC  # noqa: E402
import _pdhg_stripe_oracle as S  # noqa: E402

F32 = np.float32


# ------------------------------------------------------------------------------------------------ the two launches
# (shift of y, r, b, sigma and s-bar; shift of the partial sums): all on 16-byte boundaries, all one float past one (the
# scalar path), and only the partial sums off (the 16-byte form needs every array)
SHIFTS = ((0, 0), (1, 1), (0, 1))


@pytest.mark.parametrize("nu", SC.KERNEL_NU)
@pytest.mark.parametrize("na", SC.KERNEL_NA)
def test_fused_dual_equals_the_oracle(na, nu):
    from tomobar_amd import ops
    for nz in SC.KERNEL_NZ:
        y0, r, b, sig, sbar = SC.kernel_inputs(nz, na, nu)
        assert (b < 0).any() or b.size < 8
        want = {(fid, per): S.sino_dual_stripe(y0, r, b, sbar, fid, sig if per else SC.KERNEL_SIGMA)
                for fid in P.FIDELITIES for per in (False, True)}
        if y0.size >= 64:   # a condition on the inputs: the L1 clip acts on a part of the samples
            assert 0.05 < np.mean(np.abs(want["L1", False][0]) == 1) < 0.95
        for shift, pshift in SHIFTS:
            rg, bg, sg, sbg = (guarded(a, shift=shift) for a in (r, b, sig, sbar))
            for (fid, per), (want_y, want_part) in want.items():
                yg, pg = guarded(y0, shift=shift), guarded(want_part.shape, shift=pshift)
                ops.pdhg_sino_dual_stripe(yg.view, rg.view, bg.view, sbg.view, pg.view, fid, sg.view if per else SC.KERNEL_SIGMA)
                what = (nz, na, nu, fid, "per sample" if per else "scalar", shift, pshift)
                same_bits(yg.host(), want_y, what + ("y",))
                same_bits(pg.host(), want_part, what + ("part",))
                assert yg.intact() and pg.intact(), (what, "a guard was written")
            for g in (rg, bg, sg, sbg):
                g.check((nz, na, nu, shift), read_only=True)


@pytest.mark.parametrize("nu", SC.KERNEL_NU)
@pytest.mark.parametrize("na", SC.KERNEL_NA)
def test_stripe_update_equals_the_oracle(na, nu):
    from tomobar_amd import ops
    rng = np.random.default_rng([7, na, nu])
    for nz in SC.KERNEL_NZ:
        # 1. exact arithmetic that lands on +-theta, in the dead zone and just outside; 2. seeded values that round
        s1, part1 = SC.update_inputs(nz, na, nu)
        s2 = rng.standard_normal((nz, nu)).astype(F32)
        part2 = rng.standard_normal(part1.shape).astype(F32)
        for s0, part, tau_s, theta in ((s1, part1, SC.KERNEL_TAU_S, SC.KERNEL_THETA), (s2, part2, F32(0.37), F32(0.21))):
            want_s, want_sbar = S.stripe_update(s0, part, tau_s, theta)
            if s0 is s1 and s0.size >= 7:   # conditions on the inputs
                c = part.sum(axis=0, dtype=np.float32)
                w = (s0 - tau_s * c).reshape(-1)
                assert w[0] == theta and w[1] == -theta and abs(w[2]) < theta and w[3] == 0 and w[4] > theta and w[5] < -theta
                assert (want_s.reshape(-1)[:4] == 0).all() and not np.signbit(want_s.reshape(-1)[:4]).any()
                assert want_s.reshape(-1)[4] > 0 > want_s.reshape(-1)[5]
            for shift, pshift in SHIFTS:
                sg, bg, pg = guarded(s0, shift=shift), guarded(s0.shape, shift=shift), guarded(part, shift=pshift)
                ops.pdhg_stripe_update(sg.view, bg.view, pg.view, na, tau_s, theta)
                what = (nz, na, nu, float(theta), shift, pshift)
                same_bits(sg.host(), want_s, what + ("s",))
                same_bits(bg.host(), want_sbar, what + ("s-bar",))
                assert sg.intact() and bg.intact(), (what, "a guard was written")
                pg.check(what, read_only=True)


def test_launches_refuse_what_they_cannot_run():
    from tomobar_amd import ops
    nz, na, nu = 2, 70, 8
    y, r, b, sig = (torch.full((nz, na, nu), float(k), device="cuda") for k in range(1, 5))
    s, sbar = torch.zeros((nz, nu), device="cuda"), torch.ones((nz, nu), device="cuda")
    part = torch.full((2, nz, nu), 7.0, device="cuda")
    keep = [t.clone() for t in (y, s, sbar, part)]
    dual = lambda **kw: ops.pdhg_sino_dual_stripe(**dict(dict(y=y, r=r, b=b, sbar=sbar, part=part, fidelity="LS", sigma=0.25), **kw))  # noqa: E731
    update = lambda **kw: ops.pdhg_stripe_update(**dict(dict(s=s, sbar=sbar, part=part, na=na, tau_s=0.1, theta=0.3), **kw))  # noqa: E731
    with pytest.raises(ValueError, match="unknown PDHG data term"):
        dual(fidelity="PWLS")
    for kw in (dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan"))):
        with pytest.raises(ValueError, match="sigma"):
            dual(**kw)
    for kw in (dict(r=y), dict(b=y), dict(sigma=y), dict(sbar=part[0])):
        with pytest.raises(ValueError, match="alias"):
            dual(**kw)
    for kw in (dict(r=r[:1]), dict(sigma=sig[:, :1]), dict(sbar=sbar[:1]), dict(part=part[:1]), dict(sbar=sbar.T.contiguous().T),
               dict(y=y[0]), dict(part=part.double())):
        with pytest.raises(ValueError, match="shape|contiguous|float32|array"):
            dual(**kw)
    for kw in (dict(tau_s=0.0), dict(tau_s=float("inf")), dict(theta=-0.1), dict(theta=float("nan"))):
        with pytest.raises(ValueError, match="tau_s|theta"):
            update(**kw)
    for kw in (dict(sbar=s), dict(sbar=part[0]), dict(part=part[:1])):
        with pytest.raises(ValueError, match="alias|shape"):
            update(**kw)
    with pytest.raises(ValueError, match="shape"):
        update(na=64)           # one segment where the array holds two
    torch.cuda.synchronize()
    assert all(torch.equal(t, k) for t, k in zip((y, s, sbar, part), keep)), "a refused call launched"


# ------------------------------------------------------------------------------------------------ past 2^31 samples
def test_fused_dual_past_two_to_the_31_samples():
    """tests/_large_index.PROJ_SINO's shape, 8203 x 512 x 512 = 2 150 367 232 samples, every array with the period 5 along z: a
    plane depends on its own z only, so plane z must hold the bits the oracle gives for plane z % 5 -- checked plane by plane
    on the device, for y, for every segment of the partial sums, and for the arrays the launch only reads"""
    from tomobar_amd import ops
    nz, na, nu, p = LI.PROJ_SINO["nz"], LI.PROJ_SINO["na"], LI.PROJ_SINO["nu"], LI.PROJ_PERIOD
    assert nz * na * nu > 2 ** 31
    y0, r0, b0, _, sb0 = SC.kernel_inputs(p, na, nu, seed=8)
    want_y, want_part = S.sino_dual_stripe(y0, r0, b0, sb0, "KL", SC.KERNEL_SIGMA)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    bases = [dev(a) for a in (y0, r0, b0, sb0)]
    y, r, b, sbar = (LI.tiled(t, nz) for t in bases)
    part = torch.full((S.n_seg(na), nz, nu), float("nan"), device="cuda")
    ops.pdhg_sino_dual_stripe(y, r, b, sbar, part, "KL", SC.KERNEL_SIGMA)
    torch.cuda.synchronize()
    checks = [("y", y, dev(want_y)), ("r", r, bases[1]), ("b", b, bases[2]), ("s-bar", sbar, bases[3])]
    checks += [(f"part[{k}]", part[k], dev(want_part[k])) for k in range(part.shape[0])]
    for name, got, period in checks:
        z = LI.first_unequal_plane(got, period, 0, nz, 0)
        assert z is None, (name, "differs from the oracle's period at " + LI._where(z, LI.plane_elems(got.shape)))


# ------------------------------------------------------------------------------------------------ the driver
ITERS = 12
STRIPE_COLUMNS = (3, 11, 17)     # of the unpadded detector; the offsets are OFFSET_SHARES of the sinogram's largest value
OFFSET_SHARES = (0.5, -0.35, 0.25)


@pytest.fixture(scope="module")
def geometries(oracle, golden_dir):
    return GEO.build(oracle, golden_dir)


def _striped(geo, positive):
    """the geometry's sinogram with three offsets planted in every plane (`positive`: the KL data stay non-negative)"""
    top = float(np.abs(geo.sino).max())
    b = geo.sino.copy()
    for z in range(b.shape[0]):
        for c, share in zip(STRIPE_COLUMNS, OFFSET_SHARES):
            b[z, :, c + z] += F32(abs(share) * top if positive else share * top)
    return b


TV = {"method": "PD_TV", "regul_param": 0.002}
TGV = {"method": "PD_TGV", "regul_param": 0.002, "TGV_alpha1": 1.0, "TGV_alpha2": 2.0}
DIAG = {"PDHG_preconditioner": "diagonal"}
# name -> (geometry, _data_ keys beside stripe_lambda (mu as a share of n_angles x the sinogram's largest value), _algorithm_, _regularisation_)
DRIVER_CASES = {
    "LS+TV": ("golden", {}, {"nonnegativity": True}, TV),
    "L1+TV 48": ("n48", {"data_fidelity": "L1"}, {}, {"method": "PD_TV", "regul_param": 0.02, "methodTV": 1}),
    "KL+TV": ("golden", {"data_fidelity": "KL"}, {"nonnegativity": True}, {"method": "PD_TV", "regul_param": 0.001}),
    "LS+TGV": ("golden", {}, {}, TGV),
    "LS no regulariser": ("golden", {}, {"nonnegativity": True}, None),
    "2D KL": ("golden_2d", {"data_fidelity": "KL"}, {}, TV),
    "detector padding": ("golden_pad", {}, {}, TV),
    "initialise ratio 4": ("golden", {}, {"initialise": "x0", "PDHG_ratio": 4}, TV),
    "diagonal LS+TV": ("golden", {}, dict(DIAG, nonnegativity=True), TV),
    "diagonal L1+TV 48": ("n48", {"data_fidelity": "L1"}, dict(DIAG, PDHG_ratio=2), {"method": "PD_TV", "regul_param": 0.02}),
    "diagonal KL+TGV": ("golden", {"data_fidelity": "KL"}, DIAG, TGV),
    "diagonal 2D no regulariser": ("golden_2d", {}, DIAG, None),
    "diagonal detector padding": ("golden_pad", {}, DIAG, TV),
}
MU_SHARE = {"LS": 0.02, "L1": 0.25, "KL": 0.005}   # mu = share x n_angles (x the largest sample for LS: its dual grows with the data)


def _mu(geo, fidelity):
    scale = float(np.abs(geo.sino).max()) if fidelity == "LS" else 1.0
    return float(F32(MU_SHARE[fidelity] * len(geo.angles) * scale))


def _oracle_run(oracle, geo, d, a, r, iterations=ITERS, state=None):
    fid = d.get("data_fidelity", "LS")
    b = oracle.pad_detector(_striped(geo, fid == "KL"), geo.pad)
    x0 = GEO.x0((geo.nz, geo.size, geo.size)) if a.get("initialise") == "x0" else None
    reg = {None: None, "PD_TV": "TV", "PD_TGV": "TGV"}[(r or {}).get("method")]
    r = r or {}
    x = S.pdhg_stripe(geo.projector(), b, geo.L_A, iterations, mu=_mu(geo, fid), fidelity=fid, regulariser=reg,
                      lam=r.get("regul_param"), methodTV=r.get("methodTV", 0), alpha1=r.get("TGV_alpha1", 1.0),
                      alpha0=r.get("TGV_alpha2", 2.0), nonneg=a.get("nonnegativity", False), ratio=a.get("PDHG_ratio", 1.0), x0=x0,
                      diagonal=a.get("PDHG_preconditioner") == "diagonal", state=state)
    return np.ascontiguousarray(oracle.crop_recon(x, geo.n)) if geo.pad else x


def _data(geo, d):
    fid = d.get("data_fidelity", "LS")
    return dict({"projection_data": torch.from_numpy(_striped(geo, fid == "KL")).cuda(), "data_axes_labels_order": list(GEO.LABELS),
                 "stripe_lambda": _mu(geo, fid)}, **d)


def _algorithm(geo, a, **kw):
    algo = dict({"iterations": ITERS, "lipschitz_const": geo.L_A, "recon_mask_radius": None}, **a)
    if algo.get("initialise") == "x0":
        algo["initialise"] = torch.from_numpy(GEO.x0((geo.nz, geo.size, geo.size))).cuda()
    if algo.get("PDHG_preconditioner") == "diagonal":
        del algo["lipschitz_const"]             # not read: the power method must not run either
    return dict(algo, **kw)


@pytest.mark.parametrize("name", list(DRIVER_CASES))
def test_driver_equals_the_oracle_loop(name, geometries, oracle):
    gname, d, a, r = DRIVER_CASES[name]
    geo = geometries[gname]
    state = {}
    want = _oracle_run(oracle, geo, d, a, r, state=state)
    want_s = np.ascontiguousarray(state["s"][:, geo.pad:state["s"].shape[1] - geo.pad])
    # conditions on the inputs: the variable moved, the threshold held a part of it at zero, the image is not empty
    moved = int((state["s"] != 0).sum())
    print(f"PDHG stripe driver {name}: {moved} of {state['s'].size} offsets non-zero, max|s| = {np.abs(state['s']).max():.4g}")
    assert 0 < moved < state["s"].size and np.abs(want).max() > 0
    rt = geo.tools()
    data = _data(geo, d)
    got = rt.PDHG(data, _algorithm(geo, a), None if r is None else dict(r))
    assert isinstance(got, torch.Tensor) and tuple(got.shape) == (geo.nz, geo.n, geo.n)
    run = rt.last_run
    assert (run["method"], run["iterations_done"], run["converged"]) == ("PDHG", ITERS, False)
    assert run["preconditioner"] == a.get("PDHG_preconditioner")
    same_bits(host(got), want, name)
    stripes = run["stripes"]
    assert isinstance(stripes, torch.Tensor) and stripes.dtype == torch.float32 and stripes.is_contiguous()
    assert tuple(stripes.shape) == (geo.nz, geo.n)           # [detY, detX], the padding columns dropped
    same_bits(host(stripes), want_s, (name, "stripes"))


def test_without_the_key_the_driver_returns_the_bits_it_returned(geometries, oracle):
    """absent and None are the same call as before: the float32 oracle loop without the variable, and no `stripes` record"""
    import _pdhg_oracle as PO
    geo = geometries["golden"]
    want = PO.pdhg(geo.projector(), geo.sino, geo.L_A, ITERS, fidelity="LS", lam=0.002, nonneg=True)
    for more in ({}, {"stripe_lambda": None}):
        rt = geo.tools()
        got = rt.PDHG(geo.data(**more), _algorithm(geo, {"nonnegativity": True}), dict(TV))
        same_bits(host(got), want, ("no stripes", more))
        assert "stripes" not in rt.last_run


def test_refusals_on_a_real_object(geometries):
    geo = geometries["golden"]
    algo = {"iterations": 2, "lipschitz_const": geo.L_A}
    rt = geo.tools()
    for bad in (0.0, -1.0):
        with pytest.raises(ValueError, match="stripe_lambda.*positive"):
            rt.PDHG(geo.data(stripe_lambda=bad), dict(algo), dict(TV))
    for name in ("FISTA", "ADMM", "OSEM", "SIRT", "CGLS", "Landweber"):
        with pytest.raises(ValueError, match=r"_data_\['stripe_lambda'\] is available in PDHG only"):
            getattr(rt, name)(geo.data(stripe_lambda=1.0), dict(algo))
    from tomobar_amd.methodsIR_CuPy import RecToolsIRCuPy
    sp = RecToolsIRCuPy(geo.n, 0, geo.nz, 0.0, geo.angles, geo.n, 0, 4, adjoint="matched")
    with pytest.raises(ValueError, match=r"_data_\['stripe_lambda'\] is available in PDHG only"):
        sp.SPDHG(geo.data(stripe_lambda=1.0), dict(algo), dict(TV))
    with pytest.raises(ValueError, match=r"_data_\['ringGH_lambda'\] is available in FISTA only"):
        rt.PDHG(geo.data(stripe_lambda=1.0, ringGH_lambda=0.1), dict(algo), dict(TV))
    assert np.isfinite(host(rt.PDHG(geo.data(stripe_lambda=1.0), dict(algo), dict(TV)))).all()


def test_a_cupy_caller_gets_cupy_stripes_back(geometries, monkeypatch):
    cupy = _cupy_standin.install(monkeypatch)
    geo = geometries["golden"]
    rt = geo.tools()
    algo = {"iterations": 3, "lipschitz_const": geo.L_A}
    sino_t = torch.from_numpy(_striped(geo, False)).cuda()
    data = lambda arr: {"projection_data": arr, "data_axes_labels_order": list(GEO.LABELS), "stripe_lambda": _mu(geo, "LS")}  # noqa: E731
    rt.PDHG(data(sino_t), dict(algo), dict(TV))
    want = host(rt.last_run["stripes"])
    rt.PDHG(data(cupy.ndarray(sino_t)), dict(algo), dict(TV))
    res = rt.last_run["stripes"]
    assert type(res) is cupy.ndarray and res.shape == (geo.nz, geo.n) and res.dtype == np.float32
    assert np.array_equal(res.get(), want)
