"""MI355X tests of PD_TGV in PDHG: the two marches and the driver against the float32 numpy restatement
tests/_pdhg_tgv_oracle.py, bit for bit (there is no reference implementation: formula-level parity, unpinned;
docs/kernels/pdhg.md), on the inputs of tests/_pdhg_tgv_cases.py and the geometries of tests/_pdhg_driver_geometries.py."""
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
import _pdhg_cases as K  # noqa: E402
import _pdhg_driver_geometries as GEO  # noqa: E402
import _pdhg_tgv_cases as T  # noqa: E402
import _pdhg_tgv_oracle as G  # noqa: E402

GROUPS = ("v", "vbar", "p", "q")


def _same_fields(x, xbar, fields, want, what):
    same_bits(host(x), want["x"], what + ("x",))
    same_bits(host(xbar), want["xbar"], what + ("x-bar",))
    for name in GROUPS:
        assert len(fields[name]) == len(want[name]), what + (name,)
        for k, t in enumerate(fields[name]):
            same_bits(host(t), want[name][k], what + (f"{name}{k + 1}",))


# ------------------------------------------------------------------------------------------------ steps 4 and 5
@pytest.mark.parametrize("shape", K.MARCH_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tgv_dual_and_primal_equal_the_oracle(shape):
    from tomobar_amd import ops
    gg, tg = guarded(K.march_g(shape)), guarded(T.march_tau(shape))
    for kind in ("noise", "terraces"):
        x0 = K.march_input(kind, shape)
        r1, r0 = T.MARCH_RADII[kind]
        for per_voxel in (False, True):
            for nonneg in (0, 1):
                want, shares = T.march_oracle(kind, shape, nonneg, per_voxel)
                if kind == "noise":   # a condition on the inputs: both branches of both projections run
                    assert all(0.1 <= s <= 0.9 for s in shares), (shape, shares)
                xg, bg = guarded(x0), guarded(x0)
                x, xbar = xg.view, bg.view
                start = T.march_state(shape)
                bands = {name: [guarded(a) for a in start[name]] for name in GROUPS}
                f = {name: [b.view for b in bands[name]] for name in GROUPS}
                tau_x = tg.view if per_voxel else T.MARCH_TAU_X
                for n in range(1, max(K.MARCH_COUNTS) + 1):
                    ops.pdhg_tgv_dual(xbar, f["vbar"], f["p"], f["q"], T.MARCH_SIGMA_P, T.MARCH_SIGMA_Q, r1, r0)
                    ops.pdhg_tgv_primal(x, xbar, gg.view, f["v"], f["vbar"], f["p"], f["q"], tau_x, T.MARCH_TAU_V, nonneg)
                    if n in K.MARCH_COUNTS:
                        _same_fields(x, xbar, f, want[n], (shape, kind, per_voxel, nonneg, n))
                every = [xg, bg, gg, tg] + [b for name in GROUPS for b in bands[name]]
                assert all(b.intact() for b in every), (shape, kind, "a guard was written")
                assert gg.unchanged() and tg.unchanged(), "g or tau was written"


def test_marches_refuse_what_they_cannot_run():
    from tomobar_amd import ops
    shape = (3, 4, 5)
    x, xbar, g, tau = (torch.full(shape, float(k), device="cuda") for k in range(4))
    v, vbar, p = ([torch.zeros(shape, device="cuda") for _ in range(3)] for _ in range(3))
    q = [torch.zeros(shape, device="cuda") for _ in range(6)]
    keep = [t.clone() for t in (x, xbar)]
    dual = lambda **kw: ops.pdhg_tgv_dual(**dict(dict(xbar=xbar, vbar=vbar, p=p, q=q, sigma_p=0.25, sigma_q=0.3, r1=1.0, r0=2.0), **kw))  # noqa: E731
    primal = lambda **kw: ops.pdhg_tgv_primal(**dict(dict(x=x, xbar=xbar, g=g, v=v, vbar=vbar, p=p, q=q, tau_x=0.2, tau_v=0.15), **kw))  # noqa: E731
    with pytest.raises(ValueError, match="3 dual fields"):
        dual(p=p[:2])
    with pytest.raises(ValueError, match="3 dual fields"):
        primal(v=v[:2])
    with pytest.raises(ValueError, match="6 Q fields"):
        dual(q=q[:3])
    with pytest.raises(ValueError, match="6 Q fields"):
        primal(q=q[:5])
    with pytest.raises(ValueError, match="3 Q fields"):
        ops.pdhg_tgv_dual(xbar[:1], [t[:1] for t in vbar[:2]], [t[:1] for t in p[:2]], [t[:1] for t in q], 0.25, 0.3, 1.0, 2.0)
    for kw in (dict(p=[p[0], p[1], p[0]]), dict(q=q[:5] + [q[0]]), dict(p=[p[0], p[1], xbar]), dict(q=q[:5] + [vbar[1]])):
        with pytest.raises(ValueError, match="alias"):
            dual(**kw)
    for kw in (dict(xbar=x), dict(g=xbar), dict(v=[v[0], v[1], x]), dict(vbar=[vbar[0], v[0], vbar[2]]), dict(p=[p[0], p[1], xbar]),
               dict(q=q[:5] + [g]), dict(tau_x=tau, q=q[:5] + [tau]), dict(tau_x=x), dict(tau_x=g)):
        with pytest.raises(ValueError, match="alias"):
            primal(**kw)
    with pytest.raises(ValueError, match="shape"):
        primal(g=g[:2])
    with pytest.raises(ValueError, match="shape"):
        primal(tau_x=tau[:2])
    with pytest.raises(ValueError, match="shape"):
        dual(q=q[:5] + [q[5][:2]])
    for kw in (dict(sigma_p=0.0), dict(sigma_q=-1.0), dict(r1=0.0), dict(r0=float("nan"))):
        with pytest.raises(ValueError, match="sigma|radii"):
            dual(**kw)
    for kw in (dict(tau_x=0.0), dict(tau_v=-0.5), dict(tau_x=tau, tau_v=0.0)):
        with pytest.raises(ValueError, match="tau"):
            primal(**kw)
    torch.cuda.synchronize()
    assert all(torch.equal(t, k) for t, k in zip((x, xbar), keep)), "a refused call launched"
    assert all(float(t.abs().max()) == 0.0 for t in v + vbar + p + q), "a refused call launched"


def test_work_arrays_come_from_one_placed_block_of_the_stated_size():
    from tomobar_amd import _lib, ops
    lib = _lib.lib()
    shape = (5, 13, 37)
    step = (5 * 13 * 37 * 4 + 255) // 256 * 256 + ops.ARRAY_SKEW
    xbar, g, p, q, v, vbar, lease = ops.pdhg_tgv_work_arrays(shape, "cuda:0")
    arrs = [xbar, g] + p + q + v + vbar
    assert (len(p), len(q), len(v), len(vbar), len(arrs)) == (3, 6, 3, 3, 17)
    assert all(tuple(a.shape) == shape and a.dtype == torch.float32 and a.is_contiguous() for a in arrs)
    assert [a.data_ptr() - xbar.data_ptr() for a in arrs] == [k * step for k in range(17)] and xbar.data_ptr() % 256 == 0
    assert lib.tomo_pdhg_tgv_scratch_bytes(37, 13, 5, 3) == 17 * step
    assert ops.lease_is_current(lease)
    xbar, g, p, q, v, vbar, tau, lease2 = ops.pdhg_tgv_work_arrays(shape, "cuda:0", tau=True)
    assert tau.data_ptr() - xbar.data_ptr() == 17 * step and tuple(tau.shape) == shape
    assert lib.tomo_pdhg_tgv_diag_scratch_bytes(37, 13, 5, 3) == 18 * step
    assert ops.lease_is_current(lease2) and not ops.lease_is_current(lease)
    step2 = (13 * 37 * 4 + 255) // 256 * 256 + ops.ARRAY_SKEW
    xbar, g, p, q, v, vbar, tau, _ = ops.pdhg_tgv_work_arrays((1, 13, 37), "cuda:0", tau=True)
    arrs = [xbar, g] + p + q + v + vbar + [tau]
    assert (len(p), len(q), len(v), len(vbar)) == (2, 3, 2, 2)
    assert [a.data_ptr() - xbar.data_ptr() for a in arrs] == [k * step2 for k in range(12)] and xbar.data_ptr() % 256 == 0
    assert lib.tomo_pdhg_tgv_scratch_bytes(37, 13, 5, 2) == 11 * step2 and lib.tomo_pdhg_tgv_diag_scratch_bytes(37, 13, 5, 2) == 12 * step2
    assert len(ops.pdhg_work_arrays(shape, "cuda:0", True)) == 4          # the TV call is what it was


# ------------------------------------------------------------------------------------------------ the driver
ITERS = 12


@pytest.fixture(scope="module")
def geometries(oracle, golden_dir):
    return GEO.build(oracle, golden_dir)


def _reg(lam, alpha1=1.0, alpha2=2.0):
    return {"method": "PD_TGV", "regul_param": lam, "TGV_alpha1": alpha1, "TGV_alpha2": alpha2}


# name -> (geometry, _data_ keys, _algorithm_ keys, _regularisation_)
DRIVER_CASES = {
    "LS+TGV nonneg": ("golden", {}, {"nonnegativity": True}, _reg(0.002)),
    "L1+TGV 48": ("n48", {"data_fidelity": "L1"}, {}, _reg(0.02, 1.5, 2.5)),
    "KL+TGV nonneg": ("golden", {"data_fidelity": "KL"}, {"nonnegativity": True}, _reg(0.001)),
    "2D": ("golden_2d", {"data_fidelity": "KL"}, {}, _reg(0.002, 0.75, 3.0)),
    "initialise": ("golden", {}, {"initialise": "x0"}, _reg(0.002)),
    "ratio 4": ("n48", {"data_fidelity": "L1"}, {"PDHG_ratio": 4}, _reg(0.02)),
    "mask 0.85": ("golden", {}, {"recon_mask_radius": 0.85}, _reg(0.002)),
    "detector padding": ("golden_pad", {}, {}, _reg(0.002)),
    "diagonal LS": ("golden", {}, {"PDHG_preconditioner": "diagonal", "nonnegativity": True}, _reg(0.002, 1.5, 2.5)),
    "diagonal KL": ("golden", {"data_fidelity": "KL"}, {"PDHG_preconditioner": "diagonal", "PDHG_ratio": 2}, _reg(0.001)),
}


def _oracle_run(oracle, geo, d, a, r, iterations=ITERS, many=None, state=None):
    b = oracle.pad_detector(geo.sino, geo.pad)
    x0 = GEO.x0((geo.nz, geo.size, geo.size)) if a.get("initialise") == "x0" else None
    kw = dict(fidelity=d.get("data_fidelity", "LS"), lam=r["regul_param"], alpha1=r["TGV_alpha1"], alpha0=r["TGV_alpha2"],
              nonneg=a.get("nonnegativity", False), ratio=a.get("PDHG_ratio", 1.0), x0=x0,
              diagonal=a.get("PDHG_preconditioner") == "diagonal", state=state)
    if many is not None:
        return G.pdhg_tgv_many(geo.projector(), b, geo.L_A, many, **kw)
    x = G.pdhg_tgv(geo.projector(), b, geo.L_A, iterations, **kw)
    if geo.pad:
        return np.ascontiguousarray(oracle.crop_recon(x, geo.n))     # a cropped result is not masked
    radius = a.get("recon_mask_radius")
    return x if radius is None else oracle.circular_mask(x, radius).astype(np.float32)


def _algorithm(geo, a, **kw):
    algo = dict({"iterations": ITERS, "lipschitz_const": geo.L_A, "recon_mask_radius": None}, **a)
    if algo.get("initialise") == "x0":
        algo["initialise"] = torch.from_numpy(GEO.x0((geo.nz, geo.size, geo.size))).cuda()
    return dict(algo, **kw)


@pytest.mark.parametrize("name", list(DRIVER_CASES))
def test_driver_equals_the_oracle_loop(name, geometries, oracle):
    from tomobar_amd import ops
    gname, d, a, r = DRIVER_CASES[name]
    geo = geometries[gname]
    state = {}
    want = _oracle_run(oracle, geo, d, a, r, state=state)
    rt = geo.tools()
    algo = _algorithm(geo, a)
    diag = a.get("PDHG_preconditioner") == "diagonal"
    if diag:
        del algo["lipschitz_const"]             # not read: the power method must not run either
    got = rt.PDHG(geo.data(**d), algo, dict(r))
    assert isinstance(got, torch.Tensor) and tuple(got.shape) == (geo.nz, geo.n, geo.n)
    assert rt.Atools.kernel_path("bp").startswith("matched")
    run = rt.last_run
    assert (run["method"], run["iterations_done"], run["converged"], run["regulariser"]) == ("PDHG", ITERS, False, "PD_TGV")
    assert run["preconditioner"] == ("diagonal" if diag else None) and ("lipschitz_const" in algo) == (not diag)
    assert np.abs(want).max() > 0
    same_bits(host(got), want, name)
    # the rest of the state, through the placed block
    arrays = ops.pdhg_tgv_work_arrays((geo.nz, geo.size, geo.size), "cuda:0", tau=diag)
    xbar, _, p, q, v, vbar = arrays[:6]
    same_bits(host(xbar), state["xbar"], (name, "x-bar"))
    for fields, key in ((p, "p"), (q, "q"), (v, "v"), (vbar, "vbar")):
        assert len(fields) == len(state[key])
        for k, t in enumerate(fields):
            same_bits(host(t), state[key][k], (name, f"{key}{k + 1}"))
    assert any(np.abs(c).max() > 0 for c in state["v"]) and any(np.abs(c).max() > 0 for c in state["q"]), "v or Q never moved"
    if diag:
        same_bits(host(arrays[6]), state["tau"], (name, "tau"))


def test_lipschitz_constant_comes_from_the_power_method_on_the_matched_pair(geometries, oracle):
    geo = geometries["golden"]
    rt = geo.tools()
    rt.power_seed = 5
    L_A = rt.powermethod({"projection_data": None})
    rt.power_seed = 5
    algo = {"iterations": 3, "recon_mask_radius": None}
    got = rt.PDHG(geo.data(), algo, {"method": "PD_TGV", "regul_param": 0.002})
    assert algo["lipschitz_const"] == L_A
    want = G.pdhg_tgv(geo.projector(), geo.sino, L_A, 3, lam=0.002)
    same_bits(host(got), want, "power method")


def test_a_run_stopped_by_the_tolerance_is_the_run_of_that_many_iterations(geometries, oracle):
    geo = geometries["golden"]
    gname, d, a, r = DRIVER_CASES["LS+TGV nonneg"]
    total = 30
    its = _oracle_run(oracle, geo, d, a, r, many=range(1, total + 1))
    from _tgv_oracle import rel_d
    seq = [rel_d(its[1], np.zeros_like(its[1]))] + [rel_d(its[k], its[k - 1]) for k in range(2, total + 1)]
    j = 14
    tol = float(np.sqrt(seq[j - 2] * seq[j - 1]))
    stop = next(k for k, v in enumerate(seq, 1) if v < tol)
    # conditions on the input: the run stops inside the loop and no value lies within 1 % of the threshold
    assert 3 <= stop < total and all(abs(v - tol) >= 0.01 * tol for v in seq), (stop, tol, seq)
    rt = geo.tools()
    got = host(rt.PDHG(geo.data(**d), _algorithm(geo, a, iterations=total, tolerance=tol), dict(r)))
    run = rt.last_run
    print(f"PDHG + TGV tolerance {tol:.4e}: stopped after {run['iterations_done']} (oracle {stop})")
    assert run["converged"] and run["iterations_done"] == stop and len(run["rel_change"]) == stop
    plain = host(geo.tools().PDHG(geo.data(**d), _algorithm(geo, a, iterations=run["iterations_done"]), dict(r)))
    assert np.array_equal(got, plain)
    same_bits(got, its[stop], "stopped run against the oracle")


def test_refusals_on_a_real_object(geometries):
    geo = geometries["golden"]
    algo = {"iterations": 2, "lipschitz_const": geo.L_A}
    rt = geo.tools()
    with pytest.raises(ValueError, match=r"None or 'PD_TV' \(the TV term in its dual\) or 'PD_TGV' \(the TGV term in its dual\), not 'TGV'"):
        rt.PDHG(geo.data(), dict(algo), {"method": "TGV"})
    with pytest.raises(ValueError, match="TGV_alpha1"):
        rt.PDHG(geo.data(), dict(algo), {"method": "PD_TGV", "TGV_alpha1": 0.0})
    from tomobar_amd.methodsIR_CuPy import RecToolsIRCuPy
    sp = RecToolsIRCuPy(geo.n, 0, geo.nz, 0.0, geo.angles, geo.n, 0, 4, adjoint="matched")
    with pytest.raises(ValueError, match=r"SPDHG takes _regularisation_\['method'\] = None or 'PD_TV' \(the TV term in its dual\), not 'PD_TGV'"):
        sp.SPDHG(geo.data(), dict(algo), {"method": "PD_TGV"})
    # the object still reconstructs afterwards
    assert np.isfinite(host(rt.PDHG(geo.data(), dict(algo), {"method": "PD_TGV"}))).all()


def test_layouts_are_planar_again_after_a_call_that_raises_inside_the_loop(geometries, monkeypatch):
    from tomobar_amd import ops
    geo = geometries["golden"]
    rt = geo.tools()
    A = rt.Atools
    algo = {"iterations": 4, "lipschitz_const": geo.L_A, "recon_mask_radius": None}
    reg = _reg(0.002)
    want = host(rt.PDHG(geo.data(), dict(algo), dict(reg)))
    real, calls = ops.pdhg_tgv_primal, []

    def failing(*args, **kw):
        calls.append(1)
        if len(calls) == 2:
            raise RuntimeError("stop here")
        return real(*args, **kw)

    monkeypatch.setattr(ops, "pdhg_tgv_primal", failing)
    A.set_volume_layout("zquad", require_ok=False)       # what an interrupted driver could have left behind
    with pytest.raises(RuntimeError, match="stop here"):
        rt.PDHG(geo.data(), dict(algo), dict(reg))
    assert len(calls) == 2
    assert A.residual_layout() == "planar" and A.volume_layout() == "planar"
    monkeypatch.setattr(ops, "pdhg_tgv_primal", real)
    assert np.array_equal(host(rt.PDHG(geo.data(), dict(algo), dict(reg))), want)


def test_a_cupy_caller_gets_cupy_back(geometries, monkeypatch):
    cupy = _cupy_standin.install(monkeypatch)
    geo = geometries["golden"]
    rt = geo.tools()
    algo = {"iterations": 3, "lipschitz_const": geo.L_A}
    reg = _reg(0.002)
    sino_t = torch.from_numpy(geo.sino.copy()).cuda()
    keep = sino_t.clone()
    want = rt.PDHG({"projection_data": sino_t, "data_axes_labels_order": list(GEO.LABELS)}, dict(algo), dict(reg))
    res = rt.PDHG({"projection_data": cupy.ndarray(sino_t), "data_axes_labels_order": list(GEO.LABELS)}, dict(algo), dict(reg))
    assert isinstance(want, torch.Tensor)
    assert type(res) is cupy.ndarray and res.shape == (geo.nz, geo.n, geo.n) and res.dtype == np.float32
    assert np.array_equal(res.get(), host(want))
    assert torch.equal(sino_t, keep), "the caller's projection data must not be written"
