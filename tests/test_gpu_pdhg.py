"""MI355X tests of PDHG: the three shipped kernels and the driver against the float32 numpy restatement
tests/_pdhg_oracle.py, bit for bit (there is no reference implementation: formula-level parity, unpinned;
docs/kernels/pdhg.md), on the inputs of tests/_pdhg_cases.py."""
import os
import sys
import types

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
import _pdhg_oracle as P  # noqa: E402


# ------------------------------------------------------------------------------------------------ step 2
SINO_EXTENTS = [(1,), (3,), (63,), (64,), (65,), (4099,), (5, 23, 48)]


def _sino_inputs(shape):
    rng = np.random.default_rng(41)
    y = (2.0 * rng.standard_normal(shape)).astype(np.float32)      # reaches beyond +-1: the L1 clip
    r = rng.uniform(-1.0, 9.0, shape).astype(np.float32)
    b = rng.uniform(-2.0, 8.0, shape).astype(np.float32)           # negative entries: the KL clamp
    return y, r, b


@pytest.mark.parametrize("sigma", [0.035, 1.5])
@pytest.mark.parametrize("fidelity", P.FIDELITIES)
@pytest.mark.parametrize("shape", SINO_EXTENTS, ids=lambda s: "x".join(map(str, s)))
def test_sino_dual_equals_the_oracle(shape, fidelity, sigma):
    from tomobar_amd import ops
    y, r, b = _sino_inputs(shape)
    sigma = np.float32(sigma)
    want = P.sino_dual(y, r, b, fidelity, sigma)
    assert want.dtype == np.float32
    if fidelity == "L1" and y.size > 8:
        assert (np.abs(want) == 1).any() and (np.abs(want) < 1).any()
    yg, rg, bg = guarded(y), guarded(r), guarded(b)
    yd, rd, bd = yg.view, rg.view, bg.view
    assert ops.pdhg_sino_dual(yd, rd, bd, fidelity, sigma) is yd
    same_bits(host(yd), want, (shape, fidelity, float(sigma)))
    assert yg.intact() and rg.intact() and bg.intact() and rg.unchanged() and bg.unchanged()
    # two applications: the dual is really updated in place
    ops.pdhg_sino_dual(yd, rd, bd, fidelity, sigma)
    same_bits(host(yd), P.sino_dual(want, r, b, fidelity, sigma), (shape, fidelity, "second application"))


@pytest.mark.parametrize("fidelity", P.FIDELITIES)
def test_sino_dual_on_arrays_that_are_not_16_byte_aligned(fidelity):
    """the scalar form: every array starts 4 bytes past a 16-byte boundary"""
    from tomobar_amd import ops
    y, r, b = _sino_inputs((4100,))
    sigma = np.float32(0.4)
    full = [torch.from_numpy(a).cuda() for a in (y, r, b)]
    yd, rd, bd = (t[1:] for t in full)
    assert all(t.data_ptr() % 16 == 4 and t.is_contiguous() for t in (yd, rd, bd))
    ops.pdhg_sino_dual(yd, rd, bd, fidelity, sigma)
    same_bits(host(yd), P.sino_dual(y[1:], r[1:], b[1:], fidelity, sigma), fidelity)
    assert host(full[0])[0] == y[0]


def test_sino_dual_refuses_what_it_cannot_run():
    from tomobar_amd import ops
    y, r, b = (torch.zeros(8, device="cuda") for _ in range(3))
    with pytest.raises(ValueError, match="LS, L1 and KL"):
        ops.pdhg_sino_dual(y, r, b, "PWLS", 0.5)
    with pytest.raises(ValueError):
        ops.pdhg_sino_dual(y, r[:4], b, "LS", 0.5)
    with pytest.raises(ValueError, match="sigma"):
        ops.pdhg_sino_dual(y, r, b, "LS", 0.0)


# ------------------------------------------------------------------------------------------------ steps 4 and 5
@pytest.mark.parametrize("shape", K.MARCH_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tv_dual_and_primal_equal_the_oracle(shape):
    from tomobar_amd import ops
    g_host = K.march_g(shape)
    gg = guarded(g_host)
    g = gg.view
    nd = 3 if shape[0] > 1 else 2
    for kind in ("noise", "terraces"):
        x0 = K.march_input(kind, shape)
        lam = K.MARCH_LAMBDA[kind]
        for methodTV in (0, 1):
            for nonneg in (0, 1):
                want, share = K.march_oracle(kind, shape, methodTV, nonneg)
                if kind == "noise":   # a condition on the inputs: both branches of the projection run
                    assert 0.1 <= share <= 0.9, (shape, methodTV, share)
                xg, bg = guarded(x0), guarded(x0)
                x, xbar = xg.view, bg.view
                qs = [guarded(np.zeros(shape, np.float32)) for _ in range(nd)]
                q = [b.view for b in qs]
                for n in range(1, max(K.MARCH_COUNTS) + 1):
                    ops.pdhg_tv_dual(xbar, q, K.MARCH_SIGMA, lam, methodTV)
                    ops.pdhg_primal(x, xbar, g, q, K.MARCH_TAU, nonneg)
                    if n in K.MARCH_COUNTS:
                        what = (shape, kind, methodTV, nonneg, n)
                        wx, wb, wq = want[n]
                        same_bits(host(x), wx, what + ("x",))
                        same_bits(host(xbar), wb, what + ("x-bar",))
                        for d in range(nd):
                            same_bits(host(q[d]), wq[d], what + (f"q{d + 1}",))
                assert all(b.intact() for b in [xg, bg, gg] + qs), (shape, kind, "a guard was written")
                assert gg.unchanged(), "g was written"
    # without the TV block: div q = 0
    x0 = K.march_input("noise", shape) - np.float32(0.4)
    for nonneg in (0, 1):
        want = P.march_steps(x0, g_host, K.MARCH_SIGMA, K.MARCH_TAU, None, 0, nonneg, (3,))[3]
        xg, bg = guarded(x0), guarded(x0)
        x, xbar = xg.view, bg.view
        for _ in range(3):
            ops.pdhg_primal(x, xbar, g, [], K.MARCH_TAU, nonneg)
        same_bits(host(x), want[0], (shape, "no TV", nonneg, "x"))
        same_bits(host(xbar), want[1], (shape, "no TV", nonneg, "x-bar"))
        assert xg.intact() and bg.intact() and gg.intact() and gg.unchanged()


def test_marches_refuse_what_they_cannot_run():
    from tomobar_amd import ops
    x, xbar, g, q1, q2, q3 = (torch.zeros((3, 4, 5), device="cuda") for _ in range(6))
    with pytest.raises(ValueError, match="3 dual fields"):
        ops.pdhg_tv_dual(xbar, [q1, q2], 0.25, 1.0)
    with pytest.raises(ValueError, match="lambda"):
        ops.pdhg_tv_dual(xbar, [q1, q2, q3], 0.25, 0.0)
    with pytest.raises(ValueError, match="alias"):
        ops.pdhg_tv_dual(xbar, [q1, q2, q1], 0.25, 1.0)
    with pytest.raises(ValueError, match="alias"):
        ops.pdhg_primal(x, x, g, [q1, q2, q3], 0.25)
    with pytest.raises(ValueError, match="shape"):
        ops.pdhg_primal(x, xbar, g[:2], [], 0.25)
    with pytest.raises(ValueError, match="tau"):
        ops.pdhg_primal(x, xbar, g, [], -1.0)


def test_work_arrays_come_from_one_placed_block_of_the_stated_size():
    from tomobar_amd import _lib, ops
    shape = (5, 13, 37)
    xbar, g, q, lease = ops.pdhg_work_arrays(shape, "cuda:0", True)
    arrs = [xbar, g] + q
    assert len(q) == 3 and all(tuple(a.shape) == shape and a.dtype == torch.float32 and a.is_contiguous() for a in arrs)
    step = (5 * 13 * 37 * 4 + 255) // 256 * 256 + ops.ARRAY_SKEW
    assert [a.data_ptr() - xbar.data_ptr() for a in arrs] == [k * step for k in range(5)] and xbar.data_ptr() % 256 == 0
    assert _lib.lib().tomo_pdhg_scratch_bytes(37, 13, 5, 3) == 5 * step
    assert ops.lease_is_current(lease)
    xbar2, g2, q2, _ = ops.pdhg_work_arrays((1, 13, 37), "cuda:0", True)
    assert len(q2) == 2 and ops.pdhg_work_arrays(shape, "cuda:0", False)[2] == []


# ------------------------------------------------------------------------------------------------ the driver
Geometry, LABELS = GEO.Geometry, GEO.LABELS     # under these names tests/test_gpu_streams.py builds its `golden` case
ITERS = 12


@pytest.fixture(scope="module")
def geometries(oracle, golden_dir):
    return GEO.build(oracle, golden_dir)


# name -> (geometry, _data_ keys, _algorithm_ keys, _regularisation_)
DRIVER_CASES = {
    "LS+TV nonneg": ("golden", {}, {"nonnegativity": True}, {"method": "PD_TV", "regul_param": 0.002}),
    "LS+TV nonneg 48": ("n48", {}, {"nonnegativity": True}, {"method": "PD_TV", "regul_param": 0.03}),
    "L1+aniso": ("n48", {"data_fidelity": "L1"}, {}, {"method": "PD_TV", "regul_param": 0.02, "methodTV": 1}),
    "KL+TV": ("golden", {"data_fidelity": "KL"}, {"nonnegativity": True}, {"method": "PD_TV", "regul_param": 0.001}),
    "no regulariser": ("n48", {}, {}, None),
    "initialise": ("golden", {}, {"initialise": "x0"}, {"method": "PD_TV", "regul_param": 0.002}),
    "ratio 4": ("n48", {"data_fidelity": "L1"}, {"PDHG_ratio": 4}, {"method": "PD_TV", "regul_param": 0.02}),
    "mask 0.85": ("golden", {}, {"recon_mask_radius": 0.85}, {"method": "PD_TV", "regul_param": 0.002}),
    "detector padding": ("golden_pad", {}, {}, {"method": "PD_TV", "regul_param": 0.002}),
    "2D": ("golden_2d", {"data_fidelity": "KL"}, {}, {"method": "PD_TV", "regul_param": 0.002, "methodTV": 1}),
}


def _oracle_run(oracle, geo, d, a, r, iterations=ITERS, many=None):
    b = oracle.pad_detector(geo.sino, geo.pad)
    x0 = GEO.x0((geo.nz, geo.size, geo.size)) if a.get("initialise") == "x0" else None
    kw = dict(fidelity=d.get("data_fidelity", "LS"), lam=None if r is None else r["regul_param"],
              methodTV=0 if r is None else r.get("methodTV", 0), nonneg=a.get("nonnegativity", False),
              ratio=a.get("PDHG_ratio", 1.0), x0=x0)
    if many is not None:
        return P.pdhg_many(geo.projector(), b, geo.L_A, many, **kw)
    x = P.pdhg(geo.projector(), b, geo.L_A, iterations, **kw)
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
    gname, d, a, r = DRIVER_CASES[name]
    geo = geometries[gname]
    want = _oracle_run(oracle, geo, d, a, r)
    rt = geo.tools()
    got = rt.PDHG(geo.data(**d), _algorithm(geo, a), None if r is None else dict(r))
    assert isinstance(got, torch.Tensor) and tuple(got.shape) == (geo.nz, geo.n, geo.n)
    assert rt.Atools.kernel_path("bp").startswith("matched")
    assert rt.last_run["method"] == "PDHG" and rt.last_run["iterations_done"] == ITERS and not rt.last_run["converged"]
    assert np.abs(want).max() > 0
    same_bits(host(got), want, name)


def test_lipschitz_constant_comes_from_the_power_method_on_the_matched_pair(geometries, oracle):
    geo = geometries["golden"]
    rt = geo.tools()
    rt.power_seed = 5
    L_A = rt.powermethod({"projection_data": None})
    rt.power_seed = 5
    algo = {"iterations": 3, "recon_mask_radius": None}
    got = rt.PDHG(geo.data(), algo, {"method": "PD_TV", "regul_param": 0.002})
    assert algo["lipschitz_const"] == L_A
    want = P.pdhg(geo.projector(), geo.sino, L_A, 3, lam=0.002)
    same_bits(host(got), want, "power method")


def test_a_run_stopped_by_the_tolerance_is_the_run_of_that_many_iterations(geometries, oracle):
    geo = geometries["golden"]
    gname, d, a, r = DRIVER_CASES["LS+TV nonneg"]
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
    print(f"PDHG tolerance {tol:.4e}: stopped after {run['iterations_done']} (oracle {stop})")
    assert run["converged"] and run["iterations_done"] == stop and len(run["rel_change"]) == stop
    plain = host(geo.tools().PDHG(geo.data(**d), _algorithm(geo, a, iterations=run["iterations_done"]), dict(r)))
    assert np.array_equal(got, plain)
    same_bits(got, its[stop], "stopped run against the oracle")


def test_refusals_on_a_real_object(geometries):
    geo = geometries["golden"]
    algo = {"iterations": 2, "lipschitz_const": geo.L_A}
    with pytest.raises(ValueError, match='construct with adjoint="matched"'):
        geo.tools(adjoint="unmatched").PDHG(geo.data(), dict(algo))
    with pytest.raises(ValueError, match="ordered-subsets"):
        geo.tools(OS_number=4).PDHG(geo.data(), dict(algo))
    rt = geo.tools()
    rt.slab = types.SimpleNamespace(world=2, rank=0)
    with pytest.raises(ValueError, match="z-slab"):
        rt.PDHG(geo.data(), dict(algo))
    rt = geo.tools()
    with pytest.raises(ValueError, match="PWLS"):
        rt.PDHG(geo.data(data_fidelity="PWLS"), dict(algo))
    with pytest.raises(ValueError, match="None or 'PD_TV'"):
        rt.PDHG(geo.data(), dict(algo), {"method": "ROF_TV"})
    with pytest.raises(ValueError, match="should be provided as 'LS', 'PWLS', 'KL'"):
        rt.FISTA(geo.data(data_fidelity="L1"), dict(algo))
    # the object still reconstructs afterwards
    assert np.isfinite(host(rt.PDHG(geo.data(), dict(algo)))).all()


def test_layouts_are_planar_again_after_a_call_that_raises_inside_the_loop(geometries, monkeypatch):
    from tomobar_amd import ops
    geo = geometries["golden"]
    rt = geo.tools()
    A = rt.Atools
    algo = {"iterations": 4, "lipschitz_const": geo.L_A, "recon_mask_radius": None}
    reg = {"method": "PD_TV", "regul_param": 0.002}
    want = host(rt.PDHG(geo.data(), dict(algo), dict(reg)))
    real, calls = ops.pdhg_primal, []

    def failing(*args, **kw):
        calls.append(1)
        if len(calls) == 2:
            raise RuntimeError("stop here")
        return real(*args, **kw)

    monkeypatch.setattr(ops, "pdhg_primal", failing)
    A.set_volume_layout("zquad", require_ok=False)       # what an interrupted driver could have left behind
    with pytest.raises(RuntimeError, match="stop here"):
        rt.PDHG(geo.data(), dict(algo), dict(reg))
    assert len(calls) == 2
    assert A.residual_layout() == "planar" and A.volume_layout() == "planar"
    monkeypatch.setattr(ops, "pdhg_primal", real)
    assert np.array_equal(host(rt.PDHG(geo.data(), dict(algo), dict(reg))), want)


def test_a_cupy_caller_gets_cupy_back(geometries, monkeypatch):
    cupy = _cupy_standin.install(monkeypatch)
    geo = geometries["golden"]
    rt = geo.tools()
    algo = {"iterations": 3, "lipschitz_const": geo.L_A}
    reg = {"method": "PD_TV", "regul_param": 0.002}
    sino_t = torch.from_numpy(geo.sino.copy()).cuda()
    keep = sino_t.clone()
    want = rt.PDHG({"projection_data": sino_t, "data_axes_labels_order": list(LABELS)}, dict(algo), dict(reg))
    res = rt.PDHG({"projection_data": cupy.ndarray(sino_t), "data_axes_labels_order": list(LABELS)}, dict(algo), dict(reg))
    assert isinstance(want, torch.Tensor)
    assert type(res) is cupy.ndarray and res.shape == (geo.nz, geo.n, geo.n) and res.dtype == np.float32
    assert np.array_equal(res.get(), host(want))
    assert torch.equal(sino_t, keep), "the caller's projection data must not be written"
