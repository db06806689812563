"""PDHG without a GPU: properties of the numpy restatement (tests/_pdhg_oracle.py; the algorithm is the specification,
docs/kernels/pdhg.md) on the inputs of tests/_pdhg_cases.py, and the host surface of the feature -- dictionary defaults, the
refusals, the C-ABI's argument checks and scratch size (the library loads and validates without a device)."""
import ctypes as C
import types

import numpy as np
import pytest

import _pdhg_cases as K
import _pdhg_oracle as P


# ------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("name", list(K.CASES))
def test_float32_against_float64(name):
    """the float32 arithmetic the kernels reproduce holds the project's parity bar against the same algorithm in double
    (largest value seen: 3.1e-6, LS without TV after 300 iterations; docs/kernels/pdhg.md)"""
    f32, f64 = K.run(name, "float32", K.COUNTS), K.run(name, "float64", K.COUNTS)
    for n in K.COUNTS:
        r = P.rel_l2(f32[n], f64[n])
        print(f"PDHG {name} after {n}: float32 vs float64 rel-L2 = {r:.2e}")
        assert f32[n].dtype == np.float32 and f64[n].dtype == np.float64
        assert f32[n].shape == (K.NZ, K.N, K.N)
        assert r <= 1e-5, (name, n, r)


@pytest.mark.parametrize("fidelity", P.FIDELITIES)
@pytest.mark.parametrize("sigma", [0.035, 1.5])
def test_dual_prox_satisfies_moreau(fidelity, sigma):
    """v = prox_{sigma F*}(v) + sigma prox_{F / sigma}(v / sigma) in float64, with the closed-form prox of F itself"""
    rng = np.random.default_rng(31)
    v = rng.uniform(-6.0, 6.0, 4096)
    b = rng.uniform(-2.0, 8.0, 4096)            # negative entries: the KL clamp
    y = P.sino_dual(v, np.zeros_like(v), b, fidelity, sigma)   # y + sigma r = v
    assert y.dtype == np.float64
    back = y + sigma * P.prox_primal(v / sigma, b, fidelity, 1.0 / sigma)
    err = float(np.abs(back - v).max())
    print(f"Moreau {fidelity} sigma {sigma}: max |error| = {err:.2e}")
    assert err <= 1e-12, (fidelity, sigma, err)
    if fidelity == "L1":
        assert (np.abs(y) == 1.0).any() and (np.abs(y) < 1.0).any()   # both branches of the clip


@pytest.mark.parametrize("name", ["LS+TV", "L1+TV", "KL+TV"])
def test_objective_falls_along_the_checkpoints(name):
    kw, positive = K.CASES[name]
    b = K.sinogram(positive=positive)
    its = K.run(name, "float64", K.CHECKPOINTS)
    obj = [P.objective(K.dense(), its[n], b, kw["fidelity"], kw["lam"]) for n in K.CHECKPOINTS]
    at_zero = P.objective(K.dense(), np.zeros((K.NZ, K.N, K.N)), b, kw["fidelity"], kw["lam"])
    print(f"PDHG {name}: objective at 0 = {at_zero:.6g}, at {K.CHECKPOINTS} = {['%.8g' % v for v in obj]}")
    assert all(np.isfinite(obj))
    assert all(later < earlier for earlier, later in zip(obj, obj[1:])), obj
    if kw["fidelity"] == "KL":
        assert at_zero == float("inf")          # log 0: the later checkpoints are compared with x_10 instead
        assert all(v < obj[0] for v in obj[1:])
    else:
        assert all(v < at_zero for v in obj)


def test_l1_survives_zingers_that_ruin_least_squares():
    """+40 on 2 % of the samples: after 1000 float64 iterations L1 + TV is closer to the phantom than LS + TV for every
    lambda tried, by more than the factor 2 asserted (measured: 0.161 against 1.035, a factor 6.4)"""
    l1, ls = K.zinger_errors()
    best = min(ls.values())
    print(f"zingers: L1 + TV error {l1:.4f}; LS + TV errors {ls}; ratio {best / l1:.2f}")
    assert l1 < 0.5 * best, (l1, ls)


@pytest.mark.parametrize("kw", [dict(fidelity="LS", lam=0.5), dict(fidelity="L1", lam=0.5, methodTV=1),
                                dict(fidelity="KL", lam=0.05, nonneg=True)], ids=lambda k: k["fidelity"])
def test_z_constant_volume_gives_the_2d_bits_plane_for_plane(kw):
    """z-terms come last in every sum: with the same L_K, nd = 3 on z-constant data is nd = 2 of one plane"""
    plane = np.ascontiguousarray(K.sinogram(1, positive=kw["fidelity"] == "KL"))
    stack = np.ascontiguousarray(np.broadcast_to(plane[0], (K.NZ,) + plane.shape[1:]))
    L_K = np.float32(K.lipschitz()) + np.float32(12)
    want = P.pdhg(K.matched(1), plane, None, 25, nd=2, L_K=L_K, **kw)
    got = P.pdhg(K.matched(K.NZ), stack, None, 25, nd=3, L_K=L_K, **kw)
    assert got.dtype == want.dtype == np.float32 and np.abs(want).max() > 0
    for z in range(K.NZ):
        assert np.array_equal(got[z].view(np.uint32), want[0].view(np.uint32)), z


@pytest.mark.parametrize("shape", K.MARCH_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_test_inputs_exercise_both_branches_of_the_projection(shape):
    """a condition on the INPUTS of the GPU tests: on the noise input the projection of step 4 changes between 10 % and 90 %
    of the voxels in the first step"""
    for methodTV in (0, 1):
        share = K.march_oracle("noise", shape, methodTV, 0)[1]
        assert 0.1 <= share <= 0.9, (shape, methodTV, share)
    res, _ = K.march_oracle("terraces", shape, 0, 1)
    assert all(np.isfinite(x).all() for x, _, _ in res.values())


def test_scalars_are_float32_and_follow_the_specification():
    sigma, tau = P.scalars(734.7, 3, True, 4.0)
    s = np.float32(0.95) / np.sqrt(np.float32(734.7) + np.float32(12))
    assert type(sigma) is np.float32 and type(tau) is np.float32
    assert sigma == np.float32(s * np.float32(4)) and tau == np.float32(s / np.float32(4))
    assert P.scalars(734.7, 3, False)[0] == np.float32(0.95) / np.sqrt(np.float32(734.7))
    assert P.scalars(734.7, 2)[0] == np.float32(0.95) / np.sqrt(np.float32(734.7) + np.float32(8))


# ------------------------------------------------------------------------------------------------ host surface
def _self(**kw):
    base = dict(Atools=types.SimpleNamespace(device_index=0), OS_number=1, slab=None, adjoint="matched", nonneg_regul=0)
    return types.SimpleNamespace(**dict(base, **kw))


def _dicts(data=None, algo=None, reg=None, method_run="PDHG", me=None):
    import torch
    import tomobar_amd.ops as ops
    from tomobar_amd.supp.dicts import dicts_check
    d = dict({"projection_data": torch.zeros((2, 3, 4), dtype=torch.float32)}, **(data or {}))
    keep = ops.to_device
    ops.to_device = lambda x, index: x   # no GPU here: the projections stay where they are
    try:
        return dicts_check(me or _self(), d, algo, reg, method_run=method_run)
    finally:
        ops.to_device = keep


def test_dicts_check_defaults():
    d, a, r = _dicts()
    assert d["data_fidelity"] == "LS"
    assert a["iterations"] == 500 and a["PDHG_ratio"] == 1.0
    assert (a["nonnegativity"], a["initialise"], a["recon_mask_radius"], a["tolerance"], a["verbose"]) == (False, None, 1.0, 0.0, False)
    assert "lipschitz_const" not in a          # the driver takes it from the power method
    assert r == {"method": None}
    d, a, r = _dicts({"data_fidelity": "L1"}, {"iterations": 7, "PDHG_ratio": 4}, {"method": "PD_TV"})
    assert d["data_fidelity"] == "L1" and a["iterations"] == 7 and a["PDHG_ratio"] == 4
    assert r == {"method": "PD_TV", "regul_param": 0.001, "methodTV": 0}   # nothing else is read, nothing else is filled
    _, _, r = _dicts({"data_fidelity": "KL"}, None, {"method": "PD_TV", "regul_param": 0.3, "methodTV": 1})
    assert r["regul_param"] == 0.3 and r["methodTV"] == 1


REFUSED = [
    ("unmatched adjoint", dict(me=_self(adjoint="unmatched")), 'construct with adjoint="matched"'),
    ("ordered subsets", dict(me=_self(OS_number=4)), "ordered-subsets"),
    ("z-slab", dict(me=_self(slab=object())), "z-slab"),
    ("PWLS", dict(data={"data_fidelity": "PWLS"}), "PWLS"),
    ("SWLS", dict(data={"data_fidelity": "SWLS"}), "SWLS"),
    ("ring key", dict(data={"ringGH_lambda": 0.01}), "ringGH_lambda"),
    ("huber", dict(data={"huber_threshold": 1.0}), "huber_threshold"),
    ("studentst", dict(data={"studentst_threshold": 1.0}), "studentst_threshold"),
    ("unknown fidelity", dict(data={"data_fidelity": "Huber"}), "data_fidelity"),
    ("ROF_TV", dict(reg={"method": "ROF_TV"}), "None or 'PD_TV'"),
    ("TGV", dict(reg={"method": "TGV"}), "None or 'PD_TV'"),
    ("wavelets suffix", dict(reg={"method": "PD_TV_WAVELETS"}), "None or 'PD_TV'"),
    ("NLTV", dict(reg={"method": "NLTV"}), "None or 'PD_TV'"),
    ("slicewise", dict(reg={"method": "PD_TV", "slicewise": True}), "slicewise"),
    ("half precision", dict(reg={"method": "PD_TV", "half_precision": True}), "half_precision"),
    ("ratio 0", dict(algo={"PDHG_ratio": 0.0}), "PDHG_ratio"),
    ("ratio negative", dict(algo={"PDHG_ratio": -2.0}), "PDHG_ratio"),
    ("ratio nan", dict(algo={"PDHG_ratio": float("nan")}), "PDHG_ratio"),
    ("lambda 0", dict(reg={"method": "PD_TV", "regul_param": 0.0}), "regul_param"),
    ("methodTV 2", dict(reg={"method": "PD_TV", "methodTV": 2}), "methodTV"),
]


@pytest.mark.parametrize("what, kw, text", REFUSED, ids=[r[0] for r in REFUSED])
def test_dicts_check_refusals(what, kw, text):
    with pytest.raises(ValueError, match=text):
        _dicts(**kw)


@pytest.mark.parametrize("driver", ["FISTA", "ADMM", "OSEM"])
def test_l1_stays_refused_by_the_other_drivers(driver):
    with pytest.raises(ValueError, match="should be provided as 'LS', 'PWLS', 'KL'"):
        _dicts({"data_fidelity": "L1"}, method_run=driver)
    d, _, _ = _dicts({"data_fidelity": "KL"}, method_run=driver)       # and their dictionaries come out as before
    assert d["data_fidelity"] == "KL"
    assert "PDHG_ratio" not in _dicts(method_run=driver)[1]


def test_the_driver_refuses_before_any_projector_call(monkeypatch):
    """the refusals come from the set-up: neither the power method nor a projection runs"""
    import torch
    from tomobar_amd import methodsIR_CuPy as M
    calls = []

    class Tools:
        device_index, slab, detectors_x_pad, adjoint = 0, None, 0, "matched"
        def vol_shape(self): return (4, 6, 6)
        def sino_shape(self, sub): return (4, 5, 6)
        def __getattr__(self, name):
            calls.append(name)
            raise AssertionError(f"projector attribute {name} touched")

    def rt(**kw):
        obj = M.RecToolsIRCuPy.__new__(M.RecToolsIRCuPy)
        obj.__dict__.update(dict(Atools=Tools(), _slab=None, _OS_number=1, _objsize_user_given=None), **kw)
        return obj

    monkeypatch.setattr(M.ops, "to_device", lambda x, index: x)
    data = {"projection_data": torch.zeros((4, 5, 6), dtype=torch.float32)}
    unmatched = rt()
    unmatched.Atools.adjoint = "unmatched"
    for obj, d, reg, text in ((unmatched, {}, None, 'adjoint="matched"'), (rt(_OS_number=4), {}, None, "ordered-subsets"),
                              (rt(_slab=object()), {}, None, "z-slab"), (rt(), {"data_fidelity": "PWLS"}, None, "PWLS"),
                              (rt(), {}, {"method": "ROF_TV"}, "None or 'PD_TV'")):
        with pytest.raises(ValueError, match=text):
            obj.PDHG(dict(data, **d), {"iterations": 1}, reg)
    assert calls == []


# ------------------------------------------------------------------------------------------------ C-ABI
def test_scratch_bytes_is_the_placed_block_of_the_work_arrays():
    from tomobar_amd import _lib, ops
    lib = _lib.lib()
    skew = ops.ARRAY_SKEW
    for dx, dy, dz in [(37, 13, 7), (64, 64, 64), (1, 1, 1), (200, 150, 40)]:
        arr3 = (dx * dy * dz * 4 + 255) // 256 * 256
        arr2 = (dx * dy * 4 + 255) // 256 * 256
        assert lib.tomo_pdhg_scratch_bytes(dx, dy, dz, 3) == 5 * (arr3 + skew)   # x-bar, g, q1..q3
        assert lib.tomo_pdhg_scratch_bytes(dx, dy, dz, 2) == 4 * (arr2 + skew)   # dz is ignored in 2D


def test_invalid_arguments_are_refused_before_the_device_is_touched():
    from tomobar_amd import _lib
    lib = _lib.lib()
    p = [C.c_void_p(0x1000 * k) for k in range(1, 8)]   # never dereferenced: every case fails validation
    nul = C.c_void_p(0)

    def sino(y=p[0], r=p[1], b=p[2], n=16, fid=0, sigma=0.5):
        return lib.tomo_pdhg_sino_dual(y, r, b, n, fid, sigma, None)

    def dual(xb=p[0], q1=p[1], q2=p[2], q3=p[3], dx=4, dy=4, dz=4, nd=3, sigma=0.5, lam=1.0, m=0):
        return lib.tomo_pdhg_tv_dual(0, xb, q1, q2, q3, dx, dy, dz, nd, sigma, lam, m, None)

    def primal(x=p[0], xb=p[1], g=p[2], q1=p[3], q2=p[4], q3=p[5], dx=4, dy=4, dz=4, nd=3, tau=0.5):
        return lib.tomo_pdhg_primal(0, x, xb, g, q1, q2, q3, dx, dy, dz, nd, tau, 0, None)

    bad = [(sino, dict(fid=3)), (sino, dict(fid=-1)), (sino, dict(sigma=0.0)), (sino, dict(sigma=float("nan"))),
           (sino, dict(y=nul)), (sino, dict(r=p[0])), (sino, dict(b=p[0])),
           (dual, dict(nd=1)), (dual, dict(nd=4)), (dual, dict(dx=0)), (dual, dict(dy=-1)), (dual, dict(dz=0)),
           (dual, dict(sigma=0.0)), (dual, dict(lam=0.0)), (dual, dict(lam=-1.0)), (dual, dict(m=2)), (dual, dict(q3=nul)),
           (dual, dict(q1=p[0])), (dual, dict(q2=p[1])), (dual, dict(xb=nul)),
           (primal, dict(nd=5)), (primal, dict(dx=0)), (primal, dict(tau=0.0)), (primal, dict(tau=float("inf"))),
           (primal, dict(x=nul)), (primal, dict(xb=p[0])), (primal, dict(g=p[1])), (primal, dict(q2=nul)),
           (primal, dict(q1=nul)), (primal, dict(q3=p[0])), (primal, dict(q3=nul))]
    for fn, kw in bad:
        assert fn(**kw) == _lib.E_INVALID, (fn.__name__, kw)
        with pytest.raises(ValueError):
            _lib.check(fn(**kw))
    assert sino(n=0) == _lib.OK   # nothing to do, nothing launched
