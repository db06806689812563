"""SPDHG without a GPU: properties of the numpy restatement (tests/_spdhg_oracle.py; the algorithm is the specification,
docs/kernels/spdhg.md) on the inputs of tests/_spdhg_cases.py, and the host surface of the feature -- dictionary defaults,
the refusals, the C-ABI's argument checks and scratch size (the library loads and validates without a device)."""
import ctypes as C
import types

import numpy as np
import pytest

import _pdhg_cases as K
import _pdhg_oracle as P
import _spdhg_cases as SK
import _spdhg_oracle as S


# ------------------------------------------------------------------------------------------------ the draws
@pytest.mark.parametrize("m, iterations", [(1, 200), (4, 50), (8, 100), (12, 20)])
def test_the_tv_block_is_drawn_half_of_the_time(m, iterations):
    """a condition on the INPUT (seed 0): with TV the values >= m make up 40-60 % of at least 400 draws, every subset is
    drawn, and the sequence is the documented generator call"""
    seq = S.draws(0, m, True, iterations)
    E = 2 * m
    assert seq.size == iterations * E >= 400
    assert np.array_equal(seq, np.random.default_rng(0).integers(0, E, size=iterations * E))
    share = float(np.mean(seq >= m))
    print(f"SPDHG draws m = {m}: TV share {share:.3f} of {seq.size}")
    assert 0.4 <= share <= 0.6
    assert set(seq[seq < m]) == set(range(m))
    without = S.draws(0, m, False, iterations)
    assert without.size == iterations * m and (m == 1 or without.max() == m - 1) and without.min() == 0


def test_scalars_are_float32_and_follow_the_specification():
    f = np.float32
    sA, sG, tau, wA, wG = S.scalars(734.7, 3, 8, True, 4.0)
    assert all(type(v) is np.float32 for v in (sA, sG, tau, wA, wG))
    c, g, nA, nG = f(0.95), f(4), np.sqrt(f(734.7)), np.sqrt(f(12))
    assert (wA, wG) == (f(16), f(2))
    assert sA == (c * g) / nA and sG == (c * g) / nG
    assert tau == min((c / g) / (f(16) * nA), (c / g) / (f(2) * nG))
    # sigma_j tau |K_j|^2 <= 0.9025 p_j (up to the roundings)
    assert float(sA) * float(tau) * 734.7 <= 0.9025 / 16 * (1 + 1e-6) and float(sG) * float(tau) * 12 <= 0.9025 / 2 * (1 + 1e-6)
    sA, _, tau, wA, _ = S.scalars(734.7, 2, 6, False)
    assert wA == f(6) and tau == (c / f(1)) / (f(6) * nA) and sA == c / nA


# ------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("name", list(SK.SUBSETS))
def test_float32_against_float64(name):
    """the float32 arithmetic the kernels reproduce holds the project's parity bar against the same algorithm in double
    (the values seen are recorded in docs/kernels/spdhg.md)"""
    (f32, _), (f64, _) = SK.run(name, "float32"), SK.run(name, "float64")
    for n in SK.COUNTS:
        r = S.rel_l2(f32[n], f64[n])
        print(f"SPDHG {name} m = {SK.SUBSETS[name]} after {n} epochs: float32 vs float64 rel-L2 = {r:.2e}")
        assert f32[n].dtype == np.float32 and f64[n].dtype == np.float64
        assert f32[n].shape == (K.NZ, K.N, K.N)
        assert r <= 1e-5, (name, n, r)


@pytest.mark.parametrize("fidelity, nonneg", [("LS", False), ("KL", True), ("L1", True)])
def test_one_subset_without_tv_is_the_hand_written_loop(fidelity, nonneg):
    """m = 1, no TV: every draw is block 0, and the iterates are the four subset steps written out -- the order dual, z, x
    and the initial clamp"""
    f = np.float32
    op = SK.matched(1)
    b = np.array(K.sinogram(positive=fidelity == "KL"))
    L = f(K.lipschitz())
    assert not S.draws(3, 1, False, 7).any()
    x0 = (0.3 * np.random.default_rng(5).standard_normal((K.NZ, K.N, K.N))).astype(f)
    got = S.spdhg_many(op, b, L, 1, (1, 2, 5), fidelity=fidelity, nonneg=nonneg, x0=x0, seed=3)
    sigma = f(0.95) / np.sqrt(L)
    tau = f(0.95) / (f(1) * np.sqrt(L))
    x = np.where(x0 < 0, f(0), x0) if nonneg else x0.copy()
    assert (x0 < 0).any()
    z, y = np.zeros_like(x), np.zeros_like(b)
    for n in range(1, 6):
        r = op.fp(x)
        v = P.sino_dual(y, r, b, fidelity, sigma)
        d, y = v - y, v
        delta = op.bp(d)
        z = z + delta
        zb = z + f(1) * delta
        x = x - tau * zb
        if nonneg:
            x = np.where(x < 0, f(0), x)
        if n in got:
            assert x.dtype == got[n].dtype == f
            assert np.array_equal(x.view(np.uint32), got[n].view(np.uint32)), (fidelity, n)


@pytest.mark.parametrize("name", list(SK.SUBSETS))
def test_z_is_the_back_projection_of_the_duals(name):
    """z = sum_j A_j^T y_j - div q, recomputed from the final y and q in float64"""
    kw, _ = K.CASES[name]
    m = SK.SUBSETS[name]
    _, state = SK.run(name, "float64")
    op = SK.dense(m)
    want = sum(op.bp(state["y"][j], j) for j in range(m))
    if kw["lam"] is not None:
        want = want - S.divergence(state["q"])
    err = S.rel_l2(state["z"], want)
    print(f"SPDHG {name}: |z - (sum A_j^T y_j - div q)| / |.| = {err:.2e}; block updates {state['block_updates']}")
    assert err <= 1e-10, (name, err)
    E = S.n_blocks(m, kw["lam"] is not None)
    assert sum(state["block_updates"]) == max(SK.COUNTS) * E
    assert (state["block_updates"][1] > 0) == (kw["lam"] is not None)


# SPDHG case -> the PDHG iteration count its 100 epochs are held against
OBJECTIVE_AGAINST = {"LS+TV": 300, "L1+TV": 300, "KL+TV": 300, "LS": 100}


@pytest.mark.parametrize("name", list(OBJECTIVE_AGAINST))
def test_objective_after_100_epochs_is_below_pdhg(name):
    """F(Ax) + lambda TV(x) in float64: 100 epochs (the projector work of 100 PDHG iterations) end below PDHG after 300
    iterations with TV, after 100 without (m = 8; KL: m = 4)"""
    kw, positive = K.CASES[name]
    b = K.sinogram(positive=positive)
    its, _ = SK.run(name, "float64")
    pd = K.run(name, "float64", K.CHECKPOINTS)[OBJECTIVE_AGAINST[name]]
    obj = {n: P.objective(K.dense(), its[n], b, kw["fidelity"], kw["lam"]) for n in SK.COUNTS}
    ref = P.objective(K.dense(), pd, b, kw["fidelity"], kw["lam"])
    print(f"SPDHG {name} m = {SK.SUBSETS[name]}: objective after {SK.COUNTS} epochs = {['%.9g' % obj[n] for n in SK.COUNTS]}; "
          f"PDHG after {OBJECTIVE_AGAINST[name]} iterations = {ref:.9g}")
    assert np.isfinite(obj[100]) and np.isfinite(ref)
    assert obj[100] < ref, (name, obj, ref)


def test_subset_0_has_the_largest_norm_and_the_others_lie_close():
    """what the default lipschitz_const is the maximum of: recorded for docs/kernels/spdhg.md"""
    for m in (4, 8):
        norms = SK.subset_norms(m)
        print(f"SPDHG subset norms m = {m}: {['%.2f' % v for v in norms]}")
        assert SK.lipschitz(m) == max(norms) and min(norms) >= 0.9 * max(norms)


# ------------------------------------------------------------------------------------------------ host surface
def _self(**kw):
    base = dict(Atools=types.SimpleNamespace(device_index=0), OS_number=4, slab=None, adjoint="matched", nonneg_regul=0)
    return types.SimpleNamespace(**dict(base, **kw))


def _dicts(data=None, algo=None, reg=None, method_run="SPDHG", me=None):
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
    assert a["iterations"] == 100 and a["PDHG_ratio"] == 1.0 and a["SPDHG_seed"] == 0
    assert (a["nonnegativity"], a["initialise"], a["recon_mask_radius"], a["tolerance"], a["verbose"]) == (False, None, 1.0, 0.0, False)
    assert "lipschitz_const" not in a          # the driver takes it from the power method on every subset
    assert r == {"method": None}
    assert _dicts(me=_self(OS_number=1))[1]["iterations"] == 100
    d, a, r = _dicts({"data_fidelity": "L1"}, {"iterations": 7, "PDHG_ratio": 4, "SPDHG_seed": 11}, {"method": "PD_TV"})
    assert d["data_fidelity"] == "L1" and a["iterations"] == 7 and a["PDHG_ratio"] == 4 and a["SPDHG_seed"] == 11
    assert r == {"method": "PD_TV", "regul_param": 0.001, "methodTV": 0}   # nothing else is read, nothing else is filled
    _, _, r = _dicts({"data_fidelity": "KL"}, None, {"method": "PD_TV", "regul_param": 0.3, "methodTV": 1})
    assert r["regul_param"] == 0.3 and r["methodTV"] == 1
    assert _dicts(algo={"SPDHG_seed": np.int64(5)})[1]["SPDHG_seed"] == 5


REFUSED = [
    ("unmatched adjoint", dict(me=_self(adjoint="unmatched")), 'SPDHG needs .* construct with adjoint="matched"'),
    ("z-slab", dict(me=_self(slab=object())), "SPDHG is not available in z-slab"),
    ("PWLS", dict(data={"data_fidelity": "PWLS"}), "SPDHG supports .*PWLS"),
    ("SWLS", dict(data={"data_fidelity": "SWLS"}), "SPDHG supports .*SWLS"),
    ("ring key", dict(data={"ringGH_lambda": 0.01}), "ringGH_lambda"),
    ("huber", dict(data={"huber_threshold": 1.0}), "huber_threshold"),
    ("studentst", dict(data={"studentst_threshold": 1.0}), "studentst_threshold"),
    ("unknown fidelity", dict(data={"data_fidelity": "Huber"}), "data_fidelity"),
    ("ROF_TV", dict(reg={"method": "ROF_TV"}), "SPDHG takes .* None or 'PD_TV'"),
    ("TGV", dict(reg={"method": "TGV"}), "None or 'PD_TV'"),
    ("wavelets suffix", dict(reg={"method": "PD_TV_WAVELETS"}), "None or 'PD_TV'"),
    ("NLTV", dict(reg={"method": "NLTV"}), "None or 'PD_TV'"),
    ("slicewise", dict(reg={"method": "PD_TV", "slicewise": True}), "SPDHG does not support slicewise"),
    ("half precision", dict(reg={"method": "PD_TV", "half_precision": True}), "SPDHG does not support half_precision"),
    ("ratio 0", dict(algo={"PDHG_ratio": 0.0}), "PDHG_ratio"),
    ("ratio nan", dict(algo={"PDHG_ratio": float("nan")}), "PDHG_ratio"),
    ("seed negative", dict(algo={"SPDHG_seed": -1}), "SPDHG_seed"),
    ("seed float", dict(algo={"SPDHG_seed": 1.5}), "SPDHG_seed"),
    ("seed bool", dict(algo={"SPDHG_seed": True}), "SPDHG_seed"),
    ("lambda 0", dict(reg={"method": "PD_TV", "regul_param": 0.0}), "regul_param"),
    ("methodTV 2", dict(reg={"method": "PD_TV", "methodTV": 2}), "methodTV"),
]


@pytest.mark.parametrize("what, kw, text", REFUSED, ids=[r[0] for r in REFUSED])
def test_dicts_check_refusals(what, kw, text):
    with pytest.raises(ValueError, match=text):
        _dicts(**kw)


def test_pdhg_and_the_other_drivers_keep_their_dictionaries():
    with pytest.raises(ValueError, match="There is no ordered-subsets implementation of PDHG, please set OS_number=None"):
        _dicts(method_run="PDHG")
    a = _dicts(method_run="PDHG", me=_self(OS_number=1))[1]
    assert a["iterations"] == 500 and "SPDHG_seed" not in a
    for driver in ("FISTA", "ADMM", "OSEM"):
        with pytest.raises(ValueError, match="should be provided as 'LS', 'PWLS', 'KL'"):
            _dicts({"data_fidelity": "L1"}, method_run=driver)
        assert "SPDHG_seed" not in _dicts(method_run=driver)[1]


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
        obj.__dict__.update(dict(Atools=Tools(), _slab=None, _OS_number=4, _objsize_user_given=None), **kw)
        return obj

    monkeypatch.setattr(M.ops, "to_device", lambda x, index: x)
    data = {"projection_data": torch.zeros((4, 5, 6), dtype=torch.float32)}
    unmatched = rt()
    unmatched.Atools.adjoint = "unmatched"
    for obj, d, algo, reg, text in ((unmatched, {}, {}, None, 'adjoint="matched"'),
                                    (rt(_slab=object()), {}, {}, None, "z-slab"),
                                    (rt(), {"data_fidelity": "PWLS"}, {}, None, "PWLS"),
                                    (rt(), {"huber_threshold": 1.0}, {}, None, "huber_threshold"),
                                    (rt(), {}, {"SPDHG_seed": -3}, None, "SPDHG_seed"),
                                    (rt(), {}, {}, {"method": "ROF_TV"}, "None or 'PD_TV'"),
                                    (rt(), {}, {}, {"method": "PD_TV", "slicewise": True}, "slicewise"),
                                    (rt(), {}, {}, {"method": "PD_TV", "half_precision": True}, "half_precision")):
        with pytest.raises(ValueError, match=text):
            obj.SPDHG(dict(data, **d), dict({"iterations": 1}, **algo), reg)
    assert calls == []


# ------------------------------------------------------------------------------------------------ C-ABI
def test_scratch_bytes_is_the_placed_block_of_the_work_arrays():
    from tomobar_amd import _lib, ops
    lib = _lib.lib()
    skew = ops.ARRAY_SKEW
    for dx, dy, dz in [(37, 13, 7), (64, 64, 64), (1, 1, 1), (200, 150, 40)]:
        arr3 = (dx * dy * dz * 4 + 255) // 256 * 256
        arr2 = (dx * dy * 4 + 255) // 256 * 256
        assert lib.tomo_spdhg_scratch_bytes(dx, dy, dz, 3) == 8 * (arr3 + skew)   # z, delta, q1..q3, e1..e3
        assert lib.tomo_spdhg_scratch_bytes(dx, dy, dz, 2) == 6 * (arr2 + skew)   # dz is ignored in 2D
    assert ops.SPDHG_SLOT not in {ops.PDHG_SLOT} | {k.slot for k in ops.BY_NAME.values()}


def test_invalid_arguments_are_refused_before_the_device_is_touched():
    from tomobar_amd import _lib
    lib = _lib.lib()
    p = [C.c_void_p(0x1000 * k) for k in range(1, 9)]   # never dereferenced: every case fails validation
    nul = C.c_void_p(0)

    def sino(y=p[0], r=p[1], b=p[2], n=16, fid=0, sigma=0.5):
        return lib.tomo_spdhg_sino_dual(y, r, b, n, fid, sigma, None)

    def primal(x=p[0], z=p[1], delta=p[2], n=16, tau=0.5, w=4.0):
        return lib.tomo_spdhg_primal(x, z, delta, n, tau, w, 0, None)

    def dual(x=p[0], q1=p[1], q2=p[2], q3=p[3], e1=p[4], e2=p[5], e3=p[6], dx=4, dy=4, dz=4, nd=3, sigma=0.5, lam=1.0, m=0):
        return lib.tomo_spdhg_tv_dual(0, x, q1, q2, q3, e1, e2, e3, dx, dy, dz, nd, sigma, lam, m, None)

    def tvp(x=p[0], z=p[1], e1=p[2], e2=p[3], e3=p[4], dx=4, dy=4, dz=4, nd=3, tau=0.5, w=2.0):
        return lib.tomo_spdhg_tv_primal(0, x, z, e1, e2, e3, dx, dy, dz, nd, tau, w, 0, None)

    bad = [(sino, dict(fid=3)), (sino, dict(fid=-1)), (sino, dict(sigma=0.0)), (sino, dict(sigma=float("nan"))),
           (sino, dict(y=nul)), (sino, dict(r=nul)), (sino, dict(r=p[0])), (sino, dict(b=p[0])), (sino, dict(b=p[1])),
           (primal, dict(tau=0.0)), (primal, dict(tau=float("inf"))), (primal, dict(w=0.0)), (primal, dict(w=-2.0)),
           (primal, dict(x=nul)), (primal, dict(delta=nul)), (primal, dict(z=p[0])), (primal, dict(delta=p[1])),
           (dual, dict(nd=1)), (dual, dict(nd=4)), (dual, dict(dx=0)), (dual, dict(dy=-1)), (dual, dict(dz=0)),
           (dual, dict(sigma=0.0)), (dual, dict(lam=0.0)), (dual, dict(lam=-1.0)), (dual, dict(m=2)), (dual, dict(q3=nul)),
           (dual, dict(e3=nul)), (dual, dict(e1=nul)), (dual, dict(q1=p[0])), (dual, dict(e2=p[2])), (dual, dict(e1=p[0])),
           (dual, dict(x=nul)),
           (tvp, dict(nd=5)), (tvp, dict(dx=0)), (tvp, dict(tau=0.0)), (tvp, dict(w=float("nan"))), (tvp, dict(x=nul)),
           (tvp, dict(z=p[0])), (tvp, dict(e1=p[1])), (tvp, dict(e3=nul)), (tvp, dict(e2=p[2]))]
    for fn, kw in bad:
        assert fn(**kw) == _lib.E_INVALID, (fn.__name__, kw)
        with pytest.raises(ValueError):
            _lib.check(fn(**kw))
    assert sino(n=0) == _lib.OK and primal(n=0) == _lib.OK   # nothing to do, nothing launched
    # nd = 2 ignores the third fields, aliasing ones included: only the device call can fail from here on
    assert dual(nd=2, q3=nul, e3=nul, dx=0) == _lib.E_INVALID
