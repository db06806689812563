"""LLT_ROF without a GPU, what is LLT_ROF's own: properties of the numpy restatement (tests/_llt_rof_oracle.py; the algorithm
is the specification, docs/kernels/llt_rof.md) and the host surface of the feature -- dictionary defaults, the refusals,
ADMM's private copy, the C-ABI's symbol set.  What LLT_ROF shares with the other explicit time marches is the suite of
tests/_march_oracle_suite.py, collected at the end of this file."""
import types

import numpy as np
import pytest

import _march_oracle_suite
from _llt_rof_oracle import ORACLE as D
from _tgv_oracle import phantom, rel_l2

SHAPE_3D, SHAPE_2D = (7, 13, 37), (13, 37)
COUNTS = (1, 2, 25, 40)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("pname", sorted(D.PARAMS))
@pytest.mark.parametrize("shape", [SHAPE_3D, SHAPE_2D])
def test_float32_against_float64(shape, pname):
    """the float32 arithmetic the kernel reproduces holds the project's parity bar against the same algorithm in double.
    Largest values seen: A 2.2e-6, B 1.5e-6, C 1.9e-7 -- larger than the sibling oracles' 1e-7 because E_d is sign-like: a
    second difference at rounding level can take opposite signs in the two precisions."""
    f32, f64 = D.cached(shape, pname, COUNTS), D.cached(shape, pname, COUNTS, "float64")
    for n in COUNTS:
        r = rel_l2(f32[n], f64[n])
        print(f"LLT_ROF {pname} {shape} after {n}: float32 vs float64 rel-L2 = {r:.2e}")
        assert f32[n].dtype == np.float32 and f64[n].dtype == np.float64
        assert r <= 1e-5, (shape, pname, n, r)


@pytest.mark.parametrize("pname", sorted(D.PARAMS))
@pytest.mark.parametrize("shape", [SHAPE_3D, SHAPE_2D])
def test_both_terms_act_in_the_first_and_the_40th_iteration(shape, pname):
    """a condition on the INPUTS of the GPU tests: the full run differs from the runs with either weight set to 1e-30 of
    itself, and from the iterate entering iterations 1 and 40 the step with either weight scaled so differs from the full
    step -- a kernel that dropped or mis-weighted one term could not pass"""
    p = D.PARAMS[pname]
    f = phantom(shape)
    full = D.cached(shape, pname, COUNTS)[40]
    no_rof = D.run(f, 40, lam_rof=np.float32(p["lam_rof"]) * np.float32(1e-30), lam_llt=p["lam_llt"], tau=p["tau"])
    no_llt = D.run(f, 40, lam_rof=p["lam_rof"], lam_llt=np.float32(p["lam_llt"]) * np.float32(1e-30), tau=p["tau"])
    print(f"LLT_ROF {pname} {shape}: rel-L2 of the 40-iteration run to the run without ROF {rel_l2(no_rof, full):.2e}, "
          f"without LLT {rel_l2(no_llt, full):.2e}")
    assert rel_l2(no_rof, full) > 1e-5 and rel_l2(no_llt, full) > 1e-5
    its = {0: f}
    its.update(D.many(f, p, (39,)))
    l1, l2, tau = np.float32(p["lam_rof"]), np.float32(p["lam_llt"]), np.float32(p["tau"])
    tiny = np.float32(1e-30)
    for n in (1, 40):
        U = its[n - 1]
        want = D.step(U, f, l1, l2, tau)
        assert not np.array_equal(D.step(U, f, l1 * tiny, l2, tau), want), (pname, n, "the ROF term does nothing")
        assert not np.array_equal(D.step(U, f, l1, l2 * tiny, tau), want), (pname, n, "the LLT term does nothing")


def test_the_operator_changes_a_noisy_input():
    f = phantom(SHAPE_3D)
    for pname in D.PARAMS:
        for n in COUNTS:
            out = D.cached(SHAPE_3D, pname, COUNTS)[n]
            assert np.all(np.isfinite(out)) and not np.array_equal(out, f), (pname, n)
        assert rel_l2(D.cached(SHAPE_3D, pname, COUNTS)[40], f) > rel_l2(D.cached(SHAPE_3D, pname, COUNTS)[1], f) > 0.0


def test_one_step_is_bounded_by_the_fluxes():
    """|U' - c| <= tau (4 nd lam_llt + 2 nd lam_rof + |c - f|): the fluxes are bounded by 1 (a little slack for the roundings)"""
    for shape in (SHAPE_3D, SHAPE_2D):
        nd = len(shape)
        for pname, p in D.PARAMS.items():
            f = phantom(shape).astype(np.float64)
            U = D.cached(shape, pname, COUNTS)[25].astype(np.float64)
            new = D.step(U, f, p["lam_rof"], p["lam_llt"], p["tau"])
            bound = p["tau"] * (4 * nd * p["lam_llt"] + 2 * nd * p["lam_rof"] + np.abs(U - f))
            assert np.all(np.abs(new - U) <= bound * (1 + 1e-6)), (shape, pname)


def test_terraces_stay_finite_and_reach_the_zero_paths():
    """exact zeros and ties: 0 / (0 + eps) and 0 / sqrt(eps) give exact zeros, no masked branch"""
    from _edge_shapes import terraces
    stats = {}
    out = D.run(terraces((20, 24, 70)), iterations=3, stats=stats, **D.PARAMS["A"])
    print(f"LLT_ROF terraces (20, 24, 70): s == 0 on {stats['s_zero', 1]:.3f} / {stats['s_zero', 3]:.4f} of the voxels entering "
          f"iterations 1 / 3, |h1| < 1e-6 on {stats['h1_tiny', 1]:.3f}")
    assert np.all(np.isfinite(out))
    assert stats["s_zero", 1] >= 0.25 and stats["h1_tiny", 1] >= 0.25


def test_stitched_slabs_with_a_slab_of_exactly_two_planes():
    f = phantom(SHAPE_3D)
    want = D.cached(SHAPE_3D, "A", COUNTS)[2]
    for bounds in ([(0, 2), (2, 7)], [(0, 5), (5, 7)], [(0, 3), (3, 5), (5, 7)], [(0, 2), (2, 4), (4, 7)]):
        got = D.by_slabs(f, D.PARAMS["A"], 2, len(bounds), bounds)
        assert np.array_equal(_bits(got), _bits(want)), bounds


def test_two_ghost_planes_are_needed():
    """slabs (0,2),(2,5),(5,9) of a (9,7,11) volume: two ghost planes reproduce the whole volume, one does not (the stencil
    has radius 2)"""
    f = phantom((9, 7, 11))
    bounds = [(0, 2), (2, 5), (5, 9)]
    for pname, params in D.PARAMS.items():
        want = D.run(f, iterations=6, **params)
        assert np.array_equal(_bits(D.by_slabs(f, params, 6, 3, bounds)), _bits(want)), pname
        assert not np.array_equal(_bits(D.by_slabs(f, params, 6, 3, bounds, ghost=1)), _bits(want)), pname


# ------------------------------------------------------------------------------------------------ host surface
def _self(slab=None):
    return types.SimpleNamespace(Atools=types.SimpleNamespace(device_index=0), OS_number=1, slab=slab, nonneg_regul=0)


def _dicts(reg, method_run="FISTA"):
    from tomobar_amd.supp.dicts import dicts_check
    import torch
    data = {"projection_data": torch.zeros((2, 3, 4), dtype=torch.float32)}
    import tomobar_amd.ops as ops
    keep = ops.to_device
    ops.to_device = lambda x, index: x   # no GPU here: the projections stay where they are
    try:
        return dicts_check(_self(), data, {}, reg, method_run=method_run)[2]
    finally:
        ops.to_device = keep


def test_dicts_check_defaults_and_errors():
    r = _dicts({"method": "LLT_ROF"})
    assert r["regul_param2"] == 0.001 and "NDF_penalty" not in r and "edge_threshold" not in r
    assert _dicts({"method": "LLT_ROF", "regul_param2": 0.3})["regul_param2"] == 0.3
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="regul_param2"):
            _dicts({"method": "LLT_ROF", "regul_param2": bad})
    # dictionaries of the other methods come out as before
    for method in ("PD_TV", "ROF_TV", "TGV", "NDF", "Diff4th", None):
        r = _dicts({"method": method, "regul_param": 0.1})
        assert "regul_param2" not in r
        r = _dicts({"method": method, "regul_param": 0.1, "regul_param2": -1.0})   # not this method's key: not checked
        assert r["regul_param2"] == -1.0
    assert set(_dicts({"method": "LLT_ROF"})) - set(_dicts({"method": "ROF_TV"})) == {"regul_param2"}
    assert set(_dicts({"method": "Diff4th"})) - set(_dicts({"method": "ROF_TV"})) == {"edge_threshold"}
    assert set(_dicts({"method": "NDF"})) - set(_dicts({"method": "ROF_TV"})) == {"NDF_penalty", "edge_threshold"}


def test_admm_divides_both_weights_on_its_own_copy():
    """ADMM hands prox_regul regul_param / rho AND regul_param2 / rho (both multiply the regulariser) and leaves the
    caller's dictionary as it was.  The driver's set-up is replaced by a stub and the loop is left at its first allocation:
    what is under test is the dictionary ADMM builds before it, read from ADMM's frame."""
    import traceback
    import torch
    from tomobar_amd.methodsIR_CuPy import RecToolsIRCuPy

    class Stop(Exception):
        pass

    def init(_data_, _algorithm_, _regularisation_, name):
        assert name == "ADMM"
        algo = {"nonnegativity": False, "ADMM_rho_const": 4.0, "ADMM_relax_par": 1.6, "lipschitz_const": 1.0}
        return ({"projection_data": None}, algo, _regularisation_, torch.zeros((2, 3, 3)), None, False)

    def new_vol(*a):
        raise Stop

    me = types.SimpleNamespace(Atools=None, data_fidelity="LS", _new_vol=new_vol)
    setattr(me, "_RecToolsIRCuPy__common_initialisation", init)

    def local_copy(reg):
        with pytest.raises(Stop) as ei:
            RecToolsIRCuPy.ADMM(me, {}, {}, reg)
        return next(f.f_locals["r_local"] for f, _ in traceback.walk_tb(ei.value.__traceback__) if f.f_code.co_name == "ADMM")

    reg = {"method": "LLT_ROF", "regul_param": 0.5, "regul_param2": 0.25, "iterations": 3, "time_marching_step": 0.01}
    keep = dict(reg)
    local = local_copy(reg)
    assert reg == keep and local is not reg
    assert local["regul_param"] == 0.125 and local["regul_param2"] == 0.0625
    assert {k: v for k, v in local.items() if not k.startswith("regul_param")} == {k: v for k, v in keep.items() if not k.startswith("regul_param")}
    # a second weight a caller left in another method's dictionary is not touched
    local = local_copy(dict(reg, method="ROF_TV"))
    assert local["regul_param"] == 0.125 and local["regul_param2"] == 0.25


def test_refusals_half_precision_and_unknown_method():
    import torch
    from tomobar_amd.regularisersCuPy import LLT_ROF_cupy, check_prox_available, prox_regul, reserve_prox_scratch
    reg = {"method": "LLT_ROF", "regul_param": 0.3, "regul_param2": 0.1, "iterations": 3, "time_marching_step": 0.005}
    X = torch.zeros((4, 5, 6), dtype=torch.float32)
    with pytest.raises(ValueError, match="LLT_ROF does not support half_precision"):
        prox_regul(_self(), X, dict(reg, half_precision=True))
    with pytest.raises(ValueError, match="half_precision"):
        reserve_prox_scratch(_self(), (4, 5, 6), dict(reg, half_precision=True))
    with pytest.raises(ValueError, match="half_precision"):
        check_prox_available(_self(), (4, 5, 6), dict(reg, half_precision=True))
    # LLT_ROF runs in z-slab mode: no refusal there
    check_prox_available(_self(slab=object()), (4, 5, 6), reg)
    with pytest.raises(ValueError, match="ROF_TV, PD_TV and TGV.*Diff4th(?s:.*)LLT_ROF"):
        prox_regul(_self(), X, dict(reg, method="NLTV"))
    import tomobar_amd
    assert tomobar_amd.LLT_ROF_cupy is LLT_ROF_cupy
    import inspect
    sig = inspect.signature(LLT_ROF_cupy)
    assert list(sig.parameters) == ["data", "regularisation_parameterROF", "regularisation_parameterLLT", "iterations",
                                    "time_marching_parameter", "gpu_device", "out", "tolerance"]
    assert [p.default for p in list(sig.parameters.values())[1:]] == [1e-05, 1e-05, 1000, 0.001, 0, None, 0.0]


def test_abi_symbols():
    from tomobar_amd import _lib
    lib = _lib.lib()
    names = ("tomo_llt_rof", "tomo_llt_rof_scratch_bytes", "tomo_llt_rof_iter_slab_range")
    for name in names:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.tomo_abi_version() == 10 == _lib.ABI_VERSION
    with _lib.use_flavour("dev") as dev:
        for name in names:
            assert hasattr(dev, name), name
        assert dev.tomo_abi_version() == 10


# ------------------------------------------------------------------------------------------------ shared with the other marches
globals().update(_march_oracle_suite.suite("LLT_ROF"))
