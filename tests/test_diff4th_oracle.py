"""Diff4th without a GPU, what is Diff4th's own: properties of the numpy restatement (tests/_diff4th_oracle.py; the algorithm
is the specification, docs/kernels/diff4th.md) and the host surface of the feature -- dictionary defaults, the refusals, the
C-ABI's symbol set.  What Diff4th shares with the other explicit time marches is the suite of tests/_march_oracle_suite.py,
collected at the end of this file."""
import types

import numpy as np
import pytest

import _march_oracle_suite
import _diff4th_oracle
from _diff4th_oracle import ORACLE as D
from _tgv_oracle import phantom, rel_l2

SHAPE_3D, SHAPE_2D = (7, 13, 37), (13, 37)
COUNTS = (1, 2, 25, 40)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("pname", sorted(D.PARAMS))
@pytest.mark.parametrize("shape", [SHAPE_3D, SHAPE_2D])
def test_float32_against_float64(shape, pname):
    """the float32 arithmetic the kernel reproduces holds the project's parity bar against the same algorithm in double"""
    f32, f64 = D.cached(shape, pname, COUNTS), D.cached(shape, pname, COUNTS, "float64")
    for n in COUNTS:
        r = rel_l2(f32[n], f64[n])
        print(f"Diff4th {pname} {shape} after {n}: float32 vs float64 rel-L2 = {r:.2e}")
        assert f32[n].dtype == np.float32 and f64[n].dtype == np.float64
        assert r <= 1e-5, (shape, pname, n, r)


@pytest.mark.parametrize("pname", sorted(D.PARAMS))
@pytest.mark.parametrize("shape", [SHAPE_3D, SHAPE_2D])
def test_the_edge_weight_is_active_on_part_of_the_voxels(shape, pname):
    """a condition on the INPUTS of the GPU tests: at the first and the last of 40 iterations between 10 % and 90 % of the
    voxels have G / s2 > 1 (cw below one half), so both regimes of the weight are exercised"""
    stats = {}
    D.run(phantom(shape), iterations=40, stats=stats, **D.PARAMS[pname])
    print(f"Diff4th {pname} {shape}: G/s2 > 1 on {stats['active', 1]:.3f} of the voxels in iteration 1, {stats['active', 40]:.3f} in iteration 40")
    for n in (1, 40):
        assert 0.10 <= stats["active", n] <= 0.90, (pname, shape, n, stats["active", n])


def test_parameter_sets_meet_the_stability_bound_and_one_has_lambda_other_than_one():
    assert 3 <= len(D.PARAMS) <= 4
    for pname, p in D.PARAMS.items():
        assert _diff4th_oracle.stable(p["lam"], p["tau"], 3) and _diff4th_oracle.stable(p["lam"], p["tau"], 2), pname
    assert any(p["lam"] != 1.0 for p in D.PARAMS.values())


def test_the_operator_changes_a_noisy_input():
    f = phantom(SHAPE_3D)
    for pname in D.PARAMS:
        for n in COUNTS:
            out = D.cached(SHAPE_3D, pname, COUNTS)[n]
            assert np.all(np.isfinite(out)) and not np.array_equal(out, f), (pname, n)
        assert rel_l2(D.cached(SHAPE_3D, pname, COUNTS)[40], f) > rel_l2(D.cached(SHAPE_3D, pname, COUNTS)[1], f) > 0.0


def test_stitched_slabs_with_a_slab_of_exactly_two_planes():
    f = phantom(SHAPE_3D)
    want = D.cached(SHAPE_3D, "A", COUNTS)[2]
    for bounds in ([(0, 2), (2, 7)], [(0, 5), (5, 7)], [(0, 3), (3, 5), (5, 7)], [(0, 2), (2, 4), (4, 7)]):
        got = D.by_slabs(f, D.PARAMS["A"], 2, len(bounds), bounds)
        assert np.array_equal(_bits(got), _bits(want)), bounds


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
    r = _dicts({"method": "Diff4th"})
    assert r["edge_threshold"] == 0.01 and "NDF_penalty" not in r
    assert _dicts({"method": "Diff4th", "edge_threshold": 0.3})["edge_threshold"] == 0.3
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="edge_threshold"):
            _dicts({"method": "Diff4th", "edge_threshold": bad})
    # dictionaries of the other methods come out as before
    for method in ("PD_TV", "ROF_TV", "TGV", None):
        r = _dicts({"method": method, "regul_param": 0.1})
        assert "NDF_penalty" not in r and "edge_threshold" not in r
        r = _dicts({"method": method, "regul_param": 0.1, "edge_threshold": -1.0})   # not this method's key: not checked
        assert r["edge_threshold"] == -1.0
    assert set(_dicts({"method": "Diff4th"})) - set(_dicts({"method": "ROF_TV"})) == {"edge_threshold"}
    assert set(_dicts({"method": "NDF"})) - set(_dicts({"method": "ROF_TV"})) == {"NDF_penalty", "edge_threshold"}


def test_refusals_half_precision_and_unknown_method():
    import torch
    from tomobar_amd.regularisersCuPy import Diff4th_cupy, check_prox_available, prox_regul, reserve_prox_scratch
    reg = {"method": "Diff4th", "regul_param": 1.0, "iterations": 3, "time_marching_step": 0.005, "edge_threshold": 2.0}
    X = torch.zeros((4, 5, 6), dtype=torch.float32)
    with pytest.raises(ValueError, match="Diff4th does not support half_precision"):
        prox_regul(_self(), X, dict(reg, half_precision=True))
    with pytest.raises(ValueError, match="half_precision"):
        reserve_prox_scratch(_self(), (4, 5, 6), dict(reg, half_precision=True))
    with pytest.raises(ValueError, match="half_precision"):
        check_prox_available(_self(), (4, 5, 6), dict(reg, half_precision=True))
    # Diff4th runs in z-slab mode: no refusal there
    check_prox_available(_self(slab=object()), (4, 5, 6), reg)
    with pytest.raises(ValueError, match="ROF_TV, PD_TV and TGV.*Diff4th"):
        prox_regul(_self(), X, dict(reg, method="NLTV"))
    import tomobar_amd
    assert tomobar_amd.Diff4th_cupy is Diff4th_cupy
    import inspect
    sig = inspect.signature(Diff4th_cupy)
    assert list(sig.parameters) == ["data", "regularisation_parameter", "edge_parameter", "iterations",
                                    "time_marching_parameter", "gpu_id", "out", "tolerance"]
    assert [p.default for p in list(sig.parameters.values())[1:]] == [1e-05, 0.01, 1000, 0.001, 0, None, 0.0]


def test_abi_symbols():
    from tomobar_amd import _lib
    lib = _lib.lib()
    for name in ("tomo_diff4th", "tomo_diff4th_scratch_bytes", "tomo_diff4th_iter_slab_range"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    with _lib.use_flavour("dev") as dev:
        assert hasattr(dev, "tomo_diff4th")


# ------------------------------------------------------------------------------------------------ shared with the other marches
globals().update(_march_oracle_suite.suite("Diff4th"))
