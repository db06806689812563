"""NDF without a GPU, what is NDF's own: properties of the numpy restatement (tests/_ndf_oracle.py; the algorithm is the
specification, docs/kernels/ndf.md) and the host surface of the feature -- dictionary defaults, the refusals, the C-ABI's
symbol set and version.  What NDF shares with the other explicit time marches is the suite of tests/_march_oracle_suite.py,
collected at the end of this file."""
import types

import numpy as np
import pytest

import _march_oracle_suite
import _ndf_oracle
from _ndf_oracle import ORACLE as N
from _tgv_oracle import phantom, rel_l2

SHAPE_3D, SHAPE_2D = (7, 13, 37), (13, 37)
COUNTS = (1, 2, 25, 40)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("pname", sorted(N.PARAMS))
@pytest.mark.parametrize("shape", [SHAPE_3D, SHAPE_2D])
def test_float32_against_float64(shape, pname):
    """the float32 arithmetic the kernel reproduces holds the project's parity bar against the same algorithm in double"""
    f32, f64 = N.cached(shape, pname, COUNTS), N.cached(shape, pname, COUNTS, "float64")
    for n in COUNTS:
        r = rel_l2(f32[n], f64[n])
        print(f"NDF {pname} {shape} after {n}: float32 vs float64 rel-L2 = {r:.2e}")
        assert f32[n].dtype == np.float32 and f64[n].dtype == np.float64
        assert r <= 1e-5, (shape, pname, n, r)


@pytest.mark.parametrize("pname", sorted(N.PARAMS))
@pytest.mark.parametrize("shape", [SHAPE_3D, SHAPE_2D])
def test_both_branches_of_every_penalty_are_exercised(shape, pname):
    """a condition on the INPUTS of the GPU tests: at the last iteration between 10 % and 90 % of the forward differences
    exceed sigma"""
    for n in COUNTS:
        stats = {}
        N.run(phantom(shape), iterations=n, stats=stats, **N.PARAMS[pname])
        print(f"NDF {pname} {shape} iteration {n}: |forward difference| > sigma on {stats['above']:.3f}")
        assert 0.10 <= stats["above"] <= 0.90, (pname, shape, n, stats)


def test_tukey_keeps_a_noiseless_step_and_huber_does_not():
    step = np.zeros((6, 8, 12), np.float32)
    step[..., 6:] = 1.0
    kept = N.run(step, iterations=25, penalty="Tukey", lam=1.0, sigma=0.1, tau=0.05)
    assert np.array_equal(_bits(kept), _bits(step)), "Tukey with sigma below the step height must not touch it"
    moved = N.run(step, iterations=25, penalty="Huber", lam=1.0, sigma=0.1, tau=0.05)
    assert not np.array_equal(moved, step)
    assert np.abs(moved - step).max() > 0.05


@pytest.mark.parametrize("penalty", _ndf_oracle.PENALTIES)
def test_backward_flux_is_the_neighbours_forward_flux_with_the_sign_turned(penalty):
    """what the kernel relies on (csrc/ndf_zmarch.inl): g(b - a) has the bits of -g(a - b) -- the penalties are odd and every
    operation in them rounds symmetrically -- except that a zero difference, and Tukey's rejected range, give +0 both ways"""
    rng = np.random.default_rng(7)
    a = (rng.standard_normal(200000) * 3.0).astype(np.float32)
    b = (rng.standard_normal(200000) * 3.0).astype(np.float32)
    b[::17] = a[::17]                                  # zero differences
    a[1::1001] *= np.float32(1e-30)                    # differences whose flux underflows
    b[1::1001] = a[1::1001] * np.float32(1.5)
    for sigma in (np.float32(0.5), np.float32(2.0), np.float32(1e6)):
        t = a - b
        g = _ndf_oracle.flux(t, sigma, penalty)
        rejected = (np.abs(t) > sigma) if penalty == "Tukey" else np.zeros(t.shape, bool)
        gn = np.where((t == 0) | rejected, np.float32(0.0), -g)
        assert np.array_equal(_bits(_ndf_oracle.flux(b - a, sigma, penalty)), _bits(gn)), (penalty, sigma)


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
    r = _dicts({"method": "NDF"})
    assert r["NDF_penalty"] == "Huber" and r["edge_threshold"] == 0.01
    r = _dicts({"method": "NDF", "NDF_penalty": "Tukey", "edge_threshold": 0.3})
    assert r["NDF_penalty"] == "Tukey" and r["edge_threshold"] == 0.3
    for bad in ("huber", "TV", None, 1):
        with pytest.raises(ValueError, match="NDF_penalty"):
            _dicts({"method": "NDF", "NDF_penalty": bad})
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="edge_threshold"):
            _dicts({"method": "NDF", "edge_threshold": bad})
    # dictionaries of the other methods come out as before
    for method in ("PD_TV", "ROF_TV", "TGV", None):
        r = _dicts({"method": method, "regul_param": 0.1})
        assert "NDF_penalty" not in r and "edge_threshold" not in r
    assert set(_dicts({"method": "NDF"})) - set(_dicts({"method": "ROF_TV"})) == {"NDF_penalty", "edge_threshold"}


def test_refusals_half_precision_unknown_method_unknown_penalty():
    import torch
    from tomobar_amd.regularisersCuPy import NDF_cupy, check_prox_available, prox_regul, reserve_prox_scratch
    reg = {"method": "NDF", "regul_param": 1.0, "iterations": 3, "time_marching_step": 0.05, "edge_threshold": 2.0}
    X = torch.zeros((4, 5, 6), dtype=torch.float32)
    with pytest.raises(ValueError, match="half_precision"):
        prox_regul(_self(), X, dict(reg, half_precision=True))
    with pytest.raises(ValueError, match="half_precision"):
        reserve_prox_scratch(_self(), (4, 5, 6), dict(reg, half_precision=True))
    # NDF runs in z-slab mode: no refusal there
    check_prox_available(_self(slab=object()), (4, 5, 6), reg)
    with pytest.raises(ValueError, match="ROF_TV, PD_TV and TGV"):
        prox_regul(_self(), X, dict(reg, method="NLTV"))
    with pytest.raises(ValueError, match="NDF penalty"):
        NDF_cupy(X, 1.0, 2.0, 3, 0.05, "Welsch")
    with pytest.raises(ValueError, match="NDF penalty"):
        prox_regul(_self(), X, dict(reg, NDF_penalty="Welsch"))
    import tomobar_amd
    assert tomobar_amd.NDF_cupy is NDF_cupy


def test_abi_symbols_and_version():
    from tomobar_amd import _lib
    lib = _lib.lib()
    for name in ("tomo_ndf", "tomo_ndf_scratch_bytes", "tomo_ndf_iter_slab_range"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 10 and lib.tomo_abi_version() == 10
    assert _lib.NDF_PENALTY == {"Huber": 0, "PM": 1, "Tukey": 2}
    with _lib.use_flavour("dev") as dev:
        assert hasattr(dev, "tomo_ndf") and dev.tomo_abi_version() == 10


# ------------------------------------------------------------------------------------------------ shared with the other marches
globals().update(_march_oracle_suite.suite("NDF"))
