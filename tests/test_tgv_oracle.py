"""TGV without a GPU: properties of the numpy restatement (tests/_tgv_oracle.py; the algorithm is the specification,
docs/kernels/tgv.md) and the host surface of the feature -- dictionary defaults, the refusals, the C-ABI's argument checks
and scratch size (the library loads and validates without a device)."""
import ctypes as C
import types

import numpy as np
import pytest

import _tgv_oracle as T

SHAPE_3D, SHAPE_2D = (7, 13, 37), (13, 37)


# ------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("shape", [SHAPE_3D, SHAPE_2D])
def test_both_projection_branches_are_active(shape):
    """a condition on the INPUTS of the GPU tests: after 40 iterations of A neither projection is always on or always off"""
    stats = {}
    T.tgv(T.phantom(shape), iterations=40, stats=stats, **T.PARAMS_A)
    print(f"TGV A {shape}: n > 1 on {stats['n_gt_1']:.3f}, m > 1 on {stats['m_gt_1']:.3f} of the voxels")
    assert 0.05 <= stats["n_gt_1"] <= 0.95, stats
    assert 0.05 <= stats["m_gt_1"] <= 0.95, stats
    T.tgv(T.phantom(shape), iterations=40, stats=stats, **T.PARAMS_B)
    print(f"TGV B {shape}: m > 1 on {stats['m_gt_1']:.3f} of the voxels")
    assert stats["m_gt_1"] > 0.9, stats


@pytest.mark.parametrize("pname", ["A", "B"])
@pytest.mark.parametrize("shape", [SHAPE_3D, SHAPE_2D])
def test_float32_against_float64(shape, pname):
    """the float32 arithmetic the kernels reproduce holds the project's parity bar against the same algorithm in double"""
    counts = (1, 2, 25, 40)
    f32, f64 = T.cached(shape, pname, counts), T.cached(shape, pname, counts, "float64")
    for n in counts:
        r = T.rel_l2(f32[n], f64[n])
        print(f"TGV {pname} {shape} after {n}: float32 vs float64 rel-L2 = {r:.2e}")
        assert f32[n].dtype == np.float32 and f64[n].dtype == np.float64
        assert r <= 1e-5, (shape, pname, n, r)


@pytest.mark.parametrize("shape", [(5, 6, 7), (6, 7)])
def test_constant_input(shape):
    c = np.float32(37.25)
    out = T.tgv(np.full(shape, c, np.float32), iterations=25, **T.PARAMS_A)
    assert np.all(out.view(np.uint32) == out.view(np.uint32).flat[0]), "the output of a constant input is not constant"
    assert abs(float(out.flat[0]) - float(c)) <= 1e-6 * float(c)


def test_z_replicated_volume_equals_the_2d_run():
    plane = T.phantom(SHAPE_2D)
    vol = np.ascontiguousarray(np.broadcast_to(plane, (5,) + SHAPE_2D))
    for params in (T.PARAMS_A, T.PARAMS_B):
        want = T.tgv(plane, iterations=25, **params)
        got = T.tgv(vol, iterations=25, **params)
        for z in range(vol.shape[0]):
            assert np.array_equal(got[z].view(np.uint32), want.view(np.uint32)), z


def test_zero_iterations_and_a_dimension_of_one():
    f = T.phantom((1, 5, 3))
    assert np.array_equal(T.tgv(f, iterations=0, **T.PARAMS_A), f)
    # along an axis of extent 1 F is 0 and B the identity: finite output
    assert np.all(np.isfinite(T.tgv(f, iterations=7, **T.PARAMS_A)))


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
    r = _dicts({"method": "TGV"})
    assert r["TGV_alpha1"] == 1.0 and r["TGV_alpha2"] == 2.0 and r["PD_LipschitzConstant"] == 12.0
    r = _dicts({"method": "TGV", "TGV_alpha1": 0.5, "TGV_alpha2": 3.0})
    assert r["TGV_alpha1"] == 0.5 and r["TGV_alpha2"] == 3.0
    for key in ("TGV_alpha1", "TGV_alpha2"):
        for bad in (0.0, -1.0, float("nan")):
            with pytest.raises(ValueError, match=key):
                _dicts({"method": "TGV", key: bad})
    # dictionaries of the other methods come out as before
    for method in ("PD_TV", "ROF_TV", None):
        r = _dicts({"method": method, "regul_param": 0.1})
        assert "TGV_alpha1" not in r and "TGV_alpha2" not in r


def test_refusals_slab_half_precision_unknown_method():
    import torch
    from tomobar_amd.regularisersCuPy import check_prox_available, prox_regul, reserve_prox_scratch
    reg = {"method": "TGV", "regul_param": 1.0, "iterations": 3, "PD_LipschitzConstant": 12.0}
    slab_self = _self(slab=object())
    X = torch.zeros((4, 5, 6), dtype=torch.float32)
    with pytest.raises(ValueError, match="TGV is not available in z-slab mode"):
        prox_regul(slab_self, X, reg)
    with pytest.raises(ValueError, match="TGV is not available in z-slab mode"):
        reserve_prox_scratch(slab_self, (4, 5, 6), reg)
    check_prox_available(slab_self, (1, 5, 6), reg)      # a single slice is not a real 3D volume
    check_prox_available(slab_self, (4, 5, 6), dict(reg, method="PD_TV"))
    with pytest.raises(ValueError, match="half_precision"):
        prox_regul(_self(), X, dict(reg, half_precision=True))
    with pytest.raises(ValueError, match="half_precision"):
        reserve_prox_scratch(_self(), (4, 5, 6), dict(reg, half_precision=True))
    with pytest.raises(ValueError, match="ROF_TV, PD_TV and TGV"):
        prox_regul(_self(), X, dict(reg, method="NLTV"))


def test_drivers_refuse_tgv_in_slab_mode_before_any_projector_call(monkeypatch):
    """the refusal comes from the set-up: neither the power method nor a projection runs"""
    import torch
    from tomobar_amd import methodsIR_CuPy as M
    calls = []

    class Tools:
        device_index, slab, detectors_x_pad = 0, None, 0
        def vol_shape(self): return (4, 6, 6)
        def sino_shape(self, sub): return (4, 5, 6)
        def __getattr__(self, name):
            calls.append(name)
            raise AssertionError(f"projector attribute {name} touched")

    rt = M.RecToolsIRCuPy.__new__(M.RecToolsIRCuPy)
    rt.__dict__.update(Atools=Tools(), _slab=object(), _OS_number=1, _objsize_user_given=None)
    monkeypatch.setattr(M.ops, "to_device", lambda x, index: x)
    data = {"projection_data": torch.zeros((4, 5, 6), dtype=torch.float32)}
    for driver in ("FISTA", "ADMM", "OSEM"):
        with pytest.raises(ValueError, match="TGV is not available in z-slab mode"):
            getattr(rt, driver)(dict(data), {"iterations": 1}, {"method": "TGV"})
    assert calls == []


def _lib():
    from tomobar_amd import _lib
    return _lib.lib()


def test_scratch_bytes():
    lib = _lib()
    skew = 69888   # the array skew (ops.ARRAY_SKEW)
    from tomobar_amd import ops
    assert ops.ARRAY_SKEW == skew
    for dx, dy, dz in [(37, 13, 7), (64, 64, 64), (1, 1, 1), (200, 150, 40)]:
        arr3 = (dx * dy * dz * 4 + 255) // 256 * 256
        arr2 = (dx * dy * 4 + 255) // 256 * 256
        assert lib.tomo_tgv_scratch_bytes(dx, dy, dz, 3) == 16 * (arr3 + skew)
        assert lib.tomo_tgv_scratch_bytes(dx, dy, dz, 2) == 10 * (arr2 + skew)   # dz is ignored in 2D


def test_invalid_arguments_are_refused_before_the_device_is_touched():
    from tomobar_amd import _lib
    lib = _lib.lib()
    a, b = C.c_void_p(0x1000), C.c_void_p(0x2000)   # never dereferenced: every case fails validation

    def call(inp=a, out=b, dx=4, dy=4, dz=4, nd=3, lam=1.0, a1=1.0, a0=2.0, iters=3, tol=0.0):
        return lib.tomo_tgv(0, inp, out, dx, dy, dz, nd, lam, a1, a0, 0.25, 0.25, iters, tol, None, None, None)

    bad = [dict(out=a), dict(nd=1), dict(nd=4), dict(dx=0), dict(dy=0), dict(dz=0), dict(dx=-3), dict(lam=0.0), dict(lam=-1.0),
           dict(a1=0.0), dict(a0=0.0), dict(a0=-2.0), dict(iters=-1), dict(tol=-1e-3), dict(tol=float("inf")),
           dict(tol=float("nan")), dict(nd=2, dy=0)]
    for kw in bad:
        assert call(**kw) == _lib.E_INVALID, kw
        with pytest.raises(ValueError):
            _lib.check(call(**kw))


def test_the_tolerance_case_of_the_gpu_tests_satisfies_its_rule():
    tol, stop, d_stop, seq = T.tolerance_plan()
    print(f"TGV tolerance case: sequence {['%.3e' % v for v in seq]}, tol {tol:.4e}, stops after {stop}")
    assert stop == 24 and d_stop < tol < seq[2]
