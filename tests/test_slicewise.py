"""The key ``_regularisation_["slicewise"]`` on the host side (no GPU): what prox_regul calls with and without it, in
whole-volume and in z-slab mode, the refusals, the scratch reservation, dicts_check, and what tests/_slicewise_cases.py
promises the GPU file (the input tells slice-wise from 3D TV; the tolerance thresholds have their margins).  The functions
the dispatch ends in are replaced by recorders, as in tests/test_regulariser_table.py; the expected calls are written out
literally."""
import inspect
import os
import sys
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _slicewise_cases as S  # noqa: E402

REG = dict(regul_param=0.11, iterations=7, time_marching_step=0.22, methodTV=1, PD_LipschitzConstant=9.5, tolerance=0.0)
# name -> (function in regularisersCuPy, driver in slab, positional arguments after the array of the function (with the device
# index 0 and half_precision) and of the driver (after the communicator)); self.nonneg_regul = 1
CALLS = {
    "ROF_TV": ("ROF_TV_cupy", "rof_tv_slab", (0.11, 7, 0.22, 0, False), (0.11, 7, 0.22, False)),
    "PD_TV": ("PD_TV_cupy", "pd_tv_slab", (0.11, 7, 1, 1, 9.5, 0, False), (0.11, 7, 1, 1, 9.5, False)),
}
OTHERS = {"TGV": "TGV_cupy", "NDF": "NDF_cupy", "Diff4th": "Diff4th_cupy", "LLT_ROF": "LLT_ROF_cupy"}
OTHER_SLABS = ("ndf_slab", "diff4th_slab", "llt_rof_slab")


class Untouchable:
    """a communicator that must not be used: every attribute access is an error"""

    def __getattribute__(self, name):
        raise AssertionError(f"the communicator was touched: {name}")


def _self(slab=None):
    return types.SimpleNamespace(nonneg_regul=1, Atools=types.SimpleNamespace(device_index=0), slab=slab)


@pytest.fixture
def calls(monkeypatch):
    from tomobar_amd import regularisersCuPy as R
    from tomobar_amd import slab as Sl
    log = []

    def recorder(name, is_slab):
        def fn(*args, **kwargs):
            log.append((name, args, dict(kwargs)))
            if is_slab:
                kwargs["info"].update(iterations_done=5, rel_change=0.25)
            return name
        return fn

    for name in [c[0] for c in CALLS.values()] + list(OTHERS.values()):
        monkeypatch.setattr(R, name, recorder(name, False))
    for name in [c[1] for c in CALLS.values()] + list(OTHER_SLABS):
        monkeypatch.setattr(Sl, name, recorder(name, True))
    return log


def _same(got, want):
    return tuple(got) == tuple(want) and [type(v) for v in got] == [type(v) for v in want]


# ------------------------------------------------------------------------------------------------ dispatch
@pytest.mark.parametrize("key", [{}, {"slicewise": False}], ids=["absent", "false"])
@pytest.mark.parametrize("name", sorted(CALLS))
def test_without_the_key_every_call_is_todays(calls, name, key):
    from tomobar_amd import regularisersCuPy as R
    fn, driver, whole, slab = CALLS[name]
    X, out, comm = torch.zeros((4, 5, 6)), torch.zeros((4, 5, 6)), object()
    reg = dict(REG, method=name, **key)
    assert R.prox_regul(_self(), X, dict(reg), out=out) == fn
    assert R.prox_regul(_self(comm), X, dict(reg), out=out) == driver
    (n0, a0, k0), (n1, a1, k1) = calls
    assert n0 == fn and a0[0] is X and _same(a0[1:], whole)
    assert set(k0) == {"out", "tolerance"} and k0["out"] is out and k0["tolerance"] == 0.0
    assert n1 == driver and a1[0] is X and a1[1] is comm and _same(a1[2:], slab)
    assert set(k1) == {"out", "tolerance", "info"} and k1["out"] is out and k1["tolerance"] == 0.0


@pytest.mark.parametrize("tolerance", [0.0, 0.001])
@pytest.mark.parametrize("suffix", ["", "_WAVELETS"])
@pytest.mark.parametrize("name", sorted(CALLS))
def test_with_the_key_the_whole_volume_function_runs_slicewise(calls, name, suffix, tolerance, monkeypatch):
    from tomobar_amd import regularisersCuPy as R
    shrunk = []
    monkeypatch.setattr(R, "WAVELETS_cupy", lambda *a, **k: shrunk.append((a, k)))
    fn, _, whole, _ = CALLS[name]
    X, out = torch.zeros((4, 5, 6)), torch.zeros((4, 5, 6))
    reg = dict(REG, method=name + suffix, slicewise=True, tolerance=tolerance)
    assert R.prox_regul(_self(), X, dict(reg), out=out) == fn
    (n, a, k), = calls
    assert n == fn and a[0] is X and _same(a[1:], whole)
    assert set(k) == {"out", "tolerance", "slicewise"} and k["out"] is out and k["tolerance"] == tolerance and k["slicewise"] is True
    assert len(shrunk) == (1 if suffix else 0)   # the shrinkage is per slice anyway: it runs as without the key


@pytest.mark.parametrize("suffix", ["", "_WAVELETS"])
@pytest.mark.parametrize("name", sorted(CALLS))
def test_a_slab_rank_runs_its_own_slices_and_never_touches_the_communicator(calls, name, suffix, monkeypatch):
    from tomobar_amd import regularisersCuPy as R
    monkeypatch.setattr(R, "WAVELETS_cupy", lambda *a, **k: None)
    fn, _, whole, _ = CALLS[name]
    X, out = torch.zeros((4, 5, 6)), torch.zeros((4, 5, 6))
    reg = dict(REG, method=name + suffix, slicewise=True)
    me = _self(Untouchable())
    R.check_prox_available(me, X.shape, reg)
    R.reserve_prox_scratch(me, X.shape, reg)      # slab ranks reserve nothing here, as without the key
    assert R.prox_regul(me, X, dict(reg), out=out) == fn
    (n, a, k), = calls
    assert n == fn and a[0] is X and _same(a[1:], whole)
    assert set(k) == {"out", "tolerance", "slicewise"} and k["slicewise"] is True and k["tolerance"] == 0.0
    # a tolerance would let the ranks stop at different iterations: refused before any work
    for call in (lambda r: R.prox_regul(me, X, r), lambda r: R.check_prox_available(me, X.shape, r)):
        with pytest.raises(ValueError) as e:
            call(dict(reg, tolerance=0.001))
        assert "does not take a tolerance in z-slab mode" in str(e.value) and str(e.value).startswith(name)
    assert len(calls) == 1


@pytest.mark.parametrize("shape", [(1, 5, 6), (4, 1, 6), (5, 6)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("slab", [False, True], ids=["whole_volume", "slab"])
@pytest.mark.parametrize("name", sorted(CALLS))
def test_a_2d_input_or_a_singleton_axis_takes_todays_path(calls, name, slab, shape):
    from tomobar_amd import regularisersCuPy as R
    fn, _, whole, _ = CALLS[name]
    X = torch.zeros(shape)
    me = _self(Untouchable() if slab else None)
    assert R.prox_regul(me, X, dict(REG, method=name, slicewise=True, tolerance=0.001)) == fn
    (n, a, k), = calls
    assert n == fn and a[0] is X and _same(a[1:], whole)
    assert set(k) == {"out", "tolerance"} and k["tolerance"] == 0.001


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("slab", [False, True], ids=["whole_volume", "slab"])
@pytest.mark.parametrize("shape", [(4, 5, 6), (1, 5, 6)], ids=["3d", "singleton"])
def test_the_other_kinds_refuse_the_key_before_any_work(calls, slab, shape):
    from tomobar_amd import regularisersCuPy as R
    X = torch.zeros(shape)
    me = _self(Untouchable() if slab else None)
    for name in OTHERS:
        for method in (name, name + "_WAVELETS") if name != "LLT_ROF" else (name,):
            reg = dict(REG, method=method, slicewise=True)
            for call in (lambda: R.prox_regul(me, X, dict(reg)), lambda: R.check_prox_available(me, X.shape, reg),
                         lambda: R.reserve_prox_scratch(me, X.shape, reg)):
                with pytest.raises(ValueError) as e:
                    call()
                assert str(e.value) == f"{name} does not support slicewise=True", (method, str(e.value))
            # False is today's call
            R.check_prox_available(_self(), X.shape, dict(reg, slicewise=False))
    assert calls == []


@pytest.mark.parametrize("value", [1, 0, "yes", None, 1.0])
def test_a_value_that_is_not_a_bool_is_a_value_error(calls, value, monkeypatch):
    from tomobar_amd import ops
    from tomobar_amd import regularisersCuPy as R
    from tomobar_amd.supp.dicts import dicts_check
    X = torch.zeros((4, 5, 6))
    for name in list(CALLS) + list(OTHERS):
        reg = dict(REG, method=name, slicewise=value)
        for call in (lambda: R.prox_regul(_self(), X, dict(reg)), lambda: R.check_prox_available(_self(), X.shape, reg),
                     lambda: R.reserve_prox_scratch(_self(), X.shape, reg)):
            with pytest.raises(ValueError, match=r"_regularisation_\['slicewise'\] must be True or False"):
                call()
    monkeypatch.setattr(ops, "to_device", lambda x, index: x)
    me = types.SimpleNamespace(Atools=types.SimpleNamespace(device_index=0), OS_number=1)
    with pytest.raises(ValueError, match=r"_regularisation_\['slicewise'\] must be True or False"):
        dicts_check(me, {"projection_data": torch.zeros((2, 3, 4))}, {}, {"method": "PD_TV", "slicewise": value}, method_run="FISTA")
    assert calls == []


# ------------------------------------------------------------------------------------------------ dicts_check, table
def test_dicts_check_adds_no_key_and_keeps_a_given_one(monkeypatch):
    from tomobar_amd import ops
    from tomobar_amd.supp.dicts import dicts_check
    monkeypatch.setattr(ops, "to_device", lambda x, index: x)
    me = types.SimpleNamespace(Atools=types.SimpleNamespace(device_index=0), OS_number=1)

    def run(reg, method_run="FISTA"):
        return dicts_check(me, {"projection_data": torch.zeros((2, 3, 4))}, {}, reg, method_run=method_run)[2]

    for method in ("PD_TV", "ROF_TV", "TGV", "NDF", "PD_TV_WAVELETS", None):
        for driver in ("FISTA", "ADMM", "OSEM"):
            assert "slicewise" not in run({"method": method}, driver)
            assert run({"method": method, "slicewise": True}, driver)["slicewise"] is True
            assert run({"method": method, "slicewise": False}, driver)["slicewise"] is False


def test_the_kinds_with_a_slicewise_form_are_one_constant_beside_the_table():
    from tomobar_amd import _lib
    from tomobar_amd.supp import regularisers as T
    assert T.SLICEWISE_KINDS == ("ROF_TV", "PD_TV") and T.SLICEWISE == "slicewise"
    assert tuple(k.name for k in T.KINDS) == ("ROF_TV", "PD_TV", "TGV", "NDF", "Diff4th", "LLT_ROF")
    assert all(name in T.BY_NAME for name in T.SLICEWISE_KINDS)
    assert T.slicewise_of({}) is False and T.slicewise_of({"slicewise": True}) is True
    for sym, nargs in (("tomo_pdtv_slices", 18), ("tomo_roftv_slices", 14), ("tomo_pdtv_slices_scratch_bytes", 4),
                       ("tomo_roftv_slices_scratch_bytes", 3)):
        assert len(_lib.SIGNATURES[sym][1]) == nargs and hasattr(_lib.lib(), sym), sym
    assert _lib.ABI_VERSION == 10


def test_the_functions_gain_one_trailing_keyword():
    from tomobar_amd import regularisersCuPy as R
    pd = list(inspect.signature(R.PD_TV_cupy).parameters.values())
    rof = list(inspect.signature(R.ROF_TV_cupy).parameters.values())
    assert [p.name for p in pd] == ["data", "regularisation_parameter", "iterations", "methodTV", "nonneg", "lipschitz_const",
                                    "gpu_id", "half_precision", "out", "tolerance", "slicewise"]
    assert [p.default for p in pd[1:]] == [1e-05, 1000, 0, 0, 8.0, 0, False, None, 0.0, False]
    assert [p.name for p in rof] == ["data", "regularisation_parameter", "iterations", "time_marching_parameter", "gpu_id",
                                     "half_precision", "out", "tolerance", "slicewise"]
    assert [p.default for p in rof[1:]] == [1e-05, 3000, 0.001, 0, False, None, 0.0, False]


# ------------------------------------------------------------------------------------------------ scratch
@pytest.fixture
def reserved(monkeypatch):
    from tomobar_amd import regularisersCuPy as R
    log = []
    monkeypatch.setattr(R, "ops", types.SimpleNamespace(
        reserve_tv_scratch=lambda *args: log.append(("tv",) + args),
        reserve_tv_slices_scratch=lambda *args: log.append(("slices",) + args),
        reserve_wavelet_scratch=lambda *args: log.append(("wavelets",) + args)))
    return log


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("name", sorted(CALLS))
def test_reserve_prox_scratch_sizes_the_arena_for_the_slicewise_form(reserved, name, half):
    from tomobar_amd import regularisersCuPy as R
    reg = {"method": name, "slicewise": True, "half_precision": half}
    R.reserve_prox_scratch(_self(), (8, 9, 10), reg)
    assert reserved == [("slices", (8, 9, 10), "cuda:0", name, half)]
    del reserved[:]
    R.reserve_prox_scratch(_self(), (8, 9, 10), dict(reg, method=name + "_WAVELETS"))
    assert reserved == [("slices", (8, 9, 10), "cuda:0", name, half), ("wavelets", (8, 9, 10), "cuda:0")]
    # a singleton axis, a 2D shape and an absent / False key: today's reservation
    for shape, passed in (((1, 9, 10), (9, 10)), ((8, 1, 10), (8, 10)), ((9, 10), (9, 10))):
        del reserved[:]
        R.reserve_prox_scratch(_self(), shape, reg)
        assert reserved == [("tv", passed, "cuda:0", name, half)]
    for key in ({}, {"slicewise": False}):
        del reserved[:]
        R.reserve_prox_scratch(_self(), (8, 9, 10), {"method": name, "half_precision": half, **key})
        assert reserved == [("tv", (8, 9, 10), "cuda:0", name, half)]
    # whole volume only
    del reserved[:]
    R.reserve_prox_scratch(_self(Untouchable()), (8, 9, 10), reg)
    assert reserved == []


def test_scratch_bytes_of_the_slicewise_form():
    """host arithmetic of the library: every work array is rounded up to 256 bytes and followed by the 69888-byte array skew"""
    from tomobar_amd import _lib, ops
    lib = _lib.lib()
    for dx, dy, nz in ((59, 9, 3), (1024, 1024, 256), (2, 2, 2)):
        nvox = dx * dy * nz
        f32 = (nvox * 4 + 255) // 256 * 256 + ops.ARRAY_SKEW
        f16 = (nvox * 2 + 255) // 256 * 256 + ops.ARRAY_SKEW
        assert lib.tomo_roftv_slices_scratch_bytes(dx, dy, nz) == f32
        assert lib.tomo_pdtv_slices_scratch_bytes(dx, dy, nz, 0) == 6 * f32
        assert lib.tomo_pdtv_slices_scratch_bytes(dx, dy, nz, 1) == 2 * f32 + 4 * f16
    with pytest.raises(ValueError, match="TGV does not support slicewise=True"):
        ops.reserve_tv_slices_scratch((8, 9, 10), "cpu", "TGV")


# ------------------------------------------------------------------------------------------------ what the GPU file relies on
def test_the_input_tells_slicewise_from_3d_on_the_oracle():
    """per-slice noise of amplitude 0.1 on a z-ramp: after 7 iterations the 3D result lies 0.13-0.16 (PD_TV) and 3-6e-3
    (ROF_TV) from the slice-wise one, so a comparison that ignores the key fails"""
    for shape in S.DISTINCT_SHAPES:
        vol = S.volume(shape)
        for method, kw, lo, hi in (("PD_TV", S.pd_kwargs(7), 0.12, 0.17), ("ROF_TV", S.rof_kwargs(7), 3e-3, 7e-3)):
            gap = float(np.abs(S.oracle_3d(method, vol, **kw) - S.oracle_slices(method, vol, **kw)).max())
            assert lo < gap < hi, (shape, method, gap)
    # the noise is seeded per slice: a sub-stack carries the noise of its own slices, `changed` touches one slice only
    a, b = S.volume((5, 7, 9)), S.volume((5, 7, 9), changed=2)
    assert np.array_equal(a[[0, 1, 3, 4]], b[[0, 1, 3, 4]]) and not np.array_equal(a[2], b[2])
    assert np.array_equal(a - np.linspace(0, 1, 5, dtype=np.float32)[:, None, None],
                          S.volume((5, 7, 9)) - np.linspace(0, 1, 5, dtype=np.float32)[:, None, None])


@pytest.mark.parametrize("name", sorted(S.TOL_CASES))
def test_the_tolerance_thresholds_have_their_margins(name):
    tol, stop, d_stop, never = S.tol_plan(name)
    assert 18 <= stop <= 60 and d_stop < tol and 0.0 < never < min(S.tol_sequence(name))


def test_the_shape_lists_cover_the_tile_edges():
    for cases, tiles in ((S.PD_CASES, (58, 60, 62)), (S.ROF_CASES, (60,))):
        widths = {shape[2] for shape, _ in cases}
        heights = {shape[1] for shape, _ in cases}
        assert any(w in widths for t in tiles for w in (t - 1,)) and any(t + 1 in widths for t in tiles) and 2 in widths
        assert {2, 7, 8, 9, 17} <= heights
        assert {shape[0] for shape, _ in cases} == {2, 3, 5}
        assert {1, 2, 3, 4, 7} <= {iters for _, iters in cases}
        assert len(cases) <= 12
