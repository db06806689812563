"""NLTV without a GPU: the numpy restatement tests/_nltv_oracle.py against what docs/kernels/nltv.md states (the
exponential, PatchSelect on images whose answer is known, the iteration on a noisy phantom, float32 beside float64), and the
host side of the method: how prox_regul / check_prox_available / reserve_prox_scratch / dicts_check treat "NLTV" (recorders in
the style of tests/test_regulariser_table.py), and the three C entry points."""
import functools
import types

import numpy as np
import pytest
import torch

import _nltv_oracle as N
import test_regulariser_table as TT

f32 = np.float32
PHANTOM_SHAPE, S, P, K, H = (70, 131), 7, 2, 15, 0.3


@functools.lru_cache(maxsize=None)
def phantom_tables():
    """the tables of the noisy 70 x 131 phantom, computed once (read-only)"""
    noisy = N.noisy_phantom(PHANTOM_SHAPE)
    tables = N.patch_select(noisy, S, P, K, H)
    for t in (noisy,) + tables:
        t.setflags(write=False)
    return noisy, tables


# ------------------------------------------------------------------------------------------------ wexp
def test_wexp_against_float64_exp():
    """relative error <= 5e-6 on [0, 87]: the bound is the rounding of the argument y = x log2(e) <= 126, 126 * 2^-24 * ln 2 =
    5.2e-6 (measured: docs/kernels/nltv.md)"""
    x = np.linspace(0.0, 87.0, 2_000_001).astype(f32)
    got = N.wexp(x).astype(np.float64)
    want = np.exp(-x.astype(np.float64))
    rel = np.abs(got - want) / want
    print(f"wexp: max relative error {rel.max():.3e} at x = {x[rel.argmax()]:.4f}")
    assert rel.max() <= 5e-6
    assert N.wexp(f32(0.0)) == f32(1.0) and N.wexp(f32(0.0)).dtype == f32
    # beyond the clamp y = 126 the value stays 2^-126 p: small, finite, not negative
    assert 0.0 <= float(N.wexp(f32(1e6))) < 1e-37


def test_wexp_constants_are_the_taylor_coefficients():
    import math
    for k, c in enumerate(N.WEXP_C):
        assert c == (-math.log(2.0)) ** k / math.factorial(k) or abs(c - (-math.log(2.0)) ** k / math.factorial(k)) <= 2e-16 * abs(c)
    assert N.LOG2E == 1.0 / math.log(2.0) or abs(N.LOG2E - 1.0 / math.log(2.0)) < 3e-16


# ------------------------------------------------------------------------------------------------ PatchSelect
def _first_candidates(shape, S_, K_):
    """the first K in-slice candidates of every pixel in candidate order, padded with the pixel itself"""
    ny, nx = shape
    hi = np.empty((K_, ny, nx), np.uint16)
    hj = np.empty((K_, ny, nx), np.uint16)
    n = np.zeros((ny, nx), int)
    for j in range(ny):
        for i in range(nx):
            inside = [(j + jm, i + im) for jm, im in N.candidates(S_) if 0 <= j + jm < ny and 0 <= i + im < nx][:K_]
            n[j, i] = len(inside)
            inside += [(j, i)] * (K_ - len(inside))
            hj[:, j, i], hi[:, j, i] = zip(*inside)
    return hi, hj, n


@pytest.mark.parametrize("shape, S_, P_, K_", [((9, 11), 2, 1, 8), ((6, 7), 3, 2, 15), ((1, 1), 3, 1, 8), ((2, 3), 3, 1, 8)],
                         ids=["9x11", "6x7", "1x1", "2x3"])
def test_patch_select_on_a_constant_image(shape, S_, P_, K_):
    """every distance is 0: the weights are exactly 1, the selection is the first K in-slice candidates in candidate order; a
    pixel with fewer than K candidates (1 x 1: none; 2 x 3: five) is padded with itself and the weight 0"""
    hi, hj, w = N.patch_select(np.full(shape, 0.37, f32), S_, P_, K_, 0.5)
    want_i, want_j, n = _first_candidates(shape, S_, K_)
    assert hi.dtype == hj.dtype == np.uint16 and w.dtype == f32 and hi.shape == hj.shape == w.shape == (K_,) + shape
    assert np.array_equal(hi, want_i) and np.array_equal(hj, want_j)
    assert np.array_equal(w, (np.arange(K_)[:, None, None] < n).astype(f32))
    if shape == (1, 1):
        assert n[0, 0] == 0
    if shape == (2, 3):
        assert np.all(n == 5)


def test_patch_select_orders_by_distance_and_breaks_ties_by_candidate_order():
    noisy, (hi, hj, w) = phantom_tables()
    d, valid = N.distances(noisy, S, P)
    cand = np.array(N.candidates(S))
    rng = np.random.default_rng(3)
    for j, i in zip(rng.integers(0, PHANTOM_SHAPE[0], 40), rng.integers(0, PHANTOM_SHAPE[1], 40)):
        ms = [m for m in range(len(cand)) if valid[m, j, i]]
        ms.sort(key=lambda m: (d[m, j, i], m))
        want = [(j + cand[m, 0], i + cand[m, 1]) for m in ms[:K]]
        assert list(zip(hj[:, j, i].tolist(), hi[:, j, i].tolist())) == want, (j, i)
    assert np.all(np.diff(w, axis=0) <= 0), "the weights fall with the rank"
    # the tie-break decides on the piecewise-constant image
    t = N.terraces((13, 37))
    thi, thj, tw = N.patch_select(t, 3, 1, 8, 0.3)
    ties = np.mean(tw[1:] == tw[:-1])
    print(f"terraces: {100 * ties:.0f} % of adjacent selected pairs tie")
    assert ties > 0.5


def test_patch_select_3d_is_the_stack_of_2d_calls():
    vol = N.noisy_phantom((3, 13, 37))
    got = N.patch_select(vol, 3, 1, 8, 0.3)
    for z in range(3):
        for a, b in zip(got, N.patch_select(vol[z], 3, 1, 8, 0.3)):
            assert a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a[:, z]).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ------------------------------------------------------------------------------------------------ NLTV
def _rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - b) ** 2)))


@pytest.mark.parametrize("lam", [0.02, 0.1, 0.5])
def test_nltv_denoises_the_phantom_and_float32_follows_float64(lam):
    """5 iterations on the noisy phantom (sigma = 0.1): the RMSE against the clean image falls, and float32 stays within 5e-6
    of float64 on the same tables (measured: docs/kernels/nltv.md)"""
    noisy, (hi, hj, w) = phantom_tables()
    clean = N.clean_phantom(PHANTOM_SHAPE)
    u32 = N.nltv(noisy, hi, hj, w, lam, 5)
    u64 = N.nltv(noisy, hi, hj, w, lam, 5, np.float64)
    before, after = _rmse(noisy, clean), _rmse(u32, clean)
    dev = float(np.abs(u32.astype(np.float64) - u64).max())
    print(f"lambda {lam}: RMSE {before:.4f} -> {after:.4f}; float32 - float64: {dev:.2e}")
    assert u32.dtype == f32 and u64.dtype == np.float64 and np.all(np.isfinite(u32))
    assert after < before
    assert dev <= 5e-6
    assert np.array_equal(N.nltv(noisy, hi, hj, w, lam, 0), noisy)


@pytest.mark.parametrize("shape", [(1, 1), (2, 3), (1, 37), (37, 1)], ids=lambda s: "x".join(map(str, s)))
def test_nltv_stays_finite_on_tiny_shapes(shape):
    f = N.noisy_phantom(shape)
    for S_, P_, K_ in ((1, 1, 8), (1, 1, 10), (3, 1, 8)):
        hi, hj, w = N.patch_select(f, S_, P_, K_, 0.3)
        assert np.all(hi < shape[1]) and np.all(hj < shape[0])
        assert np.all(np.isfinite(N.nltv(f, hi, hj, w, 0.1, 5)))


# ------------------------------------------------------------------------------------------------ the method string
def test_is_nltv_and_the_table_is_unchanged():
    from tomobar_amd.supp import regularisers as T
    assert tuple(k.name for k in T.KINDS) == TT.ORDER and "NLTV" not in T.BY_NAME
    for method in ("NLTV", "NLTV_2D", "my_NLTV"):
        assert T.is_nltv(method) and T.kind_of(method) is None
    for method in TT.METHODS + list(TT.NEITHER) + ["NLTV_PD_TV", "ROF_TV_NLTV", "NLT", "nltv"]:
        assert not T.is_nltv(method), method


def _tables(shape=(4, 5, 6), k=3):
    return {"NLTV_H_i": np.zeros((k,) + shape, np.uint16), "NLTV_H_j": np.zeros((k,) + shape, np.uint16),
            "NLTV_Weights": np.zeros((k,) + shape, f32)}


@pytest.fixture
def calls(monkeypatch):
    from tomobar_amd import regularisersCuPy as R
    log = []
    for name in [v[0] for v in TT.WHOLE.values()] + ["NLTV_cupy", "WAVELETS_cupy"]:
        monkeypatch.setattr(R, name, lambda *a, _n=name, **kw: log.append((_n, a, dict(kw))) or _n)
    return log


@pytest.mark.parametrize("shape, slab", [((4, 5, 6), False), ((4, 5, 6), True), ((1, 5, 6), True)],
                         ids=["whole_volume", "slab", "singleton_axis_with_slab"])
def test_prox_regul_calls_nltv_cupy(calls, shape, slab):
    """the whole-volume function with the three tables, regul_param and the iteration count -- on a slab rank too"""
    from tomobar_amd import regularisersCuPy as R
    X, out = torch.zeros(shape), torch.zeros(shape)
    tables = _tables(shape)
    for extra, iters in (({}, 7), ({"IterNumb": 7}, 7), ({"NumNeighb": 3, "slicewise": True}, 7)):
        del calls[:]
        reg = dict(TT.REG, method="NLTV", tolerance=0.0, **tables, **extra)
        assert R.prox_regul(TT._self(object() if slab else None), X, reg, out=out) == "NLTV_cupy"
        (name, args, kwargs), = calls
        assert name == "NLTV_cupy" and args[0] is X and all(a is tables[k] for a, k in zip(args[1:4], tables))
        assert TT._same(args[4:], (0.11, iters, 0)), args[4:]
        assert set(kwargs) == {"out", "tolerance"} and kwargs["out"] is out and kwargs["tolerance"] == 0.0
    # the demo's key alone
    del calls[:]
    reg = dict(method="NLTV", regul_param=0.2, IterNumb=4, **tables)
    R.prox_regul(TT._self(), X, reg)
    assert TT._same(calls[0][1][4:], (0.2, 4, 0))


def test_prox_regul_nltv_refusals(calls):
    from tomobar_amd import regularisersCuPy as R
    X, tables = torch.zeros((4, 5, 6)), _tables()
    for comm in (None, object()):
        me = TT._self(comm)
        for method in ("NLTV_PD_TV", "ROF_TV_NLTV", "NLTV_NDF"):
            with pytest.raises(ValueError, match="names both .* and NLTV"):
                R.prox_regul(me, X, dict(TT.REG, method=method, **tables))
        with pytest.raises(ValueError, match="NLTV does not combine with WAVELETS"):
            R.prox_regul(me, X, dict(TT.REG, method="NLTV_WAVELETS", **tables))
        with pytest.raises(ValueError, match="NLTV does not support half_precision=True"):
            R.prox_regul(me, X, dict(TT.REG, method="NLTV", half_precision=True, **tables))
        with pytest.raises(ValueError, match="NLTV does not support half_precision=True"):
            R.check_prox_available(me, X.shape, dict(TT.REG, method="NLTV", half_precision=True, **tables))
        for key in tables:
            with pytest.raises(ValueError, match=f"'{key}'"):
                R.prox_regul(me, X, {k: v for k, v in dict(TT.REG, method="NLTV", tolerance=0.0, **tables).items() if k != key})
        with pytest.raises(ValueError, match="IterNumb.*differ"):
            R.prox_regul(me, X, dict(TT.REG, method="NLTV", tolerance=0.0, IterNumb=8, **tables))
        with pytest.raises(ValueError) as e:
            R.prox_regul(me, X, dict(TT.REG, method="FGP_TV"))
        assert str(e.value) == TT.UNKNOWN
    # a tolerance on a slab rank with a real 3D volume, exactly as slicewise refuses it (TT.REG carries tolerance = 0.001)
    with pytest.raises(ValueError, match="NLTV does not take a tolerance in z-slab mode"):
        R.prox_regul(TT._self(object()), X, dict(TT.REG, method="NLTV", **tables))
    assert calls == []
    R.prox_regul(TT._self(), X, dict(TT.REG, method="NLTV", **tables))
    R.prox_regul(TT._self(object()), torch.zeros((1, 5, 6)), dict(TT.REG, method="NLTV", **_tables((1, 5, 6))))
    assert [c[2]["tolerance"] for c in calls] == [0.001, 0.001]


def test_reserve_prox_scratch_reserves_the_one_work_array(monkeypatch):
    from tomobar_amd import regularisersCuPy as R
    log = []
    monkeypatch.setattr(R, "ops", types.SimpleNamespace(reserve_nltv_scratch=lambda *a: log.append(a)))
    for comm in (None, object()):
        for shape in ((8, 9, 10), (1, 9, 10), (9, 10)):
            del log[:]
            R.reserve_prox_scratch(TT._self(comm), shape, {"method": "NLTV", "slicewise": True})
            assert log == [(shape, "cuda:0")]


# ------------------------------------------------------------------------------------------------ dicts_check
@pytest.fixture
def run(monkeypatch):
    from tomobar_amd import ops
    from tomobar_amd.supp.dicts import dicts_check
    monkeypatch.setattr(ops, "to_device", lambda x, index: x)
    me = types.SimpleNamespace(Atools=types.SimpleNamespace(device_index=0, vol_shape=lambda: (4, 5, 6)), OS_number=1)
    return lambda reg, method_run="FISTA": dicts_check(me, {"projection_data": torch.zeros((2, 3, 4))}, {}, reg, method_run=method_run)[2]


def test_dicts_check_requires_and_checks_the_tables(run):
    good = dict(method="NLTV", **_tables())
    got = run(dict(good))
    assert got["NumNeighb"] == 3 and got["iterations"] == 150 and got["regul_param"] == 0.001 and "IterNumb" not in got
    assert set(got) - set(run({"method": "ROF_TV"})) == set(_tables()) | {"NumNeighb"}
    for key in _tables():
        with pytest.raises(ValueError, match=f"_regularisation_\\['{key}'\\] is required by the NLTV method"):
            run({k: v for k, v in good.items() if k != key})
        with pytest.raises(ValueError, match=f"_regularisation_\\['{key}'\\] must be a (uint16|float32) array, got"):
            run(dict(good, **{key: good[key].astype(np.int32)}))
        with pytest.raises(ValueError, match="share one shape"):
            run(dict(good, **{key: good[key][:2]}))
    with pytest.raises(ValueError, match=r"\(neighbours, \*volume\) with the volume \(4, 5, 6\)"):
        run(dict(method="NLTV", **_tables((4, 5, 7))))
    # device tensors as PatchSelect_cupy returns them; the squeezed shape of a singleton volume
    run(dict(method="NLTV", **{k: torch.from_numpy(v) for k, v in _tables().items()}))
    run(dict(method="NLTV", **_tables((20, 6))))


def test_dicts_check_numneighb_and_iternumb(run):
    good = dict(method="NLTV", **_tables())
    assert run(dict(good, NumNeighb=3))["NumNeighb"] == 3
    with pytest.raises(ValueError, match=r"_regularisation_\['NumNeighb'\] = 15, the tables hold 3 neighbours"):
        run(dict(good, NumNeighb=15))
    assert run(dict(good, IterNumb=5))["iterations"] == 5
    assert run(dict(good, iterations=6))["iterations"] == 6
    assert run(dict(good, IterNumb=5, iterations=5))["iterations"] == 5
    with pytest.raises(ValueError, match="IterNumb.*differ"):
        run(dict(good, IterNumb=5, iterations=6))
    for method in ("NLTV_PD_TV", "NLTV_WAVELETS"):
        with pytest.raises(ValueError, match="NLTV"):
            run(dict(good, method=method))
    with pytest.raises(ValueError, match="half_precision"):
        run(dict(good, half_precision=True))
    # the reference demo's dictionary
    demo = {"method": "NLTV", "regul_param": 0.0005, "iterations": 5, "NLTV_H_i": good["NLTV_H_i"], "NLTV_H_j": good["NLTV_H_j"],
            "NLTV_Weights": good["NLTV_Weights"], "NumNeighb": 3, "IterNumb": 5, "device_regulariser": "gpu"}
    assert run(dict(demo))["iterations"] == 5


# ------------------------------------------------------------------------------------------------ ABI
def test_the_three_entry_points_are_bound_and_exported():
    from tomobar_amd import _lib
    assert _lib.ABI_VERSION == 10
    for flavour in ("shipped", "dev"):
        with _lib.use_flavour(flavour) as handle:
            assert handle.tomo_abi_version() == 10
            for name in ("tomo_nltv_scratch_bytes", "tomo_patch_select", "tomo_nltv"):
                assert name in _lib.SIGNATURES and hasattr(handle, name), (flavour, name)
            # one work array, like the other marched operators; invalid arguments are refused before any device is touched
            assert handle.tomo_nltv_scratch_bytes(37, 13, 7, 3) == handle.tomo_ndf_scratch_bytes(37, 13, 7, 3)
            bad = [dict(search=0), dict(search=16), dict(patch=0), dict(patch=5), dict(k=0), dict(k=33), dict(h=0.0), dict(dx=65536),
                   dict(dy=65536), dict(nd=4), dict(ptr=None)]
            for change in bad:
                a = dict(dict(dx=8, dy=8, nd=2, search=3, patch=1, k=8, h=0.5, ptr=64), **change)
                p = a["ptr"]
                assert handle.tomo_patch_select(0, p, p, p, p, a["dx"], a["dy"], 1, a["nd"], a["search"], a["patch"], a["k"], a["h"],
                                                None) == _lib.E_INVALID, change
            for change in (dict(k=0), dict(k=33), dict(lam=0.0), dict(dx=65536), dict(nd=1), dict(ptr=None)):
                a = dict(dict(dx=8, dy=8, nd=2, k=8, lam=0.1, ptr=64), **change)
                p = a["ptr"]
                assert handle.tomo_nltv(0, 64, 128, p, p, p, a["dx"], a["dy"], 1, a["nd"], a["k"], a["lam"], 1, 0.0, None, None,
                                        None) == _lib.E_INVALID, change


def test_package_names():
    import tomobar_amd
    from tomobar_amd import regularisersCuPy as R
    assert tomobar_amd.NLTV_cupy is R.NLTV_cupy and tomobar_amd.PatchSelect_cupy is R.PatchSelect_cupy
    from tomobar_amd import ops
    assert callable(ops.patch_select) and callable(ops.nltv) and callable(ops.reserve_nltv_scratch)
