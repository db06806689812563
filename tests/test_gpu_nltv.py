"""MI355X tests of non-local TV: the shipped patch_select and nltv_iter kernels against the float32 numpy restatement
tests/_nltv_oracle.py, bit for bit -- the index tables included (there is no reference implementation: formula-level parity,
unpinned; docs/kernels/nltv.md) --, through the ops functions, PatchSelect_cupy / NLTV_cupy, the tolerance rule, a slab rank
and the three drivers that reach NLTV through prox_regul."""
import functools
import inspect
import math
import os
import sys
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _march_gpu as G  # noqa: E402
import _nltv_oracle as N  # noqa: E402
from _march_gpu import host, same_bits  # noqa: E402
from _tolerance_cases import rel_d  # noqa: E402

f32 = np.float32
# a workgroup owns 32 x 16 pixels: one row and one column below, at and above the tile's extents
SHAPES_2D = [(1, 1), (2, 3), (1, 37), (37, 1), (13, 37), (15, 31), (16, 32), (17, 33)]
SHAPES_3D = [(7, 13, 37), (3, 70, 131)]
# (S, P, K): exactly all candidates; padding; a small window; the demo's; the largest patch and list
PARAMS = [(1, 1, 8), (1, 1, 10), (3, 1, 8), (7, 2, 15), (5, 4, 32)]
# name -> (image, h): the noisy phantom; the piecewise-constant image, where the tie-break decides; the phantom x 1000 with an
# h that puts x log2(e) on both sides of the clamp at 126
INPUTS = {"noisy": (lambda shape: N.noisy_phantom(shape), 0.3),
          "terraces": (lambda shape: N.terraces(shape), 0.3),
          "large": (lambda shape: N.noisy_phantom(shape) * f32(1000.0), 60.0)}


def _id(v):
    return "x".join(map(str, v))


@functools.lru_cache(maxsize=None)
def oracle_tables(name, shape, params):
    """(image, (H_i, H_j, W)) of the oracle, computed once per case and left unchanged"""
    make, h = INPUTS[name]
    img = make(shape)
    tables = N.patch_select(img, *params, h)
    for t in (img,) + tables:
        t.setflags(write=False)
    return img, tables


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()   # (a copy: the oracle's arrays are read-only)


def check_tables(got, want, what):
    for name, g, w in zip(("H_i", "H_j"), got[:2], want[:2]):
        g = host(g)
        assert g.dtype == np.uint16 and g.shape == w.shape, (what, name)
        assert np.array_equal(g, w), (what, name, f"{int((g != w).sum())} of {g.size} indices differ")
    same_bits(host(got[2]), want[2], (what, "Weights"))


# ------------------------------------------------------------------------------------------------ patch_select
@pytest.mark.parametrize("params", PARAMS, ids=_id)
@pytest.mark.parametrize("shape", SHAPES_2D + SHAPES_3D, ids=_id)
def test_ops_patch_select_equals_the_oracle(shape, params):
    from tomobar_amd import ops
    for name, (_, h) in INPUTS.items():
        img, want = oracle_tables(name, shape, params)
        x = dev(img)
        got = ops.patch_select(x, *params, f32(h))
        check_tables(got, want, (name, shape, params))
        assert np.array_equal(host(x).view(np.uint32), img.view(np.uint32)), "the input was written"


def test_the_inputs_exercise_ties_and_the_clamp():
    """what the three inputs are there for, stated on the oracle's tables"""
    _, (_, _, w) = oracle_tables("terraces", (13, 37), (3, 1, 8))
    assert np.mean(w[1:] == w[:-1]) > 0.5
    img, (hi, hj, w) = oracle_tables("large", (70, 131), (7, 2, 15))
    d, valid = N.distances(img, 7, 2)
    y = d[valid] * (f32(1.0) / (f32(60.0) * f32(60.0))) * f32(N.LOG2E)
    assert (y > 126).any() and (y < 126).any()
    assert (w[w > 0] < 2.0 ** -125).any() and (w > 2.0 ** -100).any()


# ------------------------------------------------------------------------------------------------ nltv
COUNTS = (1, 2, 5)
NLTV_CASES = [((1, 1), (1, 1, 10)), ((2, 3), (1, 1, 10)), ((1, 37), (3, 1, 8)), ((37, 1), (3, 1, 8)), ((13, 37), (7, 2, 15)),
              ((17, 33), (5, 4, 32)), ((7, 13, 37), (3, 1, 8)), ((3, 70, 131), (7, 2, 15))]


@functools.lru_cache(maxsize=None)
def oracle_iterates(shape, params, lam, counts):
    img, (hi, hj, w) = oracle_tables("noisy", shape, params)
    return {n: N.nltv(img, hi, hj, w, lam, n) for n in counts}


def run_nltv(img, tables, lam, n, tolerance=0.0):
    from tomobar_amd import ops
    t = [dev(a) for a in tables]
    got, (_, done, d) = G.run_op(lambda x, out: ops.nltv(x, out, *t, f32(lam), n, tolerance), img)
    for a, b in zip(t, tables):
        assert np.array_equal(host(a), b), "a table was written"
    return got, done, d


@pytest.mark.parametrize("lam", [0.02, 0.5])
@pytest.mark.parametrize("shape, params", NLTV_CASES, ids=lambda v: _id(v))
def test_ops_nltv_equals_the_oracle(shape, params, lam):
    """the kernel on the oracle's tables: 0, 1, 2 and 5 iterations into a NaN-filled output, the input checked afterwards"""
    img, tables = oracle_tables("noisy", shape, params)
    want = oracle_iterates(shape, params, lam, COUNTS)
    for n in COUNTS:
        got, done, d = run_nltv(img, tables, lam, n)
        assert done == n and math.isnan(d)
        same_bits(got, want[n], (shape, params, lam, n))
    same_bits(run_nltv(img, tables, lam, 0)[0], img, "iters = 0 copies the input")


def test_nltv_refuses_what_the_header_says():
    from tomobar_amd import ops
    img, tables = oracle_tables("noisy", (13, 37), (3, 1, 8))
    x, t = dev(img), [dev(a) for a in tables]
    with pytest.raises(ValueError, match="alias"):
        ops.nltv(x, x, *t, f32(0.1), 3)
    with pytest.raises(ValueError, match="positive"):
        ops.nltv(x, torch.empty_like(x), *t, f32(0.0), 3)
    with pytest.raises(ValueError, match="iterations"):
        ops.nltv(x, torch.empty_like(x), *t, f32(0.1), -1)
    with pytest.raises(ValueError, match="uint16"):
        ops.nltv(x, torch.empty_like(x), t[0].to(torch.int32), t[1], t[2], f32(0.1), 3)
    with pytest.raises(ValueError, match="shape"):
        ops.nltv(x, torch.empty_like(x), dev(tables[0][:, :5]), t[1], t[2], f32(0.1), 3)
    for bad in ((0, 1, 8), (16, 1, 8), (3, 0, 8), (3, 5, 8), (3, 1, 0), (3, 1, 33)):
        with pytest.raises(ValueError, match="must lie in"):
            ops.patch_select(x, *bad, f32(0.3))
    with pytest.raises(ValueError, match="positive"):
        ops.patch_select(x, 3, 1, 8, f32(0.0))


def test_a_table_with_indices_beyond_the_slice_is_clamped():
    """indices >= nx / ny: the result is what the clamped table gives -- finite, and no access outside the array"""
    shape, params, lam = (7, 13, 37), (3, 1, 8), 0.1
    img, (hi, hj, w) = oracle_tables("noisy", shape, params)
    rng = np.random.default_rng(5)
    bad_i = np.where(rng.random(hi.shape) < 0.3, rng.integers(37, 65536, hi.shape), hi).astype(np.uint16)
    bad_j = np.where(rng.random(hj.shape) < 0.3, rng.integers(13, 65536, hj.shape), hj).astype(np.uint16)
    assert (bad_i >= 37).any() and (bad_j >= 13).any() and bad_i.max() > 60000
    got, _, _ = run_nltv(img, (bad_i, bad_j, w), lam, 3)
    assert np.all(np.isfinite(got))
    same_bits(got, N.nltv(img, np.minimum(bad_i, 36), np.minimum(bad_j, 12), w, lam, 3), "clamped table")


# ------------------------------------------------------------------------------------------------ the *_cupy functions
def test_patch_select_cupy_then_nltv_cupy_equals_the_oracle_chain():
    from tomobar_amd.regularisersCuPy import NLTV_cupy, PatchSelect_cupy, last_prox
    for shape, params in (((13, 37), (7, 2, 15)), ((7, 13, 37), (3, 1, 8))):
        img, want_t = oracle_tables("noisy", shape, params)
        want = oracle_iterates(shape, params, 0.5, COUNTS)[5]
        x = dev(img)
        tables = PatchSelect_cupy(x, *params, 0.3)
        check_tables(tables, want_t, ("PatchSelect_cupy", shape))
        got = NLTV_cupy(x, *tables, 0.5, 5)
        # (a 2D array comes back with a leading singleton axis, as from every *_cupy function and from the reference's)
        assert tuple(got.shape) == ((1,) + shape if len(shape) == 2 else shape)
        same_bits(host(got).reshape(shape), want, ("NLTV_cupy", shape))
        assert last_prox()[0] == 5 and math.isnan(last_prox()[1])
        assert np.array_equal(host(x), img), "the input array was written"
        # out=, a numpy input and numpy tables
        out = torch.full_like(x, float("nan"))
        assert NLTV_cupy(x, *tables, 0.5, 5, out=out).data_ptr() == out.data_ptr()
        same_bits(host(out), want, "out=")
        same_bits(host(NLTV_cupy(img, *want_t, 0.5, 5)).reshape(shape), want, "host arrays")
        with pytest.raises(ValueError, match="alias"):
            NLTV_cupy(x, *tables, 0.5, 5, out=x)
    # the defaults are the demo's: searchwindow 7, patchwindow 2, 15 neighbours, h = 0.9
    img, _ = oracle_tables("noisy", (13, 37), (7, 2, 15))
    check_tables(PatchSelect_cupy(dev(img)), N.patch_select(img, 7, 2, 15, 0.9), "defaults")


def test_cupy_functions_with_a_singleton_axis():
    """a 3D array is a stack of slices along axis 0, singleton axes included; tables of the squeezed shape are accepted"""
    from tomobar_amd.regularisersCuPy import NLTV_cupy, PatchSelect_cupy
    plane, params = N.noisy_phantom((13, 37)), (3, 1, 8)
    for axis in range(3):
        vol = np.expand_dims(plane, axis)
        want_t = N.patch_select(vol, *params, 0.3)
        want = N.nltv(vol, *want_t, 0.1, 3)
        x = dev(vol)
        tables = PatchSelect_cupy(x, *params, 0.3)
        assert all(tuple(t.shape) == (8,) + vol.shape for t in tables)
        check_tables(tables, want_t, ("singleton axis", axis))
        got = NLTV_cupy(x, *tables, 0.1, 3)
        assert tuple(got.shape) == vol.shape
        same_bits(host(got), want, ("singleton axis", axis))
        squeezed = [t.squeeze(axis + 1) for t in tables]
        same_bits(host(NLTV_cupy(x, *squeezed, 0.1, 3)), want, ("squeezed tables", axis))
    with pytest.raises(ValueError, match="expected"):
        NLTV_cupy(dev(plane), *[dev(t[:, :, :5]) for t in N.patch_select(plane, *params, 0.3)], 0.1, 3)
    with pytest.raises(ValueError, match="float32"):
        PatchSelect_cupy(dev(plane).double())
    with pytest.raises(ValueError, match="gpu_device"):
        PatchSelect_cupy(dev(plane), gpu_id=-1)


def test_reserve_nltv_scratch():
    from tomobar_amd import ops
    ops.reserve_nltv_scratch((7, 13, 37), "cuda:0")
    ops.reserve_nltv_scratch((13, 37), "cuda:0")
    shape, params = (7, 13, 37), (3, 1, 8)
    img, tables = oracle_tables("noisy", shape, params)
    same_bits(run_nltv(img, tables, 0.5, 5)[0], oracle_iterates(shape, params, 0.5, COUNTS)[5], "after reserve")


# ------------------------------------------------------------------------------------------------ tolerance
TOL_SHAPE, TOL_PARAMS, TOL_LAM, TOL_ITERS, TOL_J = (13, 37), (7, 2, 15), 0.1, 40, 3


def tolerance_plan():
    """(tol, n the oracle's sequence stops after, the d it stops on, the whole sequence): d_n compares iterate n with iterate
    n - 6 (iterate 0 = the input) after every 6th iteration that leaves at least 3; tol is the geometric mean of the (j-1)-th
    and the j-th value, as tests/_march_oracle.py chooses its threshold"""
    points = tuple(n for n in range(6, TOL_ITERS + 1, 6) if TOL_ITERS - n >= 3)
    its = oracle_iterates(TOL_SHAPE, TOL_PARAMS, TOL_LAM, points)
    prev, seq = oracle_tables("noisy", TOL_SHAPE, TOL_PARAMS)[0], []
    for n in points:
        seq.append(rel_d(its[n], prev))
        prev = its[n]
    tol = float(np.sqrt(seq[TOL_J - 2] * seq[TOL_J - 1]))
    assert all(abs(v - tol) >= 0.01 * tol for v in seq), ("a value of the sequence is too close to the threshold", tol, seq)
    assert next(i for i, v in enumerate(seq, 1) if v < tol) == TOL_J, ("the target is not the first value below the threshold", seq)
    return tol, points[TOL_J - 1], seq[TOL_J - 1], tuple(seq), its


def test_tolerance_stops_where_the_oracle_sequence_stops():
    from tomobar_amd.regularisersCuPy import NLTV_cupy, last_prox
    tol, stop, d_stop, seq, its = tolerance_plan()
    img, tables = oracle_tables("noisy", TOL_SHAPE, TOL_PARAMS)
    x, t = dev(img), [dev(a) for a in tables]
    def run(iterations, **kw):
        return host(NLTV_cupy(x, *t, TOL_LAM, iterations, **kw)).reshape(TOL_SHAPE)

    got = run(TOL_ITERS, tolerance=tol)
    done, d = last_prox()
    print(f"NLTV tolerance {tol:.6e}: stopped after {done} (oracle {stop}), d {d:.6e} (oracle {d_stop:.6e})")
    assert done == stop
    assert abs(d - d_stop) <= got.size * 2.0 ** -53 * d_stop
    plain = run(stop)
    assert last_prox()[0] == stop and math.isnan(last_prox()[1])
    same_bits(got, plain, "a stopped run returns what iterations = n returns")
    same_bits(got, its[stop], "stopped run against the oracle")
    # an odd request: the iterate it stops on then lives in the work array and is copied to the output
    got_odd = run(TOL_ITERS - 1, tolerance=tol)
    assert last_prox()[0] == stop
    same_bits(got_odd, plain, "a stopped run of an odd request")
    # a threshold below the whole sequence: every iteration runs
    never = 0.5 * min(seq)
    full = run(TOL_ITERS, tolerance=never)
    done, d = last_prox()
    assert done == TOL_ITERS and d > never
    same_bits(full, run(TOL_ITERS), "tolerance never met")


# ------------------------------------------------------------------------------------------------ a slab rank
def test_a_slab_rank_equals_the_same_slices_of_the_whole_volume():
    from tomobar_amd import regularisersCuPy as R
    shape, params = (7, 13, 37), (3, 1, 8)
    img, tables = oracle_tables("noisy", shape, params)
    want = oracle_iterates(shape, params, 0.5, COUNTS)[5]
    keys = ("NLTV_H_i", "NLTV_H_j", "NLTV_Weights")
    for z0, z1 in ((0, 3), (3, 5), (5, 7)):
        me = types.SimpleNamespace(nonneg_regul=0, Atools=types.SimpleNamespace(device_index=0), slab=object())
        reg = dict(method="NLTV", regul_param=0.5, iterations=5, **{k: dev(t[:, z0:z1]) for k, t in zip(keys, tables)})
        got = R.prox_regul(me, dev(img[z0:z1]), reg)
        same_bits(host(got), want[z0:z1], ("slab rank", z0, z1))
        with pytest.raises(ValueError, match="tolerance in z-slab mode"):
            R.prox_regul(me, dev(img[z0:z1]), dict(reg, tolerance=1e-3))


# ------------------------------------------------------------------------------------------------ drivers
LAM, INNER, NEIGHB = 0.05, 3, 8


@functools.lru_cache(maxsize=None)
def driver_tables():
    """tables for the drivers' volume, from the unregularised gradient step as the demo takes them from an FBP image"""
    from tomobar_amd.regularisersCuPy import PatchSelect_cupy
    step = G.rt().FISTA(G.data(), {"iterations": 1, "lipschitz_const": 3000.0, "recon_mask_radius": None}, None)
    return PatchSelect_cupy(step, 3, 1, NEIGHB, 0.05)


def driver_reg(**changed):
    hi, hj, w = driver_tables()
    return dict({"method": "NLTV", "regul_param": LAM, "iterations": INNER, "NLTV_H_i": hi, "NLTV_H_j": hj, "NLTV_Weights": w},
                **changed)


@pytest.fixture
def recorded(monkeypatch):
    """a recording wrapper round ops.nltv: (shape, lambda, iterations, tolerance) of every call"""
    from tomobar_amd import ops
    calls, real = [], ops.nltv
    driver_tables()

    def wrapper(data, out, *args, **kw):
        bound = inspect.signature(real).bind(data, out, *args, **kw)
        bound.apply_defaults()
        a = bound.arguments
        calls.append((tuple(data.shape), a["lam"], a["iterations"], a["tolerance"]))
        return real(data, out, *args, **kw)

    monkeypatch.setattr(ops, "nltv", wrapper)
    return calls


def _check_calls(calls, count, lam=LAM):
    assert len(calls) == count, (len(calls), count)
    for c in calls:
        assert c == ((G.NZ, G.NN, G.NN), f32(lam), INNER, 0.0) and type(c[1]) is f32, c


def test_fista_one_iteration_is_the_prox_of_the_gradient_step(recorded):
    from tomobar_amd.regularisersCuPy import NLTV_cupy
    from tomobar_amd.supp.suppTools import check_kwargs
    algo = {"iterations": 1, "lipschitz_const": 3000.0}
    got = G.rt().FISTA(G.data(), dict(algo), driver_reg())
    _check_calls(recorded, 1)
    step = G.rt().FISTA(G.data(), dict(algo, recon_mask_radius=None), None)    # the gradient step, unmasked
    want = NLTV_cupy(step, *driver_tables(), LAM, INNER)
    same_bits(host(want), N.nltv(host(step), *[host(t) for t in driver_tables()], LAM, INNER), "NLTV_cupy against the oracle")
    want = check_kwargs(want, cupyrun=True, recon_mask_radius=1.0)          # the mask, applied afterwards as the driver does
    same_bits(host(got), host(want), "FISTA, one iteration")
    assert not np.array_equal(host(got), host(check_kwargs(step.clone(), cupyrun=True, recon_mask_radius=1.0))), "the prox did nothing"


@pytest.mark.parametrize("driver", ["FISTA", "ADMM"])
def test_ordered_subsets_drivers_call_the_prox_every_sub_iteration(driver, recorded):
    algo = {"iterations": 2, "lipschitz_const": 3000.0}
    rho = 2.0
    if driver == "ADMM":
        algo["ADMM_rho_const"] = rho
    reg = driver_reg()
    got = host(getattr(G.rt(3), driver)(G.data(), dict(algo), reg))
    assert reg["regul_param"] == LAM and reg["iterations"] == INNER and reg["NumNeighb"] == NEIGHB, "the caller's values were rewritten"
    _check_calls(recorded, 2 * 3, LAM / (rho if driver == "ADMM" else 1.0))
    plain = host(getattr(G.rt(3), driver)(G.data(), dict(algo), None))
    assert len(recorded) == 6
    assert np.all(np.isfinite(got)) and not np.array_equal(got, plain)


def test_osem_runs_with_nltv_and_differs_from_the_unregularised_run(recorded):
    algo = {"iterations": 2}
    got = host(G.rt(3).OSEM(G.data(), dict(algo), driver_reg()))
    assert len(recorded) >= 1 and all(c[1:] == (f32(LAM), INNER, 0.0) for c in recorded)
    n_calls = len(recorded)
    plain = host(G.rt(3).OSEM(G.data(), dict(algo), None))
    assert len(recorded) == n_calls
    assert np.all(np.isfinite(got)) and not np.array_equal(got, plain)


def test_the_reference_demos_dictionary_runs_through_fista(recorded):
    """Demos/methods_IR_legacy/DemoFISTA_NLTV_2D.py: the iteration count under IterNumb, NumNeighb beside the tables"""
    hi, hj, w = driver_tables()
    reg = {"method": "NLTV", "regul_param": LAM, "iterations": INNER, "NLTV_H_i": hi, "NLTV_H_j": hj, "NLTV_Weights": w,
           "NumNeighb": NEIGHB, "IterNumb": INNER, "device_regulariser": "gpu"}
    got = host(G.rt(3).FISTA(G.data(), {"iterations": 2, "lipschitz_const": 3000.0}, reg))
    _check_calls(recorded, 2 * 3)
    assert np.all(np.isfinite(got))
    with pytest.raises(ValueError, match="NumNeighb"):
        G.rt(3).FISTA(G.data(), {"iterations": 1, "lipschitz_const": 3000.0}, dict(reg, NumNeighb=15))
    with pytest.raises(ValueError, match="NLTV_Weights"):
        G.rt(3).FISTA(G.data(), {"iterations": 1, "lipschitz_const": 3000.0}, {k: v for k, v in reg.items() if k != "NLTV_Weights"})
