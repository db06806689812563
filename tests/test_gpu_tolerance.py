"""MI355X tests of the tolerance keys: the tomo_rel_change kernel, early stopping inside tomo_pdtv_tol / tomo_roftv_tol, in
the six iterative drivers and over z-slabs.  Thresholds come from the oracle's own sequences by the rule of
tests/_tolerance_cases.py (tests/test_tolerance.py checks on the CPU that every case here satisfies it)."""
import math
import os
import socket
import sys
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.multiprocessing as mp  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _tolerance_cases as T  # noqa: E402


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. the kernel
def _exact_sums(x, ref):
    x64, r64 = x.astype(np.float64), ref.astype(np.float64)
    return math.fsum(((x64 - r64) ** 2).tolist()), math.fsum((x64 ** 2).tolist())


@pytest.mark.parametrize("count", [1, 2, 3, 4, 5, 63, 64, 65, 1000003, 2 ** 24])
def test_rel_change_kernel(count):
    """num and den within count * 2^-53 relative of the exactly rounded sums of the float64 terms (the worst case of summing
    `count` non-negative doubles in any order), the snapshot bit-equal to x, inputs untouched, identical bits on a second call"""
    from tomobar_amd import ops
    rng = np.random.default_rng(count)
    x_h = rng.standard_normal(count).astype(np.float32)
    r_h = (x_h + 0.1 * rng.standard_normal(count)).astype(np.float32)
    want = _exact_sums(x_h, r_h)
    offsets = [(0, 0, 0), (1, 1, 1), (2, 2, 2), (3, 3, 3), (0, 1, 2), (3, 0, 0), (1, 1, 3)] if count < 2 ** 24 else [(0, 0, 0), (1, 1, 1), (2, 0, 3)]
    for ox, orf, ok in offsets:
        xb, rb, kb = (torch.zeros(count + 8, device="cuda") for _ in range(3))
        x, ref, keep = xb[ox:ox + count], rb[orf:orf + count], kb[ok:ok + count]
        x.copy_(torch.from_numpy(x_h))
        ref.copy_(torch.from_numpy(r_h))
        for mode in ("absent", "separate", "aliasing"):
            ref.copy_(torch.from_numpy(r_h))
            kb.fill_(-7.0)
            k = None if mode == "absent" else (keep if mode == "separate" else ref)
            got = ops.rel_change(x, ref, k)
            for g, w in zip(got, want):
                assert abs(g - w) <= count * T.EPS53 * w, (count, (ox, orf, ok), mode, g, w)
            assert np.array_equal(host(x), x_h)
            assert np.array_equal(host(xb[:ox]), np.zeros(ox, np.float32)) and np.array_equal(host(xb[ox + count:]), np.zeros(8 - ox, np.float32))
            if mode == "aliasing":
                assert np.array_equal(host(ref), x_h)
                assert float(rb[:orf].abs().sum()) == 0.0 and float(rb[orf + count:].abs().sum()) == 0.0   # nothing written outside
                continue
            assert np.array_equal(host(ref), r_h)
            assert ops.rel_change(x, ref, k) == got, "two calls must give identical bits"
            if mode == "separate":
                assert np.array_equal(host(keep), x_h)
                assert bool((kb[:ok] == -7.0).all()) and bool((kb[ok + count:] == -7.0).all())   # nothing written outside
            else:
                assert bool((kb == -7.0).all())


def test_rel_change_empty_and_degenerate():
    from tomobar_amd import ops
    from tomobar_amd.convergence import relative_change
    e = torch.zeros(0, device="cuda")
    assert ops.rel_change(e, e) == (0.0, 0.0)
    z, o = torch.zeros(100, device="cuda"), torch.ones(100, device="cuda")
    assert relative_change(*ops.rel_change(z, z)) == 0.0 and relative_change(*ops.rel_change(z, o)) == math.inf
    assert ops.rel_change(o, z) == (100.0, 100.0)


# ------------------------------------------------------------------------------------------------ 2. inner loops
def _call_inner(name, iterations, **extra):
    from tomobar_amd import regularisersCuPy as R
    method, _, kw, _ = T.INNER_CASES[name]
    x = torch.from_numpy(T.inner_input(name)).cuda()
    if method == "PD_TV":
        out = R.PD_TV_cupy(x, kw["regularisation_parameter"], iterations, kw.get("methodTV", 0), kw.get("nonneg", 0), 8.0, 0,
                           kw.get("half_precision", False), **extra)
    else:
        out = R.ROF_TV_cupy(x, kw["regularisation_parameter"], iterations, kw["time_marching_parameter"], 0,
                            kw.get("half_precision", False), **extra)
    return host(out), R.last_prox()


def _inner_case(name, arith=None):
    method, _, kw, _ = T.INNER_CASES[name]
    half = bool(kw.get("half_precision", False))
    bit_exact = method == "ROF_TV" or half or (arith is not None and arith.exact)
    tol, stop, d_stop, never = T.inner_plan(name)
    got, (done, d) = _call_inner(name, T.INNER_ITERATIONS, tolerance=tol)
    print(f"{name}: tol {tol:.6e} -> stopped after {done} (oracle {stop}), d {d:.6e} (oracle {d_stop:.6e})")
    assert done == stop
    plain, (done_plain, d_plain) = _call_inner(name, stop)
    assert done_plain == stop and math.isnan(d_plain)
    assert np.array_equal(got, plain), "a stopped run must return what iterations = iterations_done returns"
    want = T.inner_oracle(name, stop)
    if arith is not None:
        arith.check(got, want, half=half, what=f"{name} stopped after {stop}")
    else:
        assert np.array_equal(got, want), float(np.abs(got - want).max())
    if bit_exact:
        assert abs(d - d_stop) <= got.size * T.EPS53 * d_stop, (d, d_stop)
    # a threshold below the whole sequence: all 66 iterations, today's result
    got, (done, d) = _call_inner(name, T.INNER_ITERATIONS, tolerance=never)
    assert done == T.INNER_ITERATIONS and d > never
    assert np.array_equal(got, _call_inner(name, T.INNER_ITERATIONS)[0])


@pytest.mark.parametrize("name", ["pd_3d", "pd_2d", "pd_2_slices"])
def test_pdtv_inner_tolerance(name, pd_arith):
    _inner_case(name, pd_arith)


def test_pdtv_inner_tolerance_half_nonneg_aniso(pd_arith):
    _inner_case("pd_3d_half_nonneg_aniso", pd_arith)


@pytest.mark.parametrize("name", ["rof_3d", "rof_2d_half"])
def test_roftv_inner_tolerance(name):
    _inner_case(name)


@pytest.mark.parametrize("name", ["pd_3d", "pd_2d", "rof_3d"])
def test_zero_tolerance_through_the_tol_entry_points(name, pd_arith):
    """tol = 0 through tomo_pdtv_tol / tomo_roftv_tol is tomo_pdtv / tomo_roftv; the input may alias the output"""
    from tomobar_amd import ops
    method, _, kw, _ = T.INNER_CASES[name]
    x = torch.from_numpy(T.inner_input(name)).cuda()
    a, b = torch.empty_like(x), torch.empty_like(x)
    for iterations in (0, 1, 4, 7, 12):
        if method == "PD_TV":
            s = T.O.pd_scalars(kw["regularisation_parameter"], 8.0)
            ops.pdtv(x, a, *s, iterations, 0, 0, False)
            _, done, d = ops.pdtv_tol(x, b, *s, iterations, 0, 0, False, 0.0)
        else:
            ops.roftv(x, a, np.float32(0.05), np.float32(0.005), iterations, False)
            _, done, d = ops.roftv_tol(x, b, np.float32(0.05), np.float32(0.005), iterations, False, 0.0)
        assert done == iterations and math.isnan(d) and np.array_equal(host(a), host(b)), iterations
    # in place, with a tolerance that stops the loop: the same as out of place
    tol, stop, _, _ = T.inner_plan(name)
    want, _ = _call_inner(name, stop)
    y = x.clone()
    if method == "PD_TV":
        _, done, _ = ops.pdtv_tol(y, y, *T.O.pd_scalars(kw["regularisation_parameter"], 8.0), T.INNER_ITERATIONS, 0, 0, False, tol)
    else:
        _, done, _ = ops.roftv_tol(y, y, np.float32(0.05), np.float32(0.005), T.INNER_ITERATIONS, False, tol)
    assert done == stop and np.array_equal(host(y), want.reshape(y.shape))
    with pytest.raises(ValueError):
        ops.roftv_tol(x, a, np.float32(0.05), np.float32(0.005), 6, False, -1.0)


# ------------------------------------------------------------------------------------------------ 3. outer loops
@pytest.mark.parametrize("name", T.GPU_OUTER)
def test_outer_tolerance(name):
    c = T.OUTER_CASES[name]
    tol, stop, never = T.outer_plan(name)
    b = torch.from_numpy(T.sinogram()).cuda()
    rt = T.make_rt(name)
    rec = host(T.run_driver(rt, name, b, tolerance=tol))
    run = rt.last_run
    print(f"{name}: tol {tol:.6e}, oracle stops after {stop}; run {run}")
    assert run["method"] == c["driver"] and run["iterations_done"] == stop and run["converged"] is True
    assert len(run["rel_change"]) == stop and run["prox_iterations"] == []
    want = T.outer_oracle(name, stop)
    r = float(np.linalg.norm(rec.astype(np.float64) - want) / np.linalg.norm(want))
    print(f"{name}: rel-L2 vs the oracle's loop of {stop} iterations = {r:.3e}, bit-equal {np.array_equal(rec, want)}")
    if c["driver"] == "CGLS":
        assert r < T.CGLS_TOL, r
    else:
        assert np.array_equal(rec, want), (r, float(np.abs(rec - want).max()))
        assert T.close_lists(run["rel_change"], list(T.outer_sequence(name)[:stop]), rec.size), run
    assert np.array_equal(rec, host(T.run_driver(T.make_rt(name), name, b, iterations=stop)))
    # never met: 15 iterations, the volume of the run without the key
    rec = host(T.run_driver(rt, name, b, tolerance=never))
    assert rt.last_run["iterations_done"] == T.OUTER_ITERATIONS and rt.last_run["converged"] is False
    rt2 = T.make_rt(name)
    assert np.array_equal(rec, host(T.run_driver(rt2, name, b)))
    assert rt2.last_run == {"method": c["driver"], "iterations_done": T.OUTER_ITERATIONS, "converged": False, "rel_change": [],
                            "prox_iterations": []}


def test_both_tolerances():
    name = "both_fista_os4_pdtv"
    inner_tol = T.inner_tolerance_of(name)
    tol, stop, _ = T.outer_plan(name, inner_tol)
    rt = T.make_rt(name)
    rec = host(T.run_driver(rt, name, torch.from_numpy(T.sinogram()).cuda(), tolerance=tol, reg_tolerance=inner_tol))
    run = rt.last_run
    print("both tolerances:", run)
    assert run["iterations_done"] == stop and run["converged"]
    assert len(run["prox_iterations"]) == stop * T.OUTER_CASES[name]["os"]
    assert np.array_equal(rec, T.outer_oracle_counts(name, stop, run["prox_iterations"]))
    assert run["prox_iterations"] == T.outer_oracle_inner_rule(name, stop, inner_tol)[1]


# ------------------------------------------------------------------------------------------------ 4. z-slabs: two ranks sharing the GPU
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _run_ranks(worker, name, plan, world=2, limit_s=300.0):
    ctx = mp.start_processes(worker, args=(world, _free_port(), name, "gpu", plan), nprocs=world, join=False, start_method="spawn")
    deadline = time.time() + limit_s
    try:
        while not ctx.join(timeout=5.0):
            if time.time() > deadline:
                raise AssertionError(f"{world} ranks did not finish within {limit_s:.0f} s")
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()


@pytest.mark.parametrize("name", ["slab_pd_3d", "slab_rof_3d"])
def test_two_rank_inner_tolerance(name):
    _run_ranks(T.slab_inner_worker, name, T.slab_inner_plan(name))


@pytest.mark.parametrize("name", ["slab_fista_os4_pdtv", "slab_admm_os1_roftv"])
def test_two_rank_outer_and_inner_tolerance(name):
    _run_ranks(T.slab_outer_worker, name, T.slab_outer_plan(name))
