"""CPU tests of the tolerance keys (early stopping of the IR loops and the TV operators): validation, the threshold rule
for every case the GPU file uses, and the drivers' control flow on the oracle stand-in backend (tests/_cpu_backend.py +
tests/_cpu_backend_tol.py) -- unsharded in this process, z-slabs in gloo ranks.  tests/test_gpu_tolerance.py runs the
same cases on the MI355X."""
import math
import os
import socket
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.multiprocessing as mp  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _tolerance_cases as T  # noqa: E402


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.fixture
def cpu_backend(monkeypatch):
    import _cpu_backend_tol
    return _cpu_backend_tol.install(monkeypatch)


# ------------------------------------------------------------------------------------------------ the rule itself
def test_relative_change_definition():
    from tomobar_amd.convergence import check_tolerance, inner_check_due, relative_change
    assert relative_change(0.0, 0.0) == 0.0 and relative_change(0.0, 5.0) == 0.0
    assert relative_change(2.0, 0.0) == math.inf
    assert relative_change(1.0, 4.0) == 0.5
    # checks after every 6th iteration while at least 3 of the requested ones remain
    assert [n for n in range(0, 67) if inner_check_due(n, 66)] == T.check_points(66) == list(range(6, 61, 6))
    assert [n for n in range(0, 31) if inner_check_due(n, 30)] == [6, 12, 18, 24]
    assert [n for n in range(0, 10) if inner_check_due(n, 9)] == [6] and not any(inner_check_due(n, 8) for n in range(9))
    assert check_tolerance(None, "t") == 0.0 and check_tolerance(1e-3, "t") == 1e-3 and check_tolerance(0, "t") == 0.0
    for bad in (-1e-3, float("nan"), float("inf"), -float("inf"), "small"):
        with pytest.raises(ValueError):
            check_tolerance(bad, "t")


def test_launch_plans_put_every_check_point_on_a_launch_boundary():
    """the slab plan (and tomo_pdtv's pd_plan, which tests/test_host_logic.py holds equal to it) cuts the iterations so that
    every iteration count the rule checks after is the end of a launch, for every iterations-per-launch the library can answer"""
    from tomobar_amd.convergence import inner_check_due
    from tomobar_amd.slab import pd_launch_plan
    for kmax in (1, 2, 3):
        for iterations in range(0, 80):
            ends = set(np.cumsum(pd_launch_plan(iterations, False, kmax)).tolist())
            assert all(n in ends for n in range(iterations + 1) if inner_check_due(n, iterations)), (kmax, iterations)


@pytest.mark.parametrize("name", sorted(T.INNER_CASES))
def test_threshold_rule_inner_cases(name):
    tol, stop, d_stop, never = T.inner_plan(name)
    seq = T.inner_sequence(name)
    assert stop in T.check_points() and stop >= 18 and d_stop < tol < seq[T.INNER_CASES[name][3] - 2] and never < min(seq)


@pytest.mark.parametrize("name", sorted(T.OUTER_CASES))
def test_threshold_rule_outer_cases(name):
    inner_tol = T.inner_tolerance_of(name) if name.startswith(("both_", "slab_")) else None
    tol, stop, never = T.outer_plan(name, inner_tol)
    assert 3 <= stop < T.OUTER_ITERATIONS and never < min(T.outer_sequence(name, inner_tol)) and tol > 0.0
    if inner_tol is not None:   # "stop at the 18th of 30 iterations" on the first proximal call
        assert T.outer_oracle_inner_rule(name, 1, inner_tol)[1][0] == 18


# ------------------------------------------------------------------------------------------------ validation
@pytest.mark.parametrize("bad", [-1e-3, float("nan"), float("inf"), -float("inf")])
def test_bad_tolerances_raise(cpu_backend, bad):
    from tomobar_amd.supp.dicts import dicts_check
    rt = T.make_rt("fista_os4_pdtv")
    data = lambda: {"projection_data": torch.from_numpy(T.sinogram())}  # noqa: E731
    with pytest.raises(ValueError):
        dicts_check(rt, data(), {"tolerance": bad}, None, method_run="FISTA")
    with pytest.raises(ValueError):
        dicts_check(rt, data(), {}, {"method": "PD_TV", "tolerance": bad}, method_run="FISTA")
    with pytest.raises(ValueError):
        T.make_rt("landweber").Landweber(data(), {"iterations": 2, "tolerance": bad})
    from tomobar_amd.regularisersCuPy import PD_TV_cupy, ROF_TV_cupy
    x = torch.from_numpy(T.inner_input("pd_2d"))
    with pytest.raises(ValueError):
        PD_TV_cupy(x, 0.05, 12, tolerance=bad)
    with pytest.raises(ValueError):
        ROF_TV_cupy(x, 0.05, 12, 0.005, tolerance=bad)


def test_defaults_unchanged_and_off(cpu_backend):
    from tomobar_amd.supp.dicts import dicts_check
    rt = T.make_rt("fista_os4_pdtv")
    _, a, r = dicts_check(rt, {"projection_data": torch.from_numpy(T.sinogram())}, None, {"method": "PD_TV"}, method_run="FISTA")
    assert a["tolerance"] == 0.0 and r["tolerance"] == 0.0
    # off: the full count, nothing recorded, no snapshot volume, and rel_change is never called
    cpu_backend.rel_change = None
    rec = T.run_driver(rt, "fista_os4_pdtv", torch.from_numpy(T.sinogram()), iterations=2)
    assert rt.last_run == {"method": "FISTA", "iterations_done": 2, "converged": False, "rel_change": [], "prox_iterations": []}
    assert np.array_equal(rec.numpy(), T.outer_oracle("fista_os4_pdtv", 2))


# ------------------------------------------------------------------------------------------------ inner loops (stand-in backend)
@pytest.mark.parametrize("name", ["pd_3d_half_nonneg_aniso", "pd_2d", "rof_3d"])
def test_inner_tolerance_through_the_operator_functions(cpu_backend, name):
    """PD_TV_cupy / ROF_TV_cupy pass the trailing `tolerance` keyword on and report through last_prox()"""
    from tomobar_amd import regularisersCuPy as R
    method, _, kw, _ = T.INNER_CASES[name]
    tol, stop, d_stop, never = T.inner_plan(name)
    x = torch.from_numpy(T.inner_input(name))

    def call(iterations, **extra):
        if method == "PD_TV":
            return R.PD_TV_cupy(x, kw["regularisation_parameter"], iterations, kw.get("methodTV", 0), kw.get("nonneg", 0), 8.0,
                                0, kw.get("half_precision", False), **extra)
        return R.ROF_TV_cupy(x, kw["regularisation_parameter"], iterations, kw["time_marching_parameter"], 0,
                             kw.get("half_precision", False), **extra)
    got = call(T.INNER_ITERATIONS, tolerance=tol)
    done, d = R.last_prox()
    assert done == stop and abs(d - d_stop) <= x.numel() * T.EPS53 * d_stop
    assert np.array_equal(got.numpy(), T.inner_oracle(name, stop))
    got = call(T.INNER_ITERATIONS, tolerance=never)
    assert R.last_prox()[0] == T.INNER_ITERATIONS and np.array_equal(got.numpy(), T.inner_oracle(name, T.INNER_ITERATIONS))
    call(12)
    assert R.last_prox()[0] == 12 and math.isnan(R.last_prox()[1])


# ------------------------------------------------------------------------------------------------ outer loops (stand-in backend)
def _check_outer(name, rt, rec, stop, bit_exact=True):
    want = T.outer_oracle(name, stop)
    if T.OUTER_CASES[name]["driver"] == "CGLS":
        r = np.linalg.norm(rec.astype(np.float64) - want) / np.linalg.norm(want)
        assert r < T.CGLS_TOL, r
    else:
        assert np.array_equal(rec, want), float(np.abs(rec - want).max())
        assert T.close_lists(rt.last_run["rel_change"], list(T.outer_sequence(name)[:stop]), rec.size), rt.last_run


@pytest.mark.parametrize("name", T.GPU_OUTER)
def test_outer_tolerance(cpu_backend, name, capsys):
    tol, stop, never = T.outer_plan(name)
    b = torch.from_numpy(T.sinogram())
    rt = T.make_rt(name)
    rec = T.run_driver(rt, name, b, tolerance=tol).numpy()
    run = rt.last_run
    assert run["method"] == T.OUTER_CASES[name]["driver"] and run["iterations_done"] == stop and run["converged"] is True
    assert len(run["rel_change"]) == stop and run["prox_iterations"] == []
    assert all(d >= tol for d in run["rel_change"][:-1]) and run["rel_change"][-1] < tol
    _check_outer(name, rt, rec, stop)
    # the same volume as asking for that many iterations
    assert np.array_equal(rec, T.run_driver(T.make_rt(name), name, b, iterations=stop).numpy())
    # never met: all 15, and the run without the key
    rec = T.run_driver(rt, name, b, tolerance=never).numpy()
    assert rt.last_run["iterations_done"] == T.OUTER_ITERATIONS and rt.last_run["converged"] is False
    assert len(rt.last_run["rel_change"]) == T.OUTER_ITERATIONS
    assert np.array_equal(rec, T.run_driver(T.make_rt(name), name, b).numpy())
    assert "stopped" not in capsys.readouterr().out


def test_verbose_run_prints_one_line_when_it_stops(cpu_backend, capsys):
    name = "fista_os1"
    tol, stop, _ = T.outer_plan(name)
    d, a, r = T.outer_dicts(name, tol)
    d["projection_data"] = torch.from_numpy(T.sinogram())
    T.make_rt(name).FISTA(d, dict(a, verbose=True), r)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if "stopped" in ln]
    assert len(lines) == 1 and f"iteration {stop}" in lines[0]


def test_fista_early_exit_still_resets_the_projector_state(cpu_backend):
    """the `finally:` of FISTA (planar residual layout, transposed copy invalidated) runs when the loop ends early"""
    name = "fista_os4_pdtv"
    tol, stop, _ = T.outer_plan(name)
    rt = T.make_rt(name)
    calls = []
    rt.Atools.set_residual_layout = lambda layout: calls.append(layout)
    rt.Atools.invalidate = lambda: calls.append("invalidate")
    T.run_driver(rt, name, torch.from_numpy(T.sinogram()), tolerance=tol)
    assert rt.last_run["iterations_done"] == stop and calls[-2:] == ["planar", "invalidate"]


def test_both_tolerances(cpu_backend):
    name = "both_fista_os4_pdtv"
    inner_tol = T.inner_tolerance_of(name)
    tol, stop, _ = T.outer_plan(name, inner_tol)
    rt = T.make_rt(name)
    rec = T.run_driver(rt, name, torch.from_numpy(T.sinogram()), tolerance=tol, reg_tolerance=inner_tol).numpy()
    run = rt.last_run
    assert run["iterations_done"] == stop and run["converged"]
    assert len(run["prox_iterations"]) == stop * T.OUTER_CASES[name]["os"]       # one entry per proximal call
    assert run["prox_iterations"] == T.outer_oracle_inner_rule(name, stop, inner_tol)[1]
    assert np.array_equal(rec, T.outer_oracle_counts(name, stop, run["prox_iterations"]))


# ------------------------------------------------------------------------------------------------ z-slabs (gloo ranks)
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", ["slab_pd_3d", "slab_pd_3d_half_nonneg_aniso", "slab_rof_3d"])
def test_slab_inner_tolerance(world, name):
    """22 slices over 2 ranks (11 + 11) and over 3 (8 + 7 + 7: uneven slabs, an interior rank)"""
    mp.start_processes(T.slab_inner_worker, args=(world, _free_port(), name, "cpu", T.slab_inner_plan(name)), nprocs=world, join=True,
                       start_method="spawn")


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", ["slab_fista_os4_pdtv", "slab_admm_os1_roftv"])
def test_slab_outer_and_inner_tolerance(world, name):
    mp.start_processes(T.slab_outer_worker, args=(world, _free_port(), name, "cpu", T.slab_outer_plan(name)), nprocs=world,
                       join=True, start_method="spawn")
