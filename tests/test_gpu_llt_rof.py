"""MI355X tests of the LLT_ROF regulariser: the shipped kernel against the float32 numpy restatement
tests/_llt_rof_oracle.py, bit for bit (there is no reference implementation: formula-level parity, unpinned;
docs/kernels/llt_rof.md), through ops.llt_rof, LLT_ROF_cupy, the tolerance rule, the z-slab states and driver, and the three
drivers that reach it through prox_regul."""
import math
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _cupy_standin  # noqa: E402
import _llt_rof_oracle as D  # noqa: E402

COUNTS = (1, 2, 7, 40)
# the two-deep clamps overlap (extents of 1, 2, 3), tiles are ragged (60 columns per wave, 8 rows per lane, 2 x 2 waves)
SHAPES_3D = [(7, 13, 37), (2, 2, 2), (3, 3, 3), (1, 5, 3), (5, 1, 3), (5, 3, 1), (3, 70, 131)]
SHAPES_2D = [(13, 37), (1, 37), (37, 1), (2, 3), (150, 200)]


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def _f32(p):
    return np.float32(p["lam_rof"]), np.float32(p["lam_llt"]), np.float32(p["tau"])


def _ops_llt_rof(f_host, p, iterations, tolerance=0.0):
    from tomobar_amd import ops
    x = torch.from_numpy(f_host).cuda()
    out = torch.full_like(x, float("nan"))
    _, done, d = ops.llt_rof(x, out, *_f32(p), iterations, tolerance)
    assert np.array_equal(host(x).view(np.uint32), f_host.view(np.uint32)), "the input was written"
    return host(out), done, d


def _same_bits(got, want, what):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, what
    if not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        raise AssertionError((what, f"{len(bad)} of {got.size} values differ, first at {tuple(bad[0])}",
                              float(np.abs(got.astype(np.float64) - want).max())))


# ------------------------------------------------------------------------------------------------ ops.llt_rof, nd as given
@pytest.mark.parametrize("pname", sorted(D.PARAMS))
@pytest.mark.parametrize("shape", SHAPES_3D + SHAPES_2D, ids=lambda s: "x".join(map(str, s)))
def test_ops_llt_rof_equals_the_oracle(shape, pname):
    p = D.PARAMS[pname]
    want = D.cached(shape, pname, COUNTS)
    f = D.phantom(shape)
    for n in COUNTS:
        got, done, d = _ops_llt_rof(f, p, n)     # (the output array is pre-filled with NaN, the input checked afterwards)
        assert done == n and math.isnan(d)
        _same_bits(got, want[n], (shape, pname, n))
    _same_bits(_ops_llt_rof(f, p, 0)[0], f, (shape, pname, 0))   # iters = 0 copies the input


@pytest.mark.parametrize("pname", sorted(D.PARAMS))
def test_several_tiles_and_z_chunks(pname):
    """(40, 150, 200): a workgroup covers 2 x 60 columns by 2 x 8 rows, so 2 x 10 workgroup tiles in x and y (4 waves wide in
    x, the last one ragged), and, small volumes being z-chunked, three z-chunks of 14, 14 and 12 planes: the second and the
    third start with the seam prologue (E3 of two planes and R3 of one from the planes below the seam)"""
    shape = (40, 150, 200)
    want = D.cached(shape, pname, (10,))[10]
    _same_bits(_ops_llt_rof(D.phantom(shape), D.PARAMS[pname], 10)[0], want, (shape, pname))


# ------------------------------------------------------------------------------------------------ LLT_ROF_cupy
def _lr_cupy(x, iterations=7, pname="A", **kw):
    from tomobar_amd.regularisersCuPy import LLT_ROF_cupy
    p = D.PARAMS[pname]
    return LLT_ROF_cupy(x, p["lam_rof"], p["lam_llt"], iterations, p["tau"], 0, **kw)


def test_llt_rof_cupy_surface(monkeypatch):
    from tomobar_amd.regularisersCuPy import LLT_ROF_cupy, last_prox
    plane = D.phantom((13, 37))
    want2d = D.cached((13, 37), "A", COUNTS)[7]
    # a singleton axis in each position runs the 2D kernels and keeps its shape
    for axis in range(3):
        x = torch.from_numpy(np.expand_dims(plane, axis)).cuda()
        got = _lr_cupy(x)
        assert tuple(got.shape) == tuple(x.shape)
        _same_bits(np.squeeze(host(got), axis), want2d, ("singleton axis", axis))
        assert last_prox()[0] == 7 and math.isnan(last_prox()[1])
    # a non-contiguous input; the input array is unchanged
    vol = D.phantom((7, 13, 37))
    want3d = D.cached((7, 13, 37), "B", COUNTS)[7]
    xt = torch.from_numpy(np.ascontiguousarray(vol.transpose(2, 1, 0))).cuda().permute(2, 1, 0)
    assert not xt.is_contiguous()
    keep = xt.clone()
    _same_bits(host(_lr_cupy(xt, pname="B")), want3d, "non-contiguous input")
    assert torch.equal(xt, keep), "the input array was written"
    # out=, and two calls give identical bits
    x = torch.from_numpy(vol).cuda()
    out = torch.full_like(x, float("nan"))
    res = _lr_cupy(x, pname="B", out=out)
    assert res.data_ptr() == out.data_ptr()
    _same_bits(host(out), want3d, "out=")
    _same_bits(host(_lr_cupy(x, pname="B")), host(out), "second call")
    assert np.array_equal(host(x), vol), "the input array was written"
    # a CuPy-like array in -> the same kind out
    cupy = _cupy_standin.install(monkeypatch)
    res = _lr_cupy(cupy.ndarray(x), pname="B")
    assert type(res) is cupy.ndarray and res.data.ptr != x.data_ptr()
    _same_bits(res.get(), want3d, "CuPy-like input")
    # errors: dtype, gpu_id, a bad tolerance, out aliasing the input, non-positive scalars
    with pytest.raises(ValueError, match="float32"):
        _lr_cupy(x.double())
    with pytest.raises(ValueError, match="gpu_device"):
        LLT_ROF_cupy(x, 0.3, 0.1, 3, 0.005, -1)
    with pytest.raises(ValueError):
        _lr_cupy(x, tolerance=-1.0)
    with pytest.raises(ValueError, match="alias"):
        _lr_cupy(x, out=x)
    for bad in (dict(lam_rof=0.0), dict(lam_llt=-1.0), dict(lam_llt=0.0), dict(tau=0.0)):
        kw = dict(lam_rof=0.3, lam_llt=0.1, tau=0.005)
        kw.update(bad)
        with pytest.raises(ValueError, match="positive"):
            LLT_ROF_cupy(x, kw["lam_rof"], kw["lam_llt"], 3, kw["tau"], 0)


def test_reserve_tv_scratch_for_llt_rof():
    from tomobar_amd import ops
    ops.reserve_tv_scratch((7, 13, 37), "cuda:0", "LLT_ROF")
    ops.reserve_tv_scratch((13, 37), "cuda:0", "LLT_ROF")
    _same_bits(_ops_llt_rof(D.phantom((7, 13, 37)), D.PARAMS["C"], 7)[0], D.cached((7, 13, 37), "C", COUNTS)[7], "after reserve")


# ------------------------------------------------------------------------------------------------ tolerance
def test_tolerance_stops_where_the_oracle_sequence_stops():
    from tomobar_amd.regularisersCuPy import last_prox
    c = D.TOL_CASE
    tol, stop, d_stop, seq = D.tolerance_plan()
    x = torch.from_numpy(D.phantom(c["shape"])).cuda()
    got = host(_lr_cupy(x, c["iterations"], c["pname"], tolerance=tol))
    done, d = last_prox()
    print(f"LLT_ROF tolerance {tol:.6e}: stopped after {done} (oracle {stop}), d {d:.6e} (oracle {d_stop:.6e})")
    assert done == stop
    assert abs(d - d_stop) <= got.size * 2.0 ** -53 * d_stop
    plain = host(_lr_cupy(x, stop, c["pname"]))
    assert last_prox()[0] == stop and math.isnan(last_prox()[1])
    _same_bits(got, plain, "a stopped run returns what iterations = n returns")
    _same_bits(got, D.cached(c["shape"], c["pname"], tuple(range(6, 61, 6)))[stop], "stopped run against the oracle")
    # an odd request: iterate 24 then lives in the work array and is copied to the output
    got_odd = host(_lr_cupy(x, c["iterations"] - 1, c["pname"], tolerance=tol))
    assert last_prox()[0] == stop
    _same_bits(got_odd, plain, "a stopped run of an odd request")
    # a threshold below the whole sequence: every iteration runs
    never = 0.5 * min(seq)
    full = host(_lr_cupy(x, c["iterations"], c["pname"], tolerance=never))
    done, d = last_prox()
    assert done == c["iterations"] and d > never
    _same_bits(full, host(_lr_cupy(x, c["iterations"], c["pname"])), "tolerance never met")


# ------------------------------------------------------------------------------------------------ z-slabs on the one GPU
def _copy_halos(states, it):
    """rank r's send_up -> rank r+1's recv_down; rank r+1's send_down -> rank r's recv_up (planes of iterate `it`)"""
    for r in range(len(states) - 1):
        lo, hi = states[r], states[r + 1]
        for src, dst in zip(lo.send_up(it), hi.recv_down(it)):
            dst.copy_(src)
        for src, dst in zip(hi.send_down(it), lo.recv_up(it)):
            dst.copy_(src)


def _run_slabs(vd, bounds, schedule, pname, iters):
    from tomobar_amd.slab import LltRofSlab, _hip_llt_rof_step
    states = []
    for r, (z0, z1) in enumerate(bounds):
        states.append(LltRofSlab(vd[z0:z1].contiguous(), r > 0, r < len(bounds) - 1, _hip_llt_rof_step))
        for t in states[-1].U:
            t.fill_(float("nan"))
    _copy_halos(states, 0)
    args = _f32(D.PARAMS[pname])
    for it in range(iters):
        if schedule == "ranges":  # the overlapped order: boundary planes, "exchange", interior
            for s in states:
                for zr in s.boundary_ranges()[0]:
                    s.step(it, *args, zr)
            _copy_halos(states, it + 1)
            for s in states:
                s.step(it, *args, s.boundary_ranges()[1])
            continue
        for s in states:
            s.step(it, *args)
        _copy_halos(states, it + 1)
    return host(torch.cat([s.local(s.source(iters)) for s in states]))


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("schedule", ["plain", "ranges"])
@pytest.mark.parametrize("pname", sorted(D.PARAMS))
def test_llt_rof_slabs_equal_whole_volume(world, schedule, pname, shape=(19, 21, 90), iters=6):
    from tomobar_amd.slab import slab_bounds
    vd = torch.from_numpy(D.phantom(shape)).cuda()
    want = host(_lr_cupy(vd, iters, pname))
    _same_bits(want, D.cached(shape, pname, (iters,))[iters], "whole volume against the oracle")
    got = _run_slabs(vd, [slab_bounds(shape[0], world, r) for r in range(world)], schedule, pname, iters)
    _same_bits(got, want, (shape, world, schedule, pname))


@pytest.mark.parametrize("schedule", ["plain", "ranges"])
@pytest.mark.parametrize("bounds", [[(0, 2), (2, 19)], [(0, 9), (9, 11), (11, 19)], [(0, 17), (17, 19)]],
                         ids=["2+17", "9+2+8", "17+2"])
def test_llt_rof_slab_of_exactly_two_planes(bounds, schedule, shape=(19, 21, 90), iters=6):
    """one rank owns exactly two planes: both are boundary planes, and both of its neighbour's ghost planes come from it"""
    vd = torch.from_numpy(D.phantom(shape)).cuda()
    want = D.cached(shape, "A", (iters,))[iters]
    _same_bits(_run_slabs(vd, bounds, schedule, "A", iters), want, (bounds, schedule))


@pytest.mark.parametrize("pname", sorted(D.PARAMS))
def test_llt_rof_slab_driver_on_one_rank_equals_llt_rof_cupy(pname):
    from tomobar_amd.slab import SlabComm, llt_rof_slab
    p = D.PARAMS[pname]
    vd = torch.from_numpy(D.phantom((19, 21, 90))).cuda()
    want = host(_lr_cupy(vd, 7, pname))
    got = llt_rof_slab(vd, SlabComm(0, 1), p["lam_rof"], p["lam_llt"], 7, p["tau"])
    _same_bits(host(got), want, pname)
    out = torch.full_like(vd, float("nan"))
    info = {}
    assert llt_rof_slab(vd, SlabComm(0, 1), p["lam_rof"], p["lam_llt"], 7, p["tau"], out=out, info=info) is out
    _same_bits(host(out), want, (pname, "out="))
    assert info["iterations_done"] == 7 and math.isnan(info["rel_change"])
    _same_bits(host(llt_rof_slab(vd, SlabComm(0, 1), p["lam_rof"], p["lam_llt"], 0, p["tau"])), host(vd), "zero iterations")


# ------------------------------------------------------------------------------------------------ drivers
NZ, NN, NA = 6, 32, 48
ANGLES = np.linspace(0, np.pi, NA, endpoint=False)
REG = dict(method="LLT_ROF", regul_param=0.5, regul_param2=0.25, iterations=5, time_marching_step=0.01)


def _sino():
    return torch.from_numpy(np.random.default_rng(11).random((NZ, NA, NN)).astype(np.float32)).cuda()


def _data():
    return {"projection_data": _sino(), "data_axes_labels_order": ["detY", "angles", "detX"]}


def _rt(os_number=None):
    from tomobar_amd.methodsIR_CuPy import RecToolsIRCuPy
    return RecToolsIRCuPy(NN, 0, NZ, 0.0, ANGLES, NN, 0, os_number)


@pytest.fixture
def recorded(monkeypatch):
    """a recording wrapper round ops.llt_rof: the scalars of every call"""
    from tomobar_amd import ops
    calls, real = [], ops.llt_rof

    def wrapper(data, out, lam_rof, lam_llt, tau, iterations, tolerance=0.0):
        calls.append((tuple(data.shape), lam_rof, lam_llt, tau, iterations, tolerance))
        return real(data, out, lam_rof, lam_llt, tau, iterations, tolerance)

    monkeypatch.setattr(ops, "llt_rof", wrapper)
    return calls


def _check_calls(calls, count, regul_param, regul_param2):
    assert len(calls) == count, (len(calls), count)
    want = ((NZ, NN, NN), np.float32(regul_param), np.float32(regul_param2), np.float32(REG["time_marching_step"]),
            REG["iterations"], 0.0)
    for c in calls:
        assert c == want and all(type(a) is type(b) for a, b in zip(c[1:4], want[1:4])), (c, want)


def test_fista_one_iteration_is_the_prox_of_the_gradient_step(recorded):
    from tomobar_amd.regularisersCuPy import LLT_ROF_cupy
    from tomobar_amd.supp.suppTools import check_kwargs
    algo = {"iterations": 1, "lipschitz_const": 3000.0}
    got = _rt().FISTA(_data(), dict(algo), dict(REG))
    _check_calls(recorded, 1, REG["regul_param"], REG["regul_param2"])
    step = _rt().FISTA(_data(), dict(algo, recon_mask_radius=None), None)    # the gradient step, unmasked
    want = LLT_ROF_cupy(step, REG["regul_param"], REG["regul_param2"], REG["iterations"], REG["time_marching_step"], 0)
    want = check_kwargs(want, cupyrun=True, recon_mask_radius=1.0)          # the mask, applied afterwards as the driver does
    _same_bits(host(got), host(want), "FISTA, one iteration")
    assert not np.array_equal(host(got), host(check_kwargs(step.clone(), cupyrun=True, recon_mask_radius=1.0))), "the prox did nothing"


@pytest.mark.parametrize("driver", ["FISTA", "ADMM"])
def test_ordered_subsets_drivers_call_the_prox_every_sub_iteration(driver, recorded):
    algo = {"iterations": 2, "lipschitz_const": 3000.0}
    rho = 2.0
    if driver == "ADMM":
        algo["ADMM_rho_const"] = rho
    reg = dict(REG)
    got = host(getattr(_rt(3), driver)(_data(), dict(algo), reg))
    # dicts_check adds its defaults to the caller's dictionary; ADMM's regul_param / rho and regul_param2 / rho go to a copy
    assert {k: reg[k] for k in REG} == REG, "the caller's values were rewritten"
    div = rho if driver == "ADMM" else 1.0
    _check_calls(recorded, 2 * 3, REG["regul_param"] / div, REG["regul_param2"] / div)
    plain = host(getattr(_rt(3), driver)(_data(), dict(algo), None))
    assert len(recorded) == 6
    assert np.all(np.isfinite(got)) and not np.array_equal(got, plain)


def test_osem_runs_with_llt_rof_and_differs_from_the_unregularised_run(recorded):
    algo = {"iterations": 2}
    got = host(_rt(3).OSEM(_data(), dict(algo), dict(REG, regul_param2=0.05)))
    assert len(recorded) >= 1 and all(c[2] == np.float32(0.05) for c in recorded)
    n_calls = len(recorded)
    plain = host(_rt(3).OSEM(_data(), dict(algo), None))
    assert len(recorded) == n_calls
    assert np.all(np.isfinite(got)) and not np.array_equal(got, plain)
