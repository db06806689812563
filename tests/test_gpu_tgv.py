"""MI355X tests of the TGV prox: the shipped kernels against the float32 numpy restatement tests/_tgv_oracle.py, bit for bit
(there is no reference implementation: formula-level parity, unpinned; docs/kernels/tgv.md), through ops.tgv, TGV_cupy,
the tolerance rule and the three drivers that reach it through prox_regul."""
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
import _tgv_oracle as T  # noqa: E402

COUNTS = (1, 2, 7, 40)
SHAPES_3D = [(7, 13, 37), (2, 2, 2), (1, 5, 3), (5, 1, 3), (5, 3, 1), (3, 70, 131)]
SHAPES_2D = [(13, 37), (1, 37), (37, 1), (2, 3), (150, 200)]


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def _scalars(params):
    return T.scalars(params["lam"], params["alpha1"], params["alpha0"], params["L"])


def _ops_tgv(f_host, params, iterations, tolerance=0.0):
    from tomobar_amd import ops
    x = torch.from_numpy(f_host).cuda()
    out = torch.full_like(x, float("nan"))
    _, done, d = ops.tgv(x, out, *_scalars(params), iterations, tolerance)
    assert np.array_equal(host(x), f_host), "the input was written"
    return host(out), done, d


def _same_bits(got, want, what):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, what
    if not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        raise AssertionError((what, f"{len(bad)} of {got.size} values differ, first at {tuple(bad[0])}",
                              float(np.abs(got.astype(np.float64) - want).max())))


# ------------------------------------------------------------------------------------------------ ops.tgv, nd as given
@pytest.mark.parametrize("pname", ["A", "B"])
@pytest.mark.parametrize("shape", SHAPES_3D + SHAPES_2D, ids=lambda s: "x".join(map(str, s)))
def test_ops_tgv_equals_the_oracle(shape, pname):
    params = T.PARAMS_A if pname == "A" else T.PARAMS_B
    want = T.cached(shape, pname, COUNTS)
    f = T.phantom(shape)
    for n in COUNTS:
        got, done, d = _ops_tgv(f, params, n)
        assert done == n and math.isnan(d)
        _same_bits(got, want[n], (shape, pname, n))
    _same_bits(_ops_tgv(f, params, 0)[0], f, (shape, pname, 0))   # iters = 0 copies the input


def test_several_tiles_and_z_chunks():
    """(40, 150, 200): 2 x 19 workgroup tiles in x and y and, small volumes being z-chunked, three z-chunks of 14 planes"""
    shape = (40, 150, 200)
    want = T.cached(shape, "A", (10,))[10]
    _same_bits(_ops_tgv(T.phantom(shape), T.PARAMS_A, 10)[0], want, shape)


# ------------------------------------------------------------------------------------------------ TGV_cupy
def _tgv_cupy(x, iterations=7, **kw):
    from tomobar_amd.regularisersCuPy import TGV_cupy
    p = T.PARAMS_A
    return TGV_cupy(x, p["lam"], iterations, p["alpha1"], p["alpha0"], p["L"], 0, **kw)


def test_tgv_cupy_surface(monkeypatch):
    from tomobar_amd.regularisersCuPy import last_prox
    plane = T.phantom((13, 37))
    want2d = T.cached((13, 37), "A", COUNTS)[7]
    # a singleton axis in each position runs the 2D kernels and keeps its shape
    for axis in range(3):
        x = torch.from_numpy(np.expand_dims(plane, axis)).cuda()
        got = _tgv_cupy(x)
        assert tuple(got.shape) == tuple(x.shape)
        _same_bits(np.squeeze(host(got), axis), want2d, ("singleton axis", axis))
        assert last_prox()[0] == 7 and math.isnan(last_prox()[1])
    # a non-contiguous input; the input array is unchanged
    vol = T.phantom((7, 13, 37))
    want3d = T.cached((7, 13, 37), "A", COUNTS)[7]
    xt = torch.from_numpy(np.ascontiguousarray(vol.transpose(2, 1, 0))).cuda().permute(2, 1, 0)
    assert not xt.is_contiguous()
    keep = xt.clone()
    got = _tgv_cupy(xt)
    _same_bits(host(got), want3d, "non-contiguous input")
    assert torch.equal(xt, keep), "the input array was written"
    # out=, and two calls give identical bits
    x = torch.from_numpy(vol).cuda()
    out = torch.full_like(x, float("nan"))
    res = _tgv_cupy(x, out=out)
    assert res.data_ptr() == out.data_ptr()
    _same_bits(host(out), want3d, "out=")
    _same_bits(host(_tgv_cupy(x)), host(out), "second call")
    assert np.array_equal(host(x), vol), "the input array was written"
    # a CuPy-like array in -> the same kind out
    cupy = _cupy_standin.install(monkeypatch)
    res = _tgv_cupy(cupy.ndarray(x))
    assert type(res) is cupy.ndarray and res.data.ptr != x.data_ptr()
    _same_bits(res.get(), want3d, "CuPy-like input")
    with pytest.raises(ValueError):
        _tgv_cupy(x, tolerance=-1.0)


# ------------------------------------------------------------------------------------------------ tolerance
def test_tolerance_stops_where_the_oracle_sequence_stops():
    from tomobar_amd.regularisersCuPy import TGV_cupy, last_prox
    c = T.TOL_CASE
    tol, stop, d_stop, seq = T.tolerance_plan()
    p = T.PARAMS_A
    x = torch.from_numpy(T.phantom(c["shape"])).cuda()
    got = host(TGV_cupy(x, p["lam"], c["iterations"], p["alpha1"], p["alpha0"], p["L"], 0, tolerance=tol))
    done, d = last_prox()
    print(f"TGV tolerance {tol:.6e}: stopped after {done} (oracle {stop}), d {d:.6e} (oracle {d_stop:.6e})")
    assert done == stop
    assert abs(d - d_stop) <= got.size * 2.0 ** -53 * d_stop
    plain = host(TGV_cupy(x, p["lam"], stop, p["alpha1"], p["alpha0"], p["L"], 0))
    assert last_prox()[0] == stop and math.isnan(last_prox()[1])
    _same_bits(got, plain, "a stopped run returns what iterations = n returns")
    _same_bits(got, T.cached(c["shape"], c["pname"], tuple(range(6, 61, 6)))[stop], "stopped run against the oracle")
    # a threshold below the whole sequence: every iteration runs
    never = 0.5 * min(seq)
    full = host(TGV_cupy(x, p["lam"], c["iterations"], p["alpha1"], p["alpha0"], p["L"], 0, tolerance=never))
    done, d = last_prox()
    assert done == c["iterations"] and d > never
    _same_bits(full, host(TGV_cupy(x, p["lam"], c["iterations"], p["alpha1"], p["alpha0"], p["L"], 0)), "tolerance never met")


# ------------------------------------------------------------------------------------------------ drivers
NZ, N, NA = 6, 32, 48
ANGLES = np.linspace(0, np.pi, NA, endpoint=False)
REG = dict(method="TGV", regul_param=0.02, iterations=5, TGV_alpha1=0.8, TGV_alpha2=1.7, PD_LipschitzConstant=10.0)


def _sino():
    return torch.from_numpy(np.random.default_rng(11).random((NZ, NA, N)).astype(np.float32)).cuda()


def _data():
    return {"projection_data": _sino(), "data_axes_labels_order": ["detY", "angles", "detX"]}


def _rt(os_number=None):
    from tomobar_amd.methodsIR_CuPy import RecToolsIRCuPy
    return RecToolsIRCuPy(N, 0, NZ, 0.0, ANGLES, N, 0, os_number)


@pytest.fixture
def recorded(monkeypatch):
    """a recording wrapper round ops.tgv: the scalars of every call"""
    from tomobar_amd import ops
    calls, real = [], ops.tgv

    def wrapper(data, out, lam, alpha1, alpha0, tau, sigma, iterations, tolerance=0.0):
        calls.append((tuple(data.shape), lam, alpha1, alpha0, tau, sigma, iterations, tolerance))
        return real(data, out, lam, alpha1, alpha0, tau, sigma, iterations, tolerance)

    monkeypatch.setattr(ops, "tgv", wrapper)
    return calls


def _expected_call(regul_param):
    tau = np.float32(np.float32(1.0) / np.sqrt(np.float32(REG["PD_LipschitzConstant"])))
    return ((NZ, N, N), np.float32(regul_param), np.float32(REG["TGV_alpha1"]), np.float32(REG["TGV_alpha2"]), tau, tau,
            REG["iterations"], 0.0)


def _check_calls(calls, count, regul_param):
    assert len(calls) == count, (len(calls), count)
    want = _expected_call(regul_param)
    for c in calls:
        assert c == want and all(type(a) is type(b) for a, b in zip(c[1:6], want[1:6])), (c, want)


def test_fista_one_iteration_is_the_prox_of_the_gradient_step(recorded):
    from tomobar_amd.regularisersCuPy import TGV_cupy
    from tomobar_amd.supp.suppTools import check_kwargs
    algo = {"iterations": 1, "lipschitz_const": 3000.0}
    got = _rt().FISTA(_data(), dict(algo), dict(REG))
    _check_calls(recorded, 1, REG["regul_param"])
    step = _rt().FISTA(_data(), dict(algo, recon_mask_radius=None), None)    # the gradient step, unmasked
    want = TGV_cupy(step, REG["regul_param"], REG["iterations"], REG["TGV_alpha1"], REG["TGV_alpha2"], REG["PD_LipschitzConstant"], 0)
    want = check_kwargs(want, cupyrun=True, recon_mask_radius=1.0)          # the mask, applied afterwards as the driver does
    _same_bits(host(got), host(want), "FISTA, one iteration")


@pytest.mark.parametrize("driver", ["FISTA", "ADMM"])
def test_ordered_subsets_drivers_call_the_prox_every_sub_iteration(driver, recorded):
    algo = {"iterations": 2, "lipschitz_const": 3000.0}
    rho = 2.0
    if driver == "ADMM":
        algo["ADMM_rho_const"] = rho
    reg = dict(REG)
    got = host(getattr(_rt(3), driver)(_data(), dict(algo), reg))
    # dicts_check adds its defaults to the caller's dictionary; ADMM's regul_param / rho goes to a copy
    assert {k: reg[k] for k in REG} == REG, "the caller's values were rewritten"
    _check_calls(recorded, 2 * 3, REG["regul_param"] / rho if driver == "ADMM" else REG["regul_param"])
    plain = host(getattr(_rt(3), driver)(_data(), dict(algo), None))
    assert len(recorded) == 6
    assert np.all(np.isfinite(got)) and not np.array_equal(got, plain)
