"""Slice-wise PD_TV / ROF_TV on the MI355X (tomobar_amd/csrc/tv_slices.hip, docs/kernels/slicewise.md) against code the
slice-wise path does not touch: the 2D path of the same library called once per slice, and the CPU oracle's 2D operator
called once per slice.  ROF_TV (float32 and binary16 D fields), PD_TV with binary16 duals and PD_TV with variant 22 must
reproduce both bit for bit; the default (relaxed float32) PD_TV must equal the per-slice calls bit for bit and lie within
1e-5 relative L2 of the oracle (the `pd_arith` fixture of tests/conftest.py: the bound of the existing PD_TV tests).
Inputs, shapes and the tolerance cases: tests/_slicewise_cases.py (the CPU file checks what they promise)."""
import os
import sys
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _pd_relaxed as R  # noqa: E402
import _slicewise_cases as S  # noqa: E402

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def same_bits(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), (what, float(np.abs(got - want).max()), int((got != want).sum()))


def pd(x, slicewise=False, out=None, tolerance=0.0, **kw):
    from tomobar_amd.regularisersCuPy import PD_TV_cupy
    return PD_TV_cupy(x, kw["regularisation_parameter"], kw["iterations"], kw["methodTV"], kw["nonneg"], kw["lipschitz_const"], 0,
                      kw["half_precision"], out=out, tolerance=tolerance, slicewise=slicewise)


def rof(x, slicewise=False, out=None, tolerance=0.0, **kw):
    from tomobar_amd.regularisersCuPy import ROF_TV_cupy
    return ROF_TV_cupy(x, kw["regularisation_parameter"], kw["iterations"], kw["time_marching_parameter"], 0,
                       kw["half_precision"], out=out, tolerance=tolerance, slicewise=slicewise)


def _elementwise(pd_arith, got, vol, kw, what):
    """the shipped default with float32 duals, element for element against the relaxed model (tests/_pd_relaxed.py): bit
    equality where the model has no hardware-dependent operation, else within four times the family's envelope"""
    if pd_arith.exact or kw["half_precision"]:
        return
    mark = len(R.STATS)
    R.check_elementwise(got, vol, R.params(kw["regularisation_parameter"], kw["iterations"], kw["methodTV"], kw["nonneg"],
                                           kw["lipschitz_const"], slices=True), what=what)
    print(R.summary(mark, what))


def per_slice(fn, x, **kw):
    """today's 2D path of the library, once per slice (a 2D input comes back with a leading singleton axis, as from the
    reference)"""
    return np.stack([host(fn(x[k].contiguous(), **kw)).reshape(tuple(x.shape[1:])) for k in range(x.shape[0])])


# ------------------------------------------------------------------------------------------------ the two yardsticks
@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("case", S.ROF_CASES, ids=S.case_id)
def test_rof_tv_equals_the_2d_path_and_the_oracle_per_slice(case, half):
    shape, iters = case
    vol, kw = S.volume(shape), S.rof_kwargs(iters, half)
    x = dev(vol)
    got = host(rof(x, slicewise=True, **kw))
    same_bits(got, per_slice(rof, x, **kw), "2D path per slice")
    want = S.oracle_slices("ROF_TV", vol, **kw)
    same_bits(got, want, "oracle per slice")
    if shape in S.DISTINCT_SHAPES and iters == 7:   # the input tells slice-wise from 3D: 3-6e-3 on the oracle
        gap = float(np.abs(S.oracle_3d("ROF_TV", vol, **kw) - want).max())
        print(f"ROF_TV {shape}: 3D vs slice-wise {gap:.3e}")
        assert gap > 1e-3
        assert not np.array_equal(got, host(rof(x, **kw)))


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("case", S.PD_CASES, ids=S.case_id)
def test_pd_tv_equals_the_2d_path_and_the_oracle_per_slice(case, half, pd_arith):
    shape, iters = case
    vol, kw = S.volume(shape), S.pd_kwargs(iters, half=half)
    x = dev(vol)
    got = host(pd(x, slicewise=True, **kw))
    same_bits(got, per_slice(pd, x, **kw), "2D path per slice")
    want = S.oracle_slices("PD_TV", vol, **kw)
    r = pd_arith.check(got, want, half=half, what=f"slicewise PD_TV {shape} x{iters}")
    _elementwise(pd_arith, got, vol, kw, f"slicewise PD_TV {shape} x{iters}")
    print(f"PD_TV {shape} x{iters} {pd_arith.name} half={half}: rel-L2 vs oracle {r:.3e}")
    if shape in S.DISTINCT_SHAPES and iters == 7:   # 0.13-0.16 on the oracle
        gap = float(np.abs(S.oracle_3d("PD_TV", vol, **kw) - want).max())
        print(f"PD_TV {shape}: 3D vs slice-wise {gap:.3e}")
        assert gap > 0.05
        assert not np.array_equal(got, host(pd(x, **kw)))


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("methodTV, nonneg", [(1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("case", S.FLAG_SHAPES, ids=S.case_id)
def test_pd_tv_flags(case, methodTV, nonneg, half, pd_arith):
    shape, iters = case
    vol, kw = S.volume(shape), S.pd_kwargs(iters, methodTV, nonneg, half)
    x = dev(vol)
    got = host(pd(x, slicewise=True, **kw))
    same_bits(got, per_slice(pd, x, **kw), "2D path per slice")
    want = S.oracle_slices("PD_TV", vol, **kw)
    pd_arith.check(got, want, half=half, what=f"slicewise PD_TV {shape} x{iters} methodTV={methodTV} nonneg={nonneg}")
    _elementwise(pd_arith, got, vol, kw, f"slicewise PD_TV {shape} x{iters} methodTV={methodTV} nonneg={nonneg}")
    if nonneg:   # the switch is live on this input: slice 0 is noise around zero
        assert not np.array_equal(want, S.oracle_slices("PD_TV", vol, **dict(kw, nonneg=0)))


# ------------------------------------------------------------------------------------------------ properties
OPERATORS = [("PD_TV", False), ("PD_TV", True), ("ROF_TV", False), ("ROF_TV", True)]
OP_IDS = ["pd-f32", "pd-f16", "rof-f32", "rof-f16"]


def _op(method, half, iters=7):
    return (pd, S.pd_kwargs(iters, half=half)) if method == "PD_TV" else (rof, S.rof_kwargs(iters, half))


@pytest.mark.parametrize("method, half", OPERATORS, ids=OP_IDS)
def test_changing_one_slice_leaves_the_others_bit_identical(method, half):
    fn, kw = _op(method, half)
    shape, k = (5, 17, 117), 2
    a = host(fn(dev(S.volume(shape)), slicewise=True, **kw))
    b = host(fn(dev(S.volume(shape, changed=k)), slicewise=True, **kw))
    for z in range(shape[0]):
        if z == k:
            assert not np.array_equal(a[z], b[z])
        else:
            same_bits(a[z], b[z], f"slice {z}")


class _NoComm:
    """a communicator that must not be touched: every attribute access is an error"""

    def __getattribute__(self, name):
        raise AssertionError(f"the communicator was touched: {name}")


def _self(slab=None):
    return types.SimpleNamespace(nonneg_regul=0, Atools=types.SimpleNamespace(device_index=0), slab=slab)


def _reg(method, half, iters=7, **more):
    return dict(method=method, regul_param=S.LAM, iterations=iters, time_marching_step=S.ROF_TAU, methodTV=0,
                PD_LipschitzConstant=S.LIPSCHITZ, half_precision=half, slicewise=True, **more)


@pytest.mark.parametrize("method, half", OPERATORS, ids=OP_IDS)
def test_a_volume_split_into_slabs_equals_the_whole_run(method, half):
    from tomobar_amd.regularisersCuPy import last_prox, prox_regul, reserve_prox_scratch
    fn, kw = _op(method, half)
    x = dev(S.volume((5, 17, 117)))
    reg = _reg(method, half)
    reserve_prox_scratch(_self(), x.shape, reg)
    whole = host(prox_regul(_self(), x, dict(reg)))
    assert last_prox()[0] == 7
    same_bits(whole, host(fn(x, slicewise=True, **kw)), "prox_regul vs the function")
    parts = [host(prox_regul(_self(_NoComm()), x[a:b].contiguous(), dict(reg))) for a, b in ((0, 2), (2, 5))]
    same_bits(np.concatenate(parts), whole, "2 + 3 slices")
    with pytest.raises(ValueError, match="does not take a tolerance in z-slab mode"):
        prox_regul(_self(_NoComm()), x, dict(reg, tolerance=1e-3))
    # without the key the same dictionary runs 3D TV
    plain = dict(reg)
    del plain["slicewise"]
    assert not np.array_equal(host(prox_regul(_self(), x, plain)), whole)


@pytest.mark.parametrize("method, half", OPERATORS, ids=OP_IDS)
def test_out_argument_singleton_axis_and_zero_iterations(method, half):
    fn, kw = _op(method, half)
    x = dev(S.volume((3, 9, 59)))
    want = host(fn(x, slicewise=True, **kw))
    out = torch.full_like(x, float("nan"))
    res = fn(x, slicewise=True, out=out, **kw)
    assert res.data_ptr() == out.data_ptr()
    same_bits(host(out), want, "out=")
    # a singleton axis runs the 2D kernels, key or no key
    flat = x[:1].contiguous()
    same_bits(host(fn(flat, slicewise=True, **kw)), host(fn(flat, **kw)), "singleton axis")
    same_bits(host(fn(x[0].contiguous(), slicewise=True, **kw)), host(fn(x[0].contiguous(), **kw)), "2D input")
    same_bits(host(fn(flat, **kw))[0], want[0], "slice 0")
    same_bits(host(fn(x, slicewise=True, **dict(kw, iterations=0))), host(x), "iterations = 0")


def test_argument_checks_of_the_entry_points():
    from tomobar_amd import _lib, ops
    x = dev(S.volume((3, 9, 59)))
    out = torch.empty_like(x)
    with pytest.raises(ValueError, match="ROF_TV needs every dimension >= 2"):
        ops.roftv_slices(x[:, :, :1].contiguous(), out[:, :, :1].contiguous(), 0.05, 0.005, 3, False)
    with pytest.raises(ValueError, match="must not alias"):
        ops.roftv_slices(x, x, 0.05, 0.005, 3, False)
    with pytest.raises(ValueError, match="tolerance must be a finite number"):
        ops.pdtv_slices(x, out, 1.0, 0.005, 0.1, 1.0, 3, 0, 0, False, tolerance=-1.0)
    with pytest.raises(ValueError, match="a stack of slices"):
        ops.pdtv_slices(x[0].contiguous(), out[0].contiguous(), 1.0, 0.005, 0.1, 1.0, 3, 0, 0, False)
    lib = _lib.lib()
    nvox = 3 * 9 * 59
    arr = (nvox * 4 + 255) // 256 * 256 + ops.ARRAY_SKEW
    assert lib.tomo_roftv_slices_scratch_bytes(59, 9, 3) == arr
    assert lib.tomo_pdtv_slices_scratch_bytes(59, 9, 3, 0) == 6 * arr
    assert lib.tomo_pdtv_slices_scratch_bytes(59, 9, 3, 1) == 2 * arr + 4 * ((nvox * 2 + 255) // 256 * 256 + ops.ARRAY_SKEW)
    # PD_TV in place: the result is copied back
    kw = S.pd_kwargs(4)
    want = host(pd(x, slicewise=True, **kw))
    y = x.clone()
    same_bits(host(pd(y, slicewise=True, out=y, **kw)), want, "in place")


# ------------------------------------------------------------------------------------------------ tolerance
def _tolerance_case(name, check, d_margin):
    """`check(got, want, what)` compares with the oracle; `d_margin(d)`: how far the reported relative change may lie from
    the oracle's"""
    from tomobar_amd.regularisersCuPy import last_prox
    method, kw, _ = S.TOL_CASES[name]
    fn = pd if method == "PD_TV" else rof
    full = dict(S.pd_kwargs(S.TOL_ITERATIONS) if method == "PD_TV" else S.rof_kwargs(S.TOL_ITERATIONS), **kw)
    tol, stop, d_stop, never = S.tol_plan(name)
    x = dev(S.tol_input())
    got = host(fn(x, slicewise=True, tolerance=tol, **full))
    done, change = last_prox()
    print(f"{name}: tol {tol:.4e}, stopped after {done} (oracle: {stop}), d {change:.6e} (oracle: {d_stop:.6e})")
    assert done == stop
    assert abs(change - d_stop) <= d_margin(d_stop)
    # every slice ran exactly `stop` iterations
    same_bits(got, host(fn(x, slicewise=True, **dict(full, iterations=stop))), "the run of that many iterations")
    same_bits(got, per_slice(fn, x, **dict(full, iterations=stop)), "2D path per slice")
    check(got, S.tol_oracle(name, stop), f"slicewise tol {name}")
    got = host(fn(x, slicewise=True, tolerance=never, **full))
    assert last_prox()[0] == S.TOL_ITERATIONS
    same_bits(got, host(fn(x, slicewise=True, **full)), "a tolerance that is never met")


def _sum_margin(d):
    """sums of 3 x 40 x 40 non-negative doubles in another order"""
    return 3 * 40 * 40 * 2.0 ** -53 * d


@pytest.mark.parametrize("name", [n for n in sorted(S.TOL_CASES) if S.TOL_CASES[n][0] == "PD_TV"])
def test_pd_tv_tolerance_is_one_decision_over_the_whole_stack(name, pd_arith):
    half = bool(S.TOL_CASES[name][1].get("half_precision", False))
    # relaxed float32 arithmetic is held to 1e-5 of the oracle, which moves d by at most about 2e-5 (tests/_tolerance_cases.py)
    _tolerance_case(name, lambda got, want, what: pd_arith.check(got, want, half=half, what=what),
                    _sum_margin if (half or pd_arith.exact) else (lambda d: 4e-5))
    if not (half or pd_arith.exact):
        # the run that stopped equals the run of that many iterations bit for bit (_tolerance_case): that one, element for element
        full = dict(S.pd_kwargs(S.tol_plan(name)[1]), **S.TOL_CASES[name][1])
        _elementwise(pd_arith, host(pd(dev(S.tol_input()), slicewise=True, **full)), S.tol_input(), full, f"slicewise tol {name}")


@pytest.mark.parametrize("name", [n for n in sorted(S.TOL_CASES) if S.TOL_CASES[n][0] == "ROF_TV"])
def test_rof_tv_tolerance_is_one_decision_over_the_whole_stack(name):
    _tolerance_case(name, same_bits, _sum_margin)


# ------------------------------------------------------------------------------------------------ drivers
NZ, NN, NA = 4, 16, 12
ANGLES = np.linspace(0, np.pi, NA, endpoint=False)
DRIVER_REGS = {
    "pd": dict(method="PD_TV", regul_param=0.002, iterations=7, PD_LipschitzConstant=8.0),
    "pd_half": dict(method="PD_TV", regul_param=0.002, iterations=7, PD_LipschitzConstant=8.0, half_precision=True),
    "rof": dict(method="ROF_TV", regul_param=0.002, iterations=7, time_marching_step=0.002),
}


def _rt():
    from tomobar_amd.methodsIR_CuPy import RecToolsIRCuPy
    return RecToolsIRCuPy(NN, 0, NZ, 0.0, ANGLES, NN, 0, 2)


def _data():
    sino = torch.from_numpy(np.random.default_rng(11).random((NZ, NA, NN)).astype(np.float32)).cuda()
    return {"projection_data": sino, "data_axes_labels_order": ["detY", "angles", "detX"]}


def _run_both_ways(driver, reg, monkeypatch):
    """(the driver with slicewise=True, the same driver whose prox_regul is the per-slice loop of today's 2D calls)"""
    import tomobar_amd.methodsIR_CuPy as IR
    algo = {"iterations": 2}
    if driver != "OSEM":
        algo["lipschitz_const"] = 3000.0
    if driver == "ADMM":
        algo["ADMM_rho_const"] = 2.0
    got = host(getattr(_rt(), driver)(_data(), dict(algo), dict(reg, slicewise=True)))
    real, seen = IR.prox_regul, []

    def by_hand(self, X, r, out=None):
        assert r.get("slicewise") is True, "the key did not reach the proximal step"
        seen.append(r["regul_param"])
        plain = {k: v for k, v in r.items() if k != "slicewise"}
        res = torch.empty_like(X) if out is None else out
        for k in range(X.shape[0]):
            real(self, X[k].contiguous(), plain, out=res[k])
        return res

    monkeypatch.setattr(IR, "prox_regul", by_hand)
    hand = host(getattr(_rt(), driver)(_data(), dict(algo), dict(reg, slicewise=True)))
    monkeypatch.setattr(IR, "prox_regul", real)
    rho = 2.0 if driver == "ADMM" else 1.0
    assert len(seen) >= 2 and seen == [reg["regul_param"] / rho] * len(seen)
    coupled = host(getattr(_rt(), driver)(_data(), dict(algo), dict(reg)))
    return got, hand, coupled


@pytest.mark.parametrize("reg", sorted(DRIVER_REGS))
@pytest.mark.parametrize("driver", ["FISTA", "ADMM", "OSEM"])
def test_drivers_equal_the_per_slice_loop(driver, reg, monkeypatch):
    got, hand, coupled = _run_both_ways(driver, DRIVER_REGS[reg], monkeypatch)
    same_bits(got, hand, f"{driver} {reg}")
    assert np.all(np.isfinite(got)) and not np.array_equal(got, coupled)


def test_fista_with_wavelets_equals_the_per_slice_loop(monkeypatch):
    reg = dict(DRIVER_REGS["pd"], method="PD_TV_WAVELETS", regul_param2=0.004)
    got, hand, coupled = _run_both_ways("FISTA", reg, monkeypatch)
    same_bits(got, hand, "FISTA PD_TV_WAVELETS")
    assert np.all(np.isfinite(got)) and not np.array_equal(got, coupled)
