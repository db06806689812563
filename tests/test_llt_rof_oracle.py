"""LLT_ROF without a GPU: properties of the numpy restatement (tests/_llt_rof_oracle.py; the algorithm is the specification,
docs/kernels/llt_rof.md) and the host surface of the feature -- dictionary defaults, the refusals, ADMM's private copy, the
C-ABI's argument checks, scratch size and symbol set (the library loads and validates without a device)."""
import ctypes as C
import types

import numpy as np
import pytest

import _llt_rof_oracle as D

SHAPE_3D, SHAPE_2D = (7, 13, 37), (13, 37)
COUNTS = (1, 2, 25, 40)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("pname", sorted(D.PARAMS))
@pytest.mark.parametrize("shape", [SHAPE_3D, SHAPE_2D])
def test_float32_against_float64(shape, pname):
    """the float32 arithmetic the kernel reproduces holds the project's parity bar against the same algorithm in double.
    Largest values seen: A 2.2e-6, B 1.5e-6, C 1.9e-7 -- larger than the sibling oracles' 1e-7 because E_d is sign-like: a
    second difference at rounding level can take opposite signs in the two precisions."""
    f32, f64 = D.cached(shape, pname, COUNTS), D.cached(shape, pname, COUNTS, "float64")
    for n in COUNTS:
        r = D.rel_l2(f32[n], f64[n])
        print(f"LLT_ROF {pname} {shape} after {n}: float32 vs float64 rel-L2 = {r:.2e}")
        assert f32[n].dtype == np.float32 and f64[n].dtype == np.float64
        assert r <= 1e-5, (shape, pname, n, r)


@pytest.mark.parametrize("pname", sorted(D.PARAMS))
@pytest.mark.parametrize("shape", [SHAPE_3D, SHAPE_2D])
def test_both_terms_act_in_the_first_and_the_40th_iteration(shape, pname):
    """a condition on the INPUTS of the GPU tests: the full run differs from the runs with either weight set to 1e-30 of
    itself, and from the iterate entering iterations 1 and 40 the step with either weight scaled so differs from the full
    step -- a kernel that dropped or mis-weighted one term could not pass"""
    p = D.PARAMS[pname]
    f = D.phantom(shape)
    full = D.cached(shape, pname, COUNTS)[40]
    no_rof = D.llt_rof(f, np.float32(p["lam_rof"]) * np.float32(1e-30), p["lam_llt"], p["tau"], 40)
    no_llt = D.llt_rof(f, p["lam_rof"], np.float32(p["lam_llt"]) * np.float32(1e-30), p["tau"], 40)
    print(f"LLT_ROF {pname} {shape}: rel-L2 of the 40-iteration run to the run without ROF {D.rel_l2(no_rof, full):.2e}, "
          f"without LLT {D.rel_l2(no_llt, full):.2e}")
    assert D.rel_l2(no_rof, full) > 1e-5 and D.rel_l2(no_llt, full) > 1e-5
    its = {0: f}
    its.update(D.llt_rof_many(f, p, (39,)))
    l1, l2, tau = np.float32(p["lam_rof"]), np.float32(p["lam_llt"]), np.float32(p["tau"])
    tiny = np.float32(1e-30)
    for n in (1, 40):
        U = its[n - 1]
        want = D.step(U, f, l1, l2, tau)
        assert not np.array_equal(D.step(U, f, l1 * tiny, l2, tau), want), (pname, n, "the ROF term does nothing")
        assert not np.array_equal(D.step(U, f, l1, l2 * tiny, tau), want), (pname, n, "the LLT term does nothing")


def test_z_replicated_volume_equals_the_2d_run():
    """the z terms come last and are exact zeros on a volume constant along z: plane for plane the bits of the 2D run"""
    plane = D.phantom(SHAPE_2D)
    vol = np.ascontiguousarray(np.broadcast_to(plane, (5,) + SHAPE_2D))
    for pname, params in D.PARAMS.items():
        want = D.llt_rof(plane, iterations=10, **params)
        got = D.llt_rof(vol, iterations=10, **params)
        for z in range(vol.shape[0]):
            assert np.array_equal(_bits(got[z]), _bits(want)), (pname, z)


@pytest.mark.parametrize("shape", [(5, 6, 7), (6, 7)])
def test_constant_input_is_a_fixed_point(shape):
    f = np.full(shape, np.float32(37.25), np.float32)
    for pname, params in D.PARAMS.items():
        out = D.llt_rof(f, iterations=25, **params)
        assert np.array_equal(_bits(out), _bits(f)), pname


def test_the_operator_changes_a_noisy_input():
    f = D.phantom(SHAPE_3D)
    for pname in D.PARAMS:
        for n in COUNTS:
            out = D.cached(SHAPE_3D, pname, COUNTS)[n]
            assert np.all(np.isfinite(out)) and not np.array_equal(out, f), (pname, n)
        assert D.rel_l2(D.cached(SHAPE_3D, pname, COUNTS)[40], f) > D.rel_l2(D.cached(SHAPE_3D, pname, COUNTS)[1], f) > 0.0


def test_one_step_is_bounded_by_the_fluxes():
    """|U' - c| <= tau (4 nd lam_llt + 2 nd lam_rof + |c - f|): the fluxes are bounded by 1 (a little slack for the roundings)"""
    for shape in (SHAPE_3D, SHAPE_2D):
        nd = len(shape)
        for pname, p in D.PARAMS.items():
            f = D.phantom(shape).astype(np.float64)
            U = D.cached(shape, pname, COUNTS)[25].astype(np.float64)
            new = D.step(U, f, p["lam_rof"], p["lam_llt"], p["tau"])
            bound = p["tau"] * (4 * nd * p["lam_llt"] + 2 * nd * p["lam_rof"] + np.abs(U - f))
            assert np.all(np.abs(new - U) <= bound * (1 + 1e-6)), (shape, pname)


def test_terraces_stay_finite_and_reach_the_zero_paths():
    """exact zeros and ties: 0 / (0 + eps) and 0 / sqrt(eps) give exact zeros, no masked branch"""
    from _edge_shapes import terraces
    stats = {}
    out = D.llt_rof(terraces((20, 24, 70)), iterations=3, stats=stats, **D.PARAMS["A"])
    print(f"LLT_ROF terraces (20, 24, 70): s == 0 on {stats['s_zero', 1]:.3f} / {stats['s_zero', 3]:.4f} of the voxels entering "
          f"iterations 1 / 3, |h1| < 1e-6 on {stats['h1_tiny', 1]:.3f}")
    assert np.all(np.isfinite(out))
    assert stats["s_zero", 1] >= 0.25 and stats["h1_tiny", 1] >= 0.25


def test_zero_iterations_and_a_dimension_of_one():
    f = D.phantom((1, 5, 3))
    out = D.llt_rof(f, iterations=0, **D.PARAMS["A"])
    assert np.array_equal(_bits(out), _bits(f))
    for shape in [(1, 5, 3), (5, 1, 3), (5, 3, 1), (1, 37), (37, 1), (2, 2, 2)]:
        assert np.all(np.isfinite(D.llt_rof(D.phantom(shape), iterations=7, **D.PARAMS["B"]))), shape
    # an axis of extent 1 contributes exact zeros: a [1][y][x] volume is the 2D run
    plane = D.phantom(SHAPE_2D)
    for pname, params in D.PARAMS.items():
        assert np.array_equal(_bits(D.llt_rof(plane[None], iterations=7, **params)[0]), _bits(D.llt_rof(plane, iterations=7, **params)))


@pytest.mark.parametrize("world", [2, 3])
def test_stitched_slabs_equal_the_whole_volume(world):
    """llt_rof_step_slab on slabs with two ghost planes either side, exchanged after every iteration"""
    f = D.phantom(SHAPE_3D)
    for pname, params in D.PARAMS.items():
        want = D.cached(SHAPE_3D, pname, COUNTS)[2]
        assert np.array_equal(_bits(D.llt_rof_by_slabs(f, params, 2, world)), _bits(want)), (pname, world)
    want = D.cached(SHAPE_3D, "B", COUNTS)[25]
    assert np.array_equal(_bits(D.llt_rof_by_slabs(f, D.PARAMS["B"], 25, world)), _bits(want))


def test_stitched_slabs_with_a_slab_of_exactly_two_planes():
    f = D.phantom(SHAPE_3D)
    want = D.cached(SHAPE_3D, "A", COUNTS)[2]
    for bounds in ([(0, 2), (2, 7)], [(0, 5), (5, 7)], [(0, 3), (3, 5), (5, 7)], [(0, 2), (2, 4), (4, 7)]):
        got = D.llt_rof_by_slabs(f, D.PARAMS["A"], 2, len(bounds), bounds)
        assert np.array_equal(_bits(got), _bits(want)), bounds


def test_two_ghost_planes_are_needed():
    """slabs (0,2),(2,5),(5,9) of a (9,7,11) volume: two ghost planes reproduce the whole volume, one does not (the stencil
    has radius 2)"""
    f = D.phantom((9, 7, 11))
    bounds = [(0, 2), (2, 5), (5, 9)]
    for pname, params in D.PARAMS.items():
        want = D.llt_rof(f, iterations=6, **params)
        assert np.array_equal(_bits(D.llt_rof_by_slabs(f, params, 6, 3, bounds)), _bits(want)), pname
        assert not np.array_equal(_bits(D.llt_rof_by_slabs(f, params, 6, 3, bounds, ghost=1)), _bits(want)), pname


def test_slab_step_writes_only_the_range_it_is_given():
    f = D.phantom((9, 5, 9))
    out = np.full_like(f, np.nan)
    p = D.PARAMS["C"]
    D.llt_rof_step_slab(f, f, out, 9, 5, 5, 2, 2, p["lam_rof"], p["lam_llt"], p["tau"], zr=(1, 3))
    assert np.all(np.isnan(out[:3])) and np.all(np.isnan(out[5:]))
    want = D.llt_rof(f, iterations=1, **p)
    assert np.array_equal(_bits(out[3:5]), _bits(want[3:5]))


def test_the_tolerance_cases_satisfy_their_rule():
    for slab in (False, True):
        tol, stop, d_stop, seq = D.tolerance_plan(slab)
        print(f"LLT_ROF tolerance case (slab={slab}): sequence {['%.3e' % v for v in seq]}, tol {tol:.4e}, stops after {stop}")
        assert stop == 24 and d_stop < tol < seq[2]


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
    r = _dicts({"method": "LLT_ROF"})
    assert r["regul_param2"] == 0.001 and "NDF_penalty" not in r and "edge_threshold" not in r
    assert _dicts({"method": "LLT_ROF", "regul_param2": 0.3})["regul_param2"] == 0.3
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="regul_param2"):
            _dicts({"method": "LLT_ROF", "regul_param2": bad})
    # dictionaries of the other methods come out as before
    for method in ("PD_TV", "ROF_TV", "TGV", "NDF", "Diff4th", None):
        r = _dicts({"method": method, "regul_param": 0.1})
        assert "regul_param2" not in r
        r = _dicts({"method": method, "regul_param": 0.1, "regul_param2": -1.0})   # not this method's key: not checked
        assert r["regul_param2"] == -1.0
    assert set(_dicts({"method": "LLT_ROF"})) - set(_dicts({"method": "ROF_TV"})) == {"regul_param2"}
    assert set(_dicts({"method": "Diff4th"})) - set(_dicts({"method": "ROF_TV"})) == {"edge_threshold"}
    assert set(_dicts({"method": "NDF"})) - set(_dicts({"method": "ROF_TV"})) == {"NDF_penalty", "edge_threshold"}


def test_admm_divides_both_weights_on_its_own_copy():
    """ADMM hands prox_regul regul_param / rho AND regul_param2 / rho (both multiply the regulariser) and leaves the
    caller's dictionary as it was.  The driver's set-up is replaced by a stub and the loop is left at its first allocation:
    what is under test is the dictionary ADMM builds before it, read from ADMM's frame."""
    import traceback
    import torch
    from tomobar_amd.methodsIR_CuPy import RecToolsIRCuPy

    class Stop(Exception):
        pass

    def init(_data_, _algorithm_, _regularisation_, name):
        assert name == "ADMM"
        algo = {"nonnegativity": False, "ADMM_rho_const": 4.0, "ADMM_relax_par": 1.6, "lipschitz_const": 1.0}
        return ({"projection_data": None}, algo, _regularisation_, torch.zeros((2, 3, 3)), None, False)

    def new_vol(*a):
        raise Stop

    me = types.SimpleNamespace(Atools=None, data_fidelity="LS", _new_vol=new_vol)
    setattr(me, "_RecToolsIRCuPy__common_initialisation", init)

    def local_copy(reg):
        with pytest.raises(Stop) as ei:
            RecToolsIRCuPy.ADMM(me, {}, {}, reg)
        return next(f.f_locals["r_local"] for f, _ in traceback.walk_tb(ei.value.__traceback__) if f.f_code.co_name == "ADMM")

    reg = {"method": "LLT_ROF", "regul_param": 0.5, "regul_param2": 0.25, "iterations": 3, "time_marching_step": 0.01}
    keep = dict(reg)
    local = local_copy(reg)
    assert reg == keep and local is not reg
    assert local["regul_param"] == 0.125 and local["regul_param2"] == 0.0625
    assert {k: v for k, v in local.items() if not k.startswith("regul_param")} == {k: v for k, v in keep.items() if not k.startswith("regul_param")}
    # a second weight a caller left in another method's dictionary is not touched
    local = local_copy(dict(reg, method="ROF_TV"))
    assert local["regul_param"] == 0.125 and local["regul_param2"] == 0.25


def test_refusals_half_precision_and_unknown_method():
    import torch
    from tomobar_amd.regularisersCuPy import LLT_ROF_cupy, check_prox_available, prox_regul, reserve_prox_scratch
    reg = {"method": "LLT_ROF", "regul_param": 0.3, "regul_param2": 0.1, "iterations": 3, "time_marching_step": 0.005}
    X = torch.zeros((4, 5, 6), dtype=torch.float32)
    with pytest.raises(ValueError, match="LLT_ROF does not support half_precision"):
        prox_regul(_self(), X, dict(reg, half_precision=True))
    with pytest.raises(ValueError, match="half_precision"):
        reserve_prox_scratch(_self(), (4, 5, 6), dict(reg, half_precision=True))
    with pytest.raises(ValueError, match="half_precision"):
        check_prox_available(_self(), (4, 5, 6), dict(reg, half_precision=True))
    # LLT_ROF runs in z-slab mode: no refusal there
    check_prox_available(_self(slab=object()), (4, 5, 6), reg)
    with pytest.raises(ValueError, match="ROF_TV, PD_TV and TGV.*Diff4th(?s:.*)LLT_ROF"):
        prox_regul(_self(), X, dict(reg, method="NLTV"))
    import tomobar_amd
    assert tomobar_amd.LLT_ROF_cupy is LLT_ROF_cupy
    import inspect
    sig = inspect.signature(LLT_ROF_cupy)
    assert list(sig.parameters) == ["data", "regularisation_parameterROF", "regularisation_parameterLLT", "iterations",
                                    "time_marching_parameter", "gpu_device", "out", "tolerance"]
    assert [p.default for p in list(sig.parameters.values())[1:]] == [1e-05, 1e-05, 1000, 0.001, 0, None, 0.0]


def test_slab_state_bookkeeping():
    """LltRofSlab on host tensors: two ghost planes where a neighbour exists, the ranges the neighbours wait for, the slot"""
    import torch
    from tomobar_amd import slab as S
    data = torch.arange(7 * 2 * 3, dtype=torch.float32).reshape(7, 2, 3)
    st = S.LltRofSlab(data, True, True, D.llt_rof_step_slab)
    assert (st.lo, st.hi) == (2, 2) and st.inp.shape[0] == 11 and torch.equal(st.local(st.inp), data)
    assert st.boundary_ranges() == ([(0, 2), (5, 7)], (2, 5))
    assert st.source(0) is st.inp and st.source(1) is st.U[1] and st.source(2) is st.U[0]
    (su,), (ru,), (sd,), (rd,) = st.send_up(0), st.recv_up(0), st.send_down(3), st.recv_down(3)
    assert su.shape[0] == ru.shape[0] == sd.shape[0] == rd.shape[0] == 2 and all(t.is_contiguous() for t in (su, ru, sd, rd))
    assert su.data_ptr() == st.inp[7].data_ptr() and ru.data_ptr() == st.inp[9].data_ptr()
    assert sd.data_ptr() == st.U[1][2].data_ptr() and rd.data_ptr() == st.U[1][0].data_ptr()
    st = S.LltRofSlab(data[:2], True, True, D.llt_rof_step_slab)       # a slab of exactly two planes: all of it is boundary
    assert st.boundary_ranges() == ([(0, 2)], (2, 2))
    assert st.send_up(0)[0].data_ptr() == st.send_down(0)[0].data_ptr() == st.inp[2].data_ptr()
    st = S.LltRofSlab(data[:3], True, True, D.llt_rof_step_slab)
    assert st.boundary_ranges() == ([(0, 2), (2, 3)], (2, 2))
    st = S.LltRofSlab(data, False, True, D.llt_rof_step_slab)
    assert (st.lo, st.hi) == (0, 2) and st.boundary_ranges() == ([(5, 7)], (0, 5)) and st.send_down(0) == [] and st.recv_down(0) == []
    assert len({S.PLACED_SLOT_PD, S.PLACED_SLOT_ROF, S.PLACED_SLOT_NDF, S.PLACED_SLOT_DIFF4TH, S.PLACED_SLOT_LLT_ROF}) == 5 and S.PLACED_SLOT_LLT_ROF == 4


def test_one_rank_slab_driver_is_the_whole_volume_run():
    import torch
    from tomobar_amd import slab as S
    f = D.phantom((6, 5, 9))
    p = D.PARAMS["B"]
    got = S.llt_rof_slab(torch.from_numpy(f), S.SlabComm(0, 1), p["lam_rof"], p["lam_llt"], 7, p["tau"], step_fn=D.llt_rof_step_slab)
    assert np.array_equal(_bits(got.numpy()), _bits(D.llt_rof(f, iterations=7, **p)))
    got = S.llt_rof_slab(torch.from_numpy(f), S.SlabComm(0, 1), p["lam_rof"], p["lam_llt"], 0, p["tau"], step_fn=D.llt_rof_step_slab)
    assert np.array_equal(_bits(got.numpy()), _bits(f))
    out = torch.full((6, 5, 9), float("nan"))
    info = {}
    assert S.llt_rof_slab(torch.from_numpy(f), S.SlabComm(0, 1), p["lam_rof"], p["lam_llt"], 2, p["tau"], step_fn=D.llt_rof_step_slab,
                          out=out, info=info) is out
    assert np.array_equal(_bits(out.numpy()), _bits(D.llt_rof(f, iterations=2, **p))) and info["iterations_done"] == 2


def _lib():
    from tomobar_amd import _lib
    return _lib.lib()


def test_abi_symbols():
    from tomobar_amd import _lib
    lib = _lib.lib()
    names = ("tomo_llt_rof", "tomo_llt_rof_scratch_bytes", "tomo_llt_rof_iter_slab_range")
    for name in names:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.tomo_abi_version() == 10 == _lib.ABI_VERSION
    with _lib.use_flavour("dev") as dev:
        for name in names:
            assert hasattr(dev, name), name
        assert dev.tomo_abi_version() == 10


def test_scratch_bytes():
    lib = _lib()
    from tomobar_amd import ops
    skew = ops.ARRAY_SKEW
    for dx, dy, dz in [(37, 13, 7), (64, 64, 64), (1, 1, 1), (200, 150, 40)]:
        arr3 = (dx * dy * dz * 4 + 255) // 256 * 256
        arr2 = (dx * dy * 4 + 255) // 256 * 256
        assert lib.tomo_llt_rof_scratch_bytes(dx, dy, dz, 3) == arr3 + skew      # the one ping-pong partner of the output
        assert lib.tomo_llt_rof_scratch_bytes(dx, dy, dz, 2) == arr2 + skew      # dz is ignored in 2D


def test_invalid_arguments_are_refused_before_the_device_is_touched():
    from tomobar_amd import _lib
    lib = _lib.lib()
    a, b, c = C.c_void_p(0x1000), C.c_void_p(0x2000), C.c_void_p(0x3000)   # never dereferenced: every case fails validation

    def call(inp=a, out=b, dx=4, dy=4, dz=4, nd=3, lam=0.3, lam2=0.1, tau=0.005, iters=3, tol=0.0):
        return lib.tomo_llt_rof(0, inp, out, dx, dy, dz, nd, lam, lam2, tau, iters, tol, None, None, None)

    bad = [dict(out=a), dict(inp=None), dict(out=None), dict(nd=1), dict(nd=4), dict(dx=0), dict(dy=0), dict(dz=0), dict(dx=-3),
           dict(lam=0.0), dict(lam=-1.0), dict(lam2=0.0), dict(lam2=-2.0), dict(tau=0.0), dict(tau=-0.1),
           dict(lam=float("nan")), dict(lam2=float("nan")), dict(iters=-1), dict(tol=-1e-3), dict(tol=float("inf")),
           dict(tol=float("nan")), dict(nd=2, dy=0), dict(dx=1 << 15, dy=1 << 14)]
    for kw in bad:
        assert call(**kw) == _lib.E_INVALID, kw
        with pytest.raises(ValueError):
            _lib.check(call(**kw))

    def slab(inp=a, u_in=b, u_out=c, dx=4, dy=4, nzl=4, lo=2, hi=2, z0=0, z1=4, lam=0.3, lam2=0.1, tau=0.005):
        return lib.tomo_llt_rof_iter_slab_range(0, inp, u_in, u_out, dx, dy, nzl, lo, hi, z0, z1, lam, lam2, tau, None)

    bad = [dict(dx=0), dict(dy=0), dict(nzl=0), dict(lo=1), dict(hi=1), dict(lo=3), dict(lo=-1), dict(z0=-1), dict(z1=5),
           dict(z0=3, z1=2), dict(lam=0.0), dict(lam2=0.0), dict(tau=0.0), dict(inp=None), dict(u_in=None), dict(u_out=None),
           dict(u_out=b), dict(u_out=a), dict(dx=1 << 15, dy=1 << 14)]
    for kw in bad:
        assert slab(**kw) == _lib.E_INVALID, kw
    assert slab(z0=2, z1=2) == _lib.OK     # an empty range is nothing to do, before any device work
