"""NDF without a GPU: properties of the numpy restatement (tests/_ndf_oracle.py; the algorithm is the specification,
docs/kernels/ndf.md) and the host surface of the feature -- dictionary defaults, the refusals, the C-ABI's argument checks,
scratch size and symbol set (the library loads and validates without a device)."""
import ctypes as C
import types

import numpy as np
import pytest

import _ndf_oracle as N

SHAPE_3D, SHAPE_2D = (7, 13, 37), (13, 37)
COUNTS = (1, 2, 25, 40)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("pname", sorted(N.PARAMS))
@pytest.mark.parametrize("shape", [SHAPE_3D, SHAPE_2D])
def test_float32_against_float64(shape, pname):
    """the float32 arithmetic the kernel reproduces holds the project's parity bar against the same algorithm in double"""
    f32, f64 = N.cached(shape, pname, COUNTS), N.cached(shape, pname, COUNTS, "float64")
    for n in COUNTS:
        r = N.rel_l2(f32[n], f64[n])
        print(f"NDF {pname} {shape} after {n}: float32 vs float64 rel-L2 = {r:.2e}")
        assert f32[n].dtype == np.float32 and f64[n].dtype == np.float64
        assert r <= 1e-5, (shape, pname, n, r)


@pytest.mark.parametrize("pname", sorted(N.PARAMS))
@pytest.mark.parametrize("shape", [SHAPE_3D, SHAPE_2D])
def test_both_branches_of_every_penalty_are_exercised(shape, pname):
    """a condition on the INPUTS of the GPU tests: at the last iteration between 10 % and 90 % of the forward differences
    exceed sigma"""
    for n in COUNTS:
        stats = {}
        N.ndf(N.phantom(shape), iterations=n, stats=stats, **N.PARAMS[pname])
        print(f"NDF {pname} {shape} iteration {n}: |forward difference| > sigma on {stats['above']:.3f}")
        assert 0.10 <= stats["above"] <= 0.90, (pname, shape, n, stats)


def test_z_replicated_volume_equals_the_2d_run():
    """the z terms come last and are +0 on a volume constant along z: plane for plane the bits of the 2D run"""
    plane = N.phantom(SHAPE_2D)
    vol = np.ascontiguousarray(np.broadcast_to(plane, (5,) + SHAPE_2D))
    for pname, params in N.PARAMS.items():
        want = N.ndf(plane, iterations=25, **params)
        got = N.ndf(vol, iterations=25, **params)
        for z in range(vol.shape[0]):
            assert np.array_equal(_bits(got[z]), _bits(want)), (pname, z)


def test_tukey_keeps_a_noiseless_step_and_huber_does_not():
    step = np.zeros((6, 8, 12), np.float32)
    step[..., 6:] = 1.0
    kept = N.ndf(step, "Tukey", 1.0, 0.1, 0.05, iterations=25)
    assert np.array_equal(_bits(kept), _bits(step)), "Tukey with sigma below the step height must not touch it"
    moved = N.ndf(step, "Huber", 1.0, 0.1, 0.05, iterations=25)
    assert not np.array_equal(moved, step)
    assert np.abs(moved - step).max() > 0.05


@pytest.mark.parametrize("shape", [(5, 6, 7), (6, 7)])
def test_constant_input_is_a_fixed_point(shape):
    f = np.full(shape, np.float32(37.25), np.float32)
    for pname, params in N.PARAMS.items():
        out = N.ndf(f, iterations=25, **params)
        assert np.array_equal(_bits(out), _bits(f)), pname


def test_zero_iterations_and_a_dimension_of_one():
    f = N.phantom((1, 5, 3))
    out = N.ndf(f, iterations=0, **N.PARAMS["A"])
    assert np.array_equal(_bits(out), _bits(f))
    for shape in [(1, 5, 3), (5, 1, 3), (5, 3, 1), (1, 37), (37, 1)]:
        assert np.all(np.isfinite(N.ndf(N.phantom(shape), iterations=7, **N.PARAMS["B"]))), shape
    # an axis of extent 1 contributes +0 twice: a [1][y][x] volume is the 2D run
    plane = N.phantom(SHAPE_2D)
    for pname, params in N.PARAMS.items():
        assert np.array_equal(_bits(N.ndf(plane[None], iterations=7, **params)[0]), _bits(N.ndf(plane, iterations=7, **params)))


@pytest.mark.parametrize("world", [2, 3])
def test_stitched_slabs_equal_the_whole_volume(world):
    """ndf_step_slab on slabs with one ghost plane either side, exchanged after every iteration"""
    f = N.phantom(SHAPE_3D)
    for pname, params in N.PARAMS.items():
        want = N.cached(SHAPE_3D, pname, COUNTS)[2]
        assert np.array_equal(_bits(N.ndf_by_slabs(f, params, 2, world)), _bits(want)), (pname, world)
    want = N.cached(SHAPE_3D, "B", COUNTS)[25]
    assert np.array_equal(_bits(N.ndf_by_slabs(f, N.PARAMS["B"], 25, world)), _bits(want))


def test_slab_step_writes_only_the_range_it_is_given():
    f = N.phantom((6, 5, 9))
    out = np.full_like(f, np.nan)
    p = N.PARAMS["C"]
    N.ndf_step_slab(f, f, out, 9, 5, 4, 1, 1, p["lam"], p["sigma"], p["tau"], 2, zr=(1, 3))
    assert np.all(np.isnan(out[:2])) and np.all(np.isnan(out[4:]))
    want = N.ndf(f, iterations=1, **p)
    assert np.array_equal(_bits(out[2:4]), _bits(want[2:4]))


@pytest.mark.parametrize("penalty", N.PENALTIES)
def test_backward_flux_is_the_neighbours_forward_flux_with_the_sign_turned(penalty):
    """what the kernel relies on (csrc/ndf_zmarch.inl): g(b - a) has the bits of -g(a - b) -- the penalties are odd and every
    operation in them rounds symmetrically -- except that a zero difference, and Tukey's rejected range, give +0 both ways"""
    rng = np.random.default_rng(7)
    a = (rng.standard_normal(200000) * 3.0).astype(np.float32)
    b = (rng.standard_normal(200000) * 3.0).astype(np.float32)
    b[::17] = a[::17]                                  # zero differences
    a[1::1001] *= np.float32(1e-30)                    # differences whose flux underflows
    b[1::1001] = a[1::1001] * np.float32(1.5)
    for sigma in (np.float32(0.5), np.float32(2.0), np.float32(1e6)):
        t = a - b
        g = N.flux(t, sigma, penalty)
        rejected = (np.abs(t) > sigma) if penalty == "Tukey" else np.zeros(t.shape, bool)
        gn = np.where((t == 0) | rejected, np.float32(0.0), -g)
        assert np.array_equal(_bits(N.flux(b - a, sigma, penalty)), _bits(gn)), (penalty, sigma)


def test_the_tolerance_cases_satisfy_their_rule():
    for slab in (False, True):
        tol, stop, d_stop, seq = N.tolerance_plan(slab)
        print(f"NDF tolerance case (slab={slab}): sequence {['%.3e' % v for v in seq]}, tol {tol:.4e}, stops after {stop}")
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
    r = _dicts({"method": "NDF"})
    assert r["NDF_penalty"] == "Huber" and r["edge_threshold"] == 0.01
    r = _dicts({"method": "NDF", "NDF_penalty": "Tukey", "edge_threshold": 0.3})
    assert r["NDF_penalty"] == "Tukey" and r["edge_threshold"] == 0.3
    for bad in ("huber", "TV", None, 1):
        with pytest.raises(ValueError, match="NDF_penalty"):
            _dicts({"method": "NDF", "NDF_penalty": bad})
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="edge_threshold"):
            _dicts({"method": "NDF", "edge_threshold": bad})
    # dictionaries of the other methods come out as before
    for method in ("PD_TV", "ROF_TV", "TGV", None):
        r = _dicts({"method": method, "regul_param": 0.1})
        assert "NDF_penalty" not in r and "edge_threshold" not in r
    assert set(_dicts({"method": "NDF"})) - set(_dicts({"method": "ROF_TV"})) == {"NDF_penalty", "edge_threshold"}


def test_refusals_half_precision_unknown_method_unknown_penalty():
    import torch
    from tomobar_amd.regularisersCuPy import NDF_cupy, check_prox_available, prox_regul, reserve_prox_scratch
    reg = {"method": "NDF", "regul_param": 1.0, "iterations": 3, "time_marching_step": 0.05, "edge_threshold": 2.0}
    X = torch.zeros((4, 5, 6), dtype=torch.float32)
    with pytest.raises(ValueError, match="half_precision"):
        prox_regul(_self(), X, dict(reg, half_precision=True))
    with pytest.raises(ValueError, match="half_precision"):
        reserve_prox_scratch(_self(), (4, 5, 6), dict(reg, half_precision=True))
    # NDF runs in z-slab mode: no refusal there
    check_prox_available(_self(slab=object()), (4, 5, 6), reg)
    with pytest.raises(ValueError, match="ROF_TV, PD_TV and TGV"):
        prox_regul(_self(), X, dict(reg, method="NLTV"))
    with pytest.raises(ValueError, match="NDF penalty"):
        NDF_cupy(X, 1.0, 2.0, 3, 0.05, "Welsch")
    with pytest.raises(ValueError, match="NDF penalty"):
        prox_regul(_self(), X, dict(reg, NDF_penalty="Welsch"))
    import tomobar_amd
    assert tomobar_amd.NDF_cupy is NDF_cupy


def test_slab_state_bookkeeping():
    """NdfSlab on host tensors: one ghost plane where a neighbour exists, the ranges the neighbours wait for, the placed slot"""
    import torch
    from tomobar_amd import slab as S
    data = torch.arange(5 * 2 * 3, dtype=torch.float32).reshape(5, 2, 3)
    st = S.NdfSlab(data, True, True, 0, N.ndf_step_slab)
    assert (st.lo, st.hi) == (1, 1) and st.inp.shape[0] == 7 and torch.equal(st.local(st.inp), data)
    assert st.boundary_ranges() == ([(0, 1), (4, 5)], (1, 4))
    assert st.source(0) is st.inp and st.source(1) is st.U[1] and st.source(2) is st.U[0]
    assert st.send_up(0)[0].data_ptr() == st.inp[5].data_ptr() and st.recv_up(0)[0].data_ptr() == st.inp[6].data_ptr()
    assert st.send_down(3)[0].data_ptr() == st.U[1][1].data_ptr() and st.recv_down(3)[0].data_ptr() == st.U[1][0].data_ptr()
    st = S.NdfSlab(data[:1], True, True, 0, N.ndf_step_slab)
    assert st.boundary_ranges() == ([(0, 1)], (1, 1))
    st = S.NdfSlab(data, False, True, 0, N.ndf_step_slab)
    assert (st.lo, st.hi) == (0, 1) and st.boundary_ranges() == ([(4, 5)], (0, 4)) and st.send_down(0) == []
    assert len({S.PLACED_SLOT_PD, S.PLACED_SLOT_ROF, S.PLACED_SLOT_NDF}) == 3 and S.PLACED_SLOT_NDF == 2
    # one rank, host tensors, the oracle's step: the driver is the whole-volume run
    f = N.phantom((6, 5, 9))
    p = N.PARAMS["B"]
    got = S.ndf_slab(torch.from_numpy(f), S.SlabComm(0, 1), p["lam"], p["sigma"], 7, p["tau"], p["penalty"], step_fn=N.ndf_step_slab)
    assert np.array_equal(_bits(got.numpy()), _bits(N.ndf(f, iterations=7, **p)))
    got = S.ndf_slab(torch.from_numpy(f), S.SlabComm(0, 1), p["lam"], p["sigma"], 0, p["tau"], p["penalty"], step_fn=N.ndf_step_slab)
    assert np.array_equal(_bits(got.numpy()), _bits(f))


def _lib():
    from tomobar_amd import _lib
    return _lib.lib()


def test_abi_symbols_and_version():
    from tomobar_amd import _lib
    lib = _lib.lib()
    for name in ("tomo_ndf", "tomo_ndf_scratch_bytes", "tomo_ndf_iter_slab_range"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 10 and lib.tomo_abi_version() == 10
    assert _lib.NDF_PENALTY == {"Huber": 0, "PM": 1, "Tukey": 2}
    with _lib.use_flavour("dev") as dev:
        assert hasattr(dev, "tomo_ndf") and dev.tomo_abi_version() == 10


def test_scratch_bytes():
    lib = _lib()
    from tomobar_amd import ops
    skew = ops.ARRAY_SKEW
    for dx, dy, dz in [(37, 13, 7), (64, 64, 64), (1, 1, 1), (200, 150, 40)]:
        arr3 = (dx * dy * dz * 4 + 255) // 256 * 256
        arr2 = (dx * dy * 4 + 255) // 256 * 256
        assert lib.tomo_ndf_scratch_bytes(dx, dy, dz, 3) == arr3 + skew      # the one ping-pong partner of the output
        assert lib.tomo_ndf_scratch_bytes(dx, dy, dz, 2) == arr2 + skew      # dz is ignored in 2D


def test_invalid_arguments_are_refused_before_the_device_is_touched():
    from tomobar_amd import _lib
    lib = _lib.lib()
    a, b, c = C.c_void_p(0x1000), C.c_void_p(0x2000), C.c_void_p(0x3000)   # never dereferenced: every case fails validation

    def call(inp=a, out=b, dx=4, dy=4, dz=4, nd=3, lam=1.0, sigma=2.0, tau=0.05, pen=0, iters=3, tol=0.0):
        return lib.tomo_ndf(0, inp, out, dx, dy, dz, nd, lam, sigma, tau, pen, iters, tol, None, None, None)

    bad = [dict(out=a), dict(inp=None), dict(out=None), dict(nd=1), dict(nd=4), dict(dx=0), dict(dy=0), dict(dz=0), dict(dx=-3),
           dict(lam=0.0), dict(lam=-1.0), dict(sigma=0.0), dict(sigma=-2.0), dict(tau=0.0), dict(tau=-0.1),
           dict(lam=float("nan")), dict(pen=-1), dict(pen=3), dict(iters=-1), dict(tol=-1e-3), dict(tol=float("inf")),
           dict(tol=float("nan")), dict(nd=2, dy=0), dict(dx=1 << 15, dy=1 << 14)]
    for kw in bad:
        assert call(**kw) == _lib.E_INVALID, kw
        with pytest.raises(ValueError):
            _lib.check(call(**kw))

    def slab(inp=a, u_in=b, u_out=c, dx=4, dy=4, nzl=4, lo=1, hi=1, z0=0, z1=4, lam=1.0, sigma=2.0, tau=0.05, pen=0):
        return lib.tomo_ndf_iter_slab_range(0, inp, u_in, u_out, dx, dy, nzl, lo, hi, z0, z1, lam, sigma, tau, pen, None)

    bad = [dict(dx=0), dict(dy=0), dict(nzl=0), dict(lo=2), dict(hi=2), dict(lo=-1), dict(z0=-1), dict(z1=5), dict(z0=3, z1=2),
           dict(lam=0.0), dict(sigma=0.0), dict(tau=0.0), dict(pen=3), dict(inp=None), dict(u_in=None), dict(u_out=None),
           dict(u_out=b), dict(u_out=a), dict(dx=1 << 15, dy=1 << 14)]
    for kw in bad:
        assert slab(**kw) == _lib.E_INVALID, kw
    assert slab(z0=2, z1=2) == _lib.OK     # an empty range is nothing to do, before any device work
