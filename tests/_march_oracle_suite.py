"""TEST INFRASTRUCTURE: NDF, Diff4th and LLT_ROF without a GPU, the tests the three share, written once;
tests/test_ndf_oracle.py, tests/test_diff4th_oracle.py and tests/test_llt_rof_oracle.py each collect `suite(<operator>)` next to
the tests that are the operator's own.  Properties of the numpy
restatements that hold for every explicit time march (tests/_march_oracle.py runs each formula), the z-slab state and driver
on host tensors, and the C-ABI's scratch size and argument checks (the library loads and validates without a device)."""
import ctypes as C
import types

import numpy as np
import pytest

from _march_gpu import OPS
from _tgv_oracle import phantom

SHAPE_3D, SHAPE_2D = (7, 13, 37), (13, 37)
COUNTS = (1, 2, 25, 40)

# what differs between the operators, as data
Z_REPLICATED_ITERATIONS = {"NDF": 25, "Diff4th": 25, "LLT_ROF": 10}
THIN_SHAPES = [(1, 5, 3), (5, 1, 3), (5, 3, 1), (1, 37), (37, 1)]
FINITE_SHAPES = {"NDF": THIN_SHAPES, "Diff4th": THIN_SHAPES + [(2, 2, 2)], "LLT_ROF": THIN_SHAPES + [(2, 2, 2)]}
# the slab step on a [g + nzl + g][5][9] array: NDF's penalty goes in as its TOMO_NDF_* number (2 = Tukey, set C)
SLAB_STEP = {"NDF": dict(nzl=4, extra=(2,)), "Diff4th": dict(nzl=5, extra=()), "LLT_ROF": dict(nzl=5, extra=())}
# the C entry points: `args` are the parameters after nd (after hi, z0, z1 for the slab entry) with their valid values,
# `bad` / `bad_slab` the changes each entry must refuse
a, b, c = C.c_void_p(0x1000), C.c_void_p(0x2000), C.c_void_p(0x3000)   # never dereferenced: every case fails validation
ABI = {
    "NDF": types.SimpleNamespace(
        args=dict(lam=1.0, sigma=2.0, tau=0.05, pen=0),
        bad=[dict(out=a), dict(inp=None), dict(out=None), dict(nd=1), dict(nd=4), dict(dx=0), dict(dy=0), dict(dz=0), dict(dx=-3),
             dict(lam=0.0), dict(lam=-1.0), dict(sigma=0.0), dict(sigma=-2.0), dict(tau=0.0), dict(tau=-0.1),
             dict(lam=float("nan")), dict(pen=-1), dict(pen=3), dict(iters=-1), dict(tol=-1e-3), dict(tol=float("inf")),
             dict(tol=float("nan")), dict(nd=2, dy=0), dict(dx=1 << 15, dy=1 << 14)],
        bad_slab=[dict(dx=0), dict(dy=0), dict(nzl=0), dict(lo=2), dict(hi=2), dict(lo=-1), dict(z0=-1), dict(z1=5), dict(z0=3, z1=2),
                  dict(lam=0.0), dict(sigma=0.0), dict(tau=0.0), dict(pen=3), dict(inp=None), dict(u_in=None), dict(u_out=None),
                  dict(u_out=b), dict(u_out=a), dict(dx=1 << 15, dy=1 << 14)]),
    "Diff4th": types.SimpleNamespace(
        args=dict(lam=1.0, sigma=2.0, tau=0.005),
        bad=[dict(out=a), dict(inp=None), dict(out=None), dict(nd=1), dict(nd=4), dict(dx=0), dict(dy=0), dict(dz=0), dict(dx=-3),
             dict(lam=0.0), dict(lam=-1.0), dict(sigma=0.0), dict(sigma=-2.0), dict(tau=0.0), dict(tau=-0.1),
             dict(lam=float("nan")), dict(iters=-1), dict(tol=-1e-3), dict(tol=float("inf")),
             dict(tol=float("nan")), dict(nd=2, dy=0), dict(dx=1 << 15, dy=1 << 14)],
        bad_slab=[dict(dx=0), dict(dy=0), dict(nzl=0), dict(lo=1), dict(hi=1), dict(lo=3), dict(lo=-1), dict(z0=-1), dict(z1=5),
                  dict(z0=3, z1=2), dict(lam=0.0), dict(sigma=0.0), dict(tau=0.0), dict(inp=None), dict(u_in=None), dict(u_out=None),
                  dict(u_out=b), dict(u_out=a), dict(dx=1 << 15, dy=1 << 14)]),
    "LLT_ROF": types.SimpleNamespace(
        args=dict(lam=0.3, lam2=0.1, tau=0.005),
        bad=[dict(out=a), dict(inp=None), dict(out=None), dict(nd=1), dict(nd=4), dict(dx=0), dict(dy=0), dict(dz=0), dict(dx=-3),
             dict(lam=0.0), dict(lam=-1.0), dict(lam2=0.0), dict(lam2=-2.0), dict(tau=0.0), dict(tau=-0.1),
             dict(lam=float("nan")), dict(lam2=float("nan")), dict(iters=-1), dict(tol=-1e-3), dict(tol=float("inf")),
             dict(tol=float("nan")), dict(nd=2, dy=0), dict(dx=1 << 15, dy=1 << 14)],
        bad_slab=[dict(dx=0), dict(dy=0), dict(nzl=0), dict(lo=1), dict(hi=1), dict(lo=3), dict(lo=-1), dict(z0=-1), dict(z1=5),
                  dict(z0=3, z1=2), dict(lam=0.0), dict(lam2=0.0), dict(tau=0.0), dict(inp=None), dict(u_in=None), dict(u_out=None),
                  dict(u_out=b), dict(u_out=a), dict(dx=1 << 15, dy=1 << 14)]),
}


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _lib():
    from tomobar_amd import _lib
    return _lib.lib()


def suite(name):
    """{test name: test function} for the operator `name` of _march_gpu.OPS, to be put into the collecting module's
    namespace"""
    op, D, g = OPS[name], OPS[name].oracle, OPS[name].oracle.GHOST

    # -------------------------------------------------------------------------------------------- the oracle
    def test_z_replicated_volume_equals_the_2d_run():
        """the z terms come last and are exact zeros (NDF: +0) on a volume constant along z: plane for plane the bits of the 2D
        run"""
        n = Z_REPLICATED_ITERATIONS[name]
        plane = phantom(SHAPE_2D)
        vol = np.ascontiguousarray(np.broadcast_to(plane, (5,) + SHAPE_2D))
        for pname, params in D.PARAMS.items():
            want = D.run(plane, iterations=n, **params)
            got = D.run(vol, iterations=n, **params)
            for z in range(vol.shape[0]):
                assert np.array_equal(_bits(got[z]), _bits(want)), (pname, z)

    @pytest.mark.parametrize("shape", [(5, 6, 7), (6, 7)])
    def test_constant_input_is_a_fixed_point(shape):
        f = np.full(shape, np.float32(37.25), np.float32)
        for pname, params in D.PARAMS.items():
            out = D.run(f, iterations=25, **params)
            assert np.array_equal(_bits(out), _bits(f)), pname

    def test_zero_iterations_and_a_dimension_of_one():
        f = phantom((1, 5, 3))
        out = D.run(f, iterations=0, **D.PARAMS["A"])
        assert np.array_equal(_bits(out), _bits(f))
        for shape in FINITE_SHAPES[name]:
            assert np.all(np.isfinite(D.run(phantom(shape), iterations=7, **D.PARAMS["B"]))), shape
        # an axis of extent 1 contributes exact zeros (NDF: +0 twice): a [1][y][x] volume is the 2D run
        plane = phantom(SHAPE_2D)
        for pname, params in D.PARAMS.items():
            assert np.array_equal(_bits(D.run(plane[None], iterations=7, **params)[0]), _bits(D.run(plane, iterations=7, **params)))

    @pytest.mark.parametrize("world", [2, 3])
    def test_stitched_slabs_equal_the_whole_volume(world):
        """step_slab on slabs with GHOST ghost planes either side, exchanged after every iteration"""
        f = phantom(SHAPE_3D)
        for pname, params in D.PARAMS.items():
            want = D.cached(SHAPE_3D, pname, COUNTS)[2]
            assert np.array_equal(_bits(D.by_slabs(f, params, 2, world)), _bits(want)), (pname, world)
        want = D.cached(SHAPE_3D, "B", COUNTS)[25]
        assert np.array_equal(_bits(D.by_slabs(f, D.PARAMS["B"], 25, world)), _bits(want))

    def test_slab_step_writes_only_the_range_it_is_given():
        case = SLAB_STEP[name]
        f = phantom((g + case["nzl"] + g, 5, 9))
        out = np.full_like(f, np.nan)
        p = D.PARAMS["C"]
        D.step_slab(f, f, out, 9, 5, case["nzl"], g, g, *(p[k] for k in D.keys), *case["extra"], zr=(1, 3))
        assert np.all(np.isnan(out[:g + 1])) and np.all(np.isnan(out[g + 3:]))
        want = D.run(f, iterations=1, **p)
        assert np.array_equal(_bits(out[g + 1:g + 3]), _bits(want[g + 1:g + 3]))

    def test_the_tolerance_cases_satisfy_their_rule():
        for slab in (False, True):
            tol, stop, d_stop, seq = D.tolerance_plan(slab)
            print(f"{name} tolerance case (slab={slab}): sequence {['%.3e' % v for v in seq]}, tol {tol:.4e}, stops after {stop}")
            assert stop == 24 and d_stop < tol < seq[2]

    # -------------------------------------------------------------------------------------------- host surface
    def test_slab_state_bookkeeping():
        """the operator's MarchSlab on host tensors, g = GHOST: g ghost planes where a neighbour exists, the ranges the neighbours
        wait for, the placed slot; then one rank, host tensors, the oracle's step: the driver is the whole-volume run"""
        import torch
        from tomobar_amd import slab as S
        nz = 2 * g + 3

        def state(data, has_lo, has_hi):
            return getattr(S, op.slab)(data, has_lo, has_hi, *op.slab_args(D.PARAMS["A"]), D.step_slab)

        data = torch.arange(nz * 2 * 3, dtype=torch.float32).reshape(nz, 2, 3)
        st = state(data, True, True)
        assert (st.lo, st.hi) == (g, g) and st.inp.shape[0] == nz + 2 * g and torch.equal(st.local(st.inp), data)
        assert st.boundary_ranges() == ([(0, g), (nz - g, nz)], (g, nz - g))
        assert st.source(0) is st.inp and st.source(1) is st.U[1] and st.source(2) is st.U[0]
        (su,), (ru,), (sd,), (rd,) = st.send_up(0), st.recv_up(0), st.send_down(3), st.recv_down(3)
        assert su.shape[0] == ru.shape[0] == sd.shape[0] == rd.shape[0] == g and all(t.is_contiguous() for t in (su, ru, sd, rd))
        assert su.data_ptr() == st.inp[nz].data_ptr() and ru.data_ptr() == st.inp[nz + g].data_ptr()
        assert sd.data_ptr() == st.U[1][g].data_ptr() and rd.data_ptr() == st.U[1][0].data_ptr()
        st = state(data[:g], True, True)       # a slab of exactly g planes: all of it is boundary
        assert st.boundary_ranges() == ([(0, g)], (g, g))
        assert st.send_up(0)[0].data_ptr() == st.send_down(0)[0].data_ptr() == st.inp[g].data_ptr()
        st = state(data[:g + 1], True, True)
        assert st.boundary_ranges() == ([(0, g), (g, g + 1)], (g, g))
        st = state(data, False, True)
        assert (st.lo, st.hi) == (0, g) and st.boundary_ranges() == ([(nz - g, nz)], (0, nz - g)) and st.send_down(0) == [] and st.recv_down(0) == []
        slots = {S.PLACED_SLOT_PD, S.PLACED_SLOT_ROF, S.PLACED_SLOT_NDF, S.PLACED_SLOT_DIFF4TH, S.PLACED_SLOT_LLT_ROF}
        assert len(slots) == 5 and getattr(S, op.slot[0]) == op.slot[1]
        f = phantom((6, 5, 9))
        p = D.PARAMS["B"]
        driver = getattr(S, op.driver)
        got = driver(torch.from_numpy(f), S.SlabComm(0, 1), *D.call_args(p, 7), step_fn=D.step_slab)
        assert np.array_equal(_bits(got.numpy()), _bits(D.run(f, iterations=7, **p)))
        got = driver(torch.from_numpy(f), S.SlabComm(0, 1), *D.call_args(p, 0), step_fn=D.step_slab)
        assert np.array_equal(_bits(got.numpy()), _bits(f))

    def test_one_rank_slab_driver_is_the_whole_volume_run():
        import torch
        from tomobar_amd import slab as S
        driver = getattr(S, op.driver)
        f = phantom((6, 5, 9))
        p = D.PARAMS["B"]
        got = driver(torch.from_numpy(f), S.SlabComm(0, 1), *D.call_args(p, 7), step_fn=D.step_slab)
        assert np.array_equal(_bits(got.numpy()), _bits(D.run(f, iterations=7, **p)))
        got = driver(torch.from_numpy(f), S.SlabComm(0, 1), *D.call_args(p, 0), step_fn=D.step_slab)
        assert np.array_equal(_bits(got.numpy()), _bits(f))
        out = torch.full((6, 5, 9), float("nan"))
        info = {}
        assert driver(torch.from_numpy(f), S.SlabComm(0, 1), *D.call_args(p, 2), step_fn=D.step_slab, out=out, info=info) is out
        assert np.array_equal(_bits(out.numpy()), _bits(D.run(f, iterations=2, **p))) and info["iterations_done"] == 2

    def test_scratch_bytes():
        scratch_bytes = getattr(_lib(), f"tomo_{name.lower()}_scratch_bytes")
        from tomobar_amd import ops
        skew = ops.ARRAY_SKEW
        for dx, dy, dz in [(37, 13, 7), (64, 64, 64), (1, 1, 1), (200, 150, 40)]:
            arr3 = (dx * dy * dz * 4 + 255) // 256 * 256
            arr2 = (dx * dy * 4 + 255) // 256 * 256
            assert scratch_bytes(dx, dy, dz, 3) == arr3 + skew      # the one ping-pong partner of the output
            assert scratch_bytes(dx, dy, dz, 2) == arr2 + skew      # dz is ignored in 2D

    def test_invalid_arguments_are_refused_before_the_device_is_touched():
        from tomobar_amd import _lib
        lib, abi = _lib.lib(), ABI[name]

        def call(**kw):
            v = dict(inp=a, out=b, dx=4, dy=4, dz=4, nd=3, iters=3, tol=0.0, **abi.args)
            v.update(kw)
            return getattr(lib, f"tomo_{name.lower()}")(0, v["inp"], v["out"], v["dx"], v["dy"], v["dz"], v["nd"],
                                                        *(v[k] for k in abi.args), v["iters"], v["tol"], None, None, None)

        for kw in abi.bad:
            assert call(**kw) == _lib.E_INVALID, kw
            with pytest.raises(ValueError):
                _lib.check(call(**kw))

        def slab(**kw):
            v = dict(inp=a, u_in=b, u_out=c, dx=4, dy=4, nzl=4, lo=g, hi=g, z0=0, z1=4, **abi.args)
            v.update(kw)
            return getattr(lib, f"tomo_{name.lower()}_iter_slab_range")(0, v["inp"], v["u_in"], v["u_out"], v["dx"], v["dy"], v["nzl"], v["lo"],
                                                                        v["hi"], v["z0"], v["z1"], *(v[k] for k in abi.args), None)

        for kw in abi.bad_slab:
            assert slab(**kw) == _lib.E_INVALID, kw
        assert slab(z0=2, z1=2) == _lib.OK     # an empty range is nothing to do, before any device work

    tests = [test_z_replicated_volume_equals_the_2d_run,
             test_constant_input_is_a_fixed_point,
             test_zero_iterations_and_a_dimension_of_one,
             test_stitched_slabs_equal_the_whole_volume,
             test_slab_step_writes_only_the_range_it_is_given,
             test_the_tolerance_cases_satisfy_their_rule,
             test_slab_state_bookkeeping,
             test_scratch_bytes,
             test_invalid_arguments_are_refused_before_the_device_is_touched]
    if name != "NDF":    # (NDF's one-rank run is the end of its bookkeeping test)
        tests.append(test_one_rank_slab_driver_is_the_whole_volume_run)
    return {t.__name__: t for t in tests}
