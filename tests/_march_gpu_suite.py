"""TEST INFRASTRUCTURE: the MI355X tests of the explicit time-marching regularisers NDF, Diff4th and LLT_ROF, written once;
tests/test_gpu_ndf.py, tests/test_gpu_diff4th.py and tests/test_gpu_llt_rof.py each collect `suite(<operator>)`.  The shipped
kernel against the float32 numpy restatement (tests/_ndf_oracle.py, tests/_diff4th_oracle.py, tests/_llt_rof_oracle.py), bit
for bit (there is no reference implementation: formula-level parity, unpinned;
docs/kernels/{ndf,diff4th,llt_rof}.md), through the ops function, the *_cupy function, the tolerance rule, the z-slab states
and driver, and the three drivers that reach it through prox_regul.  What differs between the operators is the table
tests/_march_gpu.OPS."""
import inspect
import math

import numpy as np
import pytest
import torch

import _cupy_standin
import _march_gpu as G
from _march_gpu import OPS, host, same_bits
from _tgv_oracle import phantom

COUNTS = (1, 2, 7, 40)
# the two-deep clamps overlap (extents of 1, 2, 3), tiles are ragged (60 columns per wave -- NDF: 62 --, 8 rows per lane,
# 2 x 2 waves)
SHAPES_3D = [(7, 13, 37), (2, 2, 2), (1, 5, 3), (5, 1, 3), (5, 3, 1), (3, 70, 131)]
SHAPES_2D = [(13, 37), (1, 37), (37, 1), (2, 3), (150, 200)]
SHAPES = {"NDF": SHAPES_3D + SHAPES_2D, "Diff4th": SHAPES_3D + [(3, 3, 3)] + SHAPES_2D, "LLT_ROF": SHAPES_3D + [(3, 3, 3)] + SHAPES_2D}


def suite(name):
    """{test name: test function} (and the `recorded` fixture) for the operator `name` of _march_gpu.OPS, to be put into the
    collecting module's namespace; LOW in a name below stands for the operator's name in lower case"""
    op, D = OPS[name], OPS[name].oracle

    @pytest.mark.parametrize("pname", sorted(D.PARAMS))
    @pytest.mark.parametrize("shape", SHAPES[name], ids=lambda s: "x".join(map(str, s)))
    def test_ops_equals_the_oracle(shape, pname):
        p = D.PARAMS[pname]
        want = D.cached(shape, pname, COUNTS)
        f = phantom(shape)
        for n in COUNTS:
            got, done, d = G.march(name, f, p, n)     # (the output array is pre-filled with NaN, the input checked afterwards)
            assert done == n and math.isnan(d)
            same_bits(got, want[n], (name, shape, pname, n))
        same_bits(G.march(name, f, p, 0)[0], f, (name, shape, pname, 0))   # iters = 0 copies the input

    @pytest.mark.parametrize("pname", sorted(D.PARAMS))
    def test_several_tiles_and_z_chunks(pname):
        """(40, 150, 200): a workgroup covers 2 x 60 (NDF: 2 x 62) columns by 2 x 8 rows, so 2 x 10 workgroup tiles in x and y
        (4 waves wide in x, the last one ragged), and, small volumes being z-chunked, three z-chunks of 14, 14 and 12 planes:
        Diff4th's and LLT_ROF's second and third start with the seam prologue (two W planes; E3 of two planes and R3 of one,
        from the planes below the seam)"""
        shape = (40, 150, 200)
        want = D.cached(shape, pname, (10,))[10]
        same_bits(G.march(name, phantom(shape), D.PARAMS[pname], 10)[0], want, (name, shape, pname))

    # -------------------------------------------------------------------------------------------- the *_cupy function
    def test_cupy_surface(monkeypatch):
        from tomobar_amd.regularisersCuPy import last_prox
        fn = G.cupy_fn(name)
        plane = phantom((13, 37))
        want2d = D.cached((13, 37), "A", COUNTS)[7]
        # a singleton axis in each position runs the 2D kernels and keeps its shape
        for axis in range(3):
            x = torch.from_numpy(np.expand_dims(plane, axis)).cuda()
            got = G.cupy(name, x)
            assert tuple(got.shape) == tuple(x.shape)
            same_bits(np.squeeze(host(got), axis), want2d, ("singleton axis", axis))
            assert last_prox()[0] == 7 and math.isnan(last_prox()[1])
        # a non-contiguous input; the input array is unchanged
        vol = phantom((7, 13, 37))
        want3d = D.cached((7, 13, 37), "B", COUNTS)[7]
        xt = torch.from_numpy(np.ascontiguousarray(vol.transpose(2, 1, 0))).cuda().permute(2, 1, 0)
        assert not xt.is_contiguous()
        keep = xt.clone()
        same_bits(host(G.cupy(name, xt, pname="B")), want3d, "non-contiguous input")
        assert torch.equal(xt, keep), "the input array was written"
        # out=, and two calls give identical bits
        x = torch.from_numpy(vol).cuda()
        out = torch.full_like(x, float("nan"))
        res = G.cupy(name, x, pname="B", out=out)
        assert res.data_ptr() == out.data_ptr()
        same_bits(host(out), want3d, "out=")
        same_bits(host(G.cupy(name, x, pname="B")), host(out), "second call")
        assert np.array_equal(host(x), vol), "the input array was written"
        # a CuPy-like array in -> the same kind out
        cupy = _cupy_standin.install(monkeypatch)
        res = G.cupy(name, cupy.ndarray(x), pname="B")
        assert type(res) is cupy.ndarray and res.data.ptr != x.data_ptr()
        same_bits(res.get(), want3d, "CuPy-like input")
        # errors: dtype, gpu_id, the operator's own (NDF: an unknown penalty), a bad tolerance, out aliasing the input,
        # non-positive scalars
        with pytest.raises(ValueError, match="float32"):
            G.cupy(name, x.double())
        with pytest.raises(ValueError, match="gpu_device"):
            fn(x, *D.call_args(op.good, 3), -1)
        for change, message in op.refused:
            with pytest.raises(ValueError, match=message):
                fn(x, *D.call_args(dict(op.good, **change), 3), 0)
        with pytest.raises(ValueError):
            G.cupy(name, x, tolerance=-1.0)
        with pytest.raises(ValueError, match="alias"):
            G.cupy(name, x, out=x)
        for bad in op.not_positive:
            with pytest.raises(ValueError, match="positive"):
                fn(x, *D.call_args(dict(op.good, **bad), 3), 0)

    def test_reserve_tv_scratch():
        from tomobar_amd import ops
        ops.reserve_tv_scratch((7, 13, 37), "cuda:0", name)
        ops.reserve_tv_scratch((13, 37), "cuda:0", name)
        same_bits(G.march(name, phantom((7, 13, 37)), D.PARAMS["C"], 7)[0], D.cached((7, 13, 37), "C", COUNTS)[7], "after reserve")

    # -------------------------------------------------------------------------------------------- tolerance
    def test_tolerance_stops_where_the_oracle_sequence_stops():
        from tomobar_amd.regularisersCuPy import last_prox
        c = D.TOL_CASE
        tol, stop, d_stop, seq = D.tolerance_plan()
        x = torch.from_numpy(phantom(c["shape"])).cuda()
        got = host(G.cupy(name, x, c["iterations"], c["pname"], tolerance=tol))
        done, d = last_prox()
        print(f"{name} tolerance {tol:.6e}: stopped after {done} (oracle {stop}), d {d:.6e} (oracle {d_stop:.6e})")
        assert done == stop
        assert abs(d - d_stop) <= got.size * 2.0 ** -53 * d_stop
        plain = host(G.cupy(name, x, stop, c["pname"]))
        assert last_prox()[0] == stop and math.isnan(last_prox()[1])
        same_bits(got, plain, "a stopped run returns what iterations = n returns")
        same_bits(got, D.cached(c["shape"], c["pname"], tuple(range(6, 61, 6)))[stop], "stopped run against the oracle")
        # an odd request: iterate 24 then lives in the work array and is copied to the output
        got_odd = host(G.cupy(name, x, c["iterations"] - 1, c["pname"], tolerance=tol))
        assert last_prox()[0] == stop
        same_bits(got_odd, plain, "a stopped run of an odd request")
        # a threshold below the whole sequence: every iteration runs
        never = 0.5 * min(seq)
        full = host(G.cupy(name, x, c["iterations"], c["pname"], tolerance=never))
        done, d = last_prox()
        assert done == c["iterations"] and d > never
        same_bits(full, host(G.cupy(name, x, c["iterations"], c["pname"])), "tolerance never met")

    # -------------------------------------------------------------------------------------------- z-slabs on the one GPU
    @pytest.mark.parametrize("world", [2, 3])
    @pytest.mark.parametrize("schedule", ["plain", "ranges"])
    @pytest.mark.parametrize("pname", op.slab_pnames, ids=op.slab_ids)
    def test_slabs_equal_whole_volume(world, schedule, pname):
        G.check_slabs_equal_whole_volume(name, world, schedule, pname)

    @pytest.mark.parametrize("schedule", ["plain", "ranges"])
    @pytest.mark.parametrize("bounds", [[(0, 2), (2, 19)], [(0, 9), (9, 11), (11, 19)], [(0, 17), (17, 19)]],
                             ids=["2+17", "9+2+8", "17+2"])
    def test_slab_of_exactly_two_planes(bounds, schedule, shape=(19, 21, 90), iters=6):
        """one rank owns exactly two planes: both are boundary planes, and both of its neighbour's ghost planes come from it"""
        vd = torch.from_numpy(phantom(shape)).cuda()
        want = D.cached(shape, "A", (iters,))[iters]
        same_bits(G.run_slabs(name, vd, bounds, schedule, "A", iters), want, (name, bounds, schedule))

    @pytest.mark.parametrize("pname", op.slab_pnames, ids=op.slab_ids)
    def test_slab_driver_on_one_rank_equals_the_cupy_function(pname):
        from tomobar_amd import slab as S
        driver = getattr(S, op.driver)
        p = D.PARAMS[pname]
        vd = torch.from_numpy(phantom((19, 21, 90))).cuda()
        want = host(G.cupy(name, vd, 7, pname))
        got = driver(vd, S.SlabComm(0, 1), *D.call_args(p, 7))
        same_bits(host(got), want, (name, pname))
        out = torch.full_like(vd, float("nan"))
        info = {}
        assert driver(vd, S.SlabComm(0, 1), *D.call_args(p, 7), out=out, info=info) is out
        same_bits(host(out), want, (name, pname, "out="))
        assert info["iterations_done"] == 7 and math.isnan(info["rel_change"])
        same_bits(host(driver(vd, S.SlabComm(0, 1), *D.call_args(p, 0))), host(vd), "zero iterations")

    # -------------------------------------------------------------------------------------------- drivers
    def _call(name, reg, **changed):
        """what a call of the ops function records under the dictionary `reg`: the scalars as float32"""
        reg = dict(reg, **changed)
        n = len(D.keys)
        keys = op.reg_keys
        return ((G.NZ, G.NN, G.NN),) + tuple(np.float32(reg[k]) for k in keys[:n]) + tuple(reg[k] for k in keys[n:]) + (reg["iterations"], 0.0)

    def _reg_args(name, reg):
        """`reg` in the order the *_cupy function takes it"""
        a, b, tau, *rest = (reg[k] for k in op.reg_keys)
        return (a, b, reg["iterations"], tau, *rest)

    @pytest.fixture
    def recorded(monkeypatch):
        """a recording wrapper round the ops function: the shape and the scalars of every call, defaults filled in"""
        from tomobar_amd import ops
        calls, real = [], G.ops_fn(name)

        def wrapper(data, out, *args, **kw):
            bound = inspect.signature(real).bind(data, out, *args, **kw)
            bound.apply_defaults()
            calls.append((tuple(data.shape),) + tuple(bound.arguments.values())[2:])
            return real(data, out, *args, **kw)

        monkeypatch.setattr(ops, name.lower(), wrapper)
        return calls

    def _check_calls(name, calls, count, **changed):
        assert len(calls) == count, (len(calls), count)
        want = _call(name, op.REG, **changed)
        for c in calls:
            assert c == want and all(type(a) is type(b) for a, b in zip(c[1:4], want[1:4])), (c, want)

    def test_fista_one_iteration_is_the_prox_of_the_gradient_step(recorded):
        from tomobar_amd.supp.suppTools import check_kwargs
        REG = op.REG
        algo = {"iterations": 1, "lipschitz_const": 3000.0}
        got = G.rt().FISTA(G.data(), dict(algo), dict(REG))
        _check_calls(name, recorded, 1)
        step = G.rt().FISTA(G.data(), dict(algo, recon_mask_radius=None), None)    # the gradient step, unmasked
        want = G.cupy_fn(name)(step, *_reg_args(name, REG), 0)
        want = check_kwargs(want, cupyrun=True, recon_mask_radius=1.0)          # the mask, applied afterwards as the driver does
        same_bits(host(got), host(want), "FISTA, one iteration")
        assert not np.array_equal(host(got), host(check_kwargs(step.clone(), cupyrun=True, recon_mask_radius=1.0))), "the prox did nothing"

    @pytest.mark.parametrize("driver", ["FISTA", "ADMM"])
    def test_ordered_subsets_drivers_call_the_prox_every_sub_iteration(driver, recorded):
        REG = op.REG
        algo = {"iterations": 2, "lipschitz_const": 3000.0}
        rho = 2.0
        if driver == "ADMM":
            algo["ADMM_rho_const"] = rho
        reg = dict(REG)
        got = host(getattr(G.rt(3), driver)(G.data(), dict(algo), reg))
        # dicts_check adds its defaults to the caller's dictionary; ADMM's weights / rho (regul_param; LLT_ROF: and regul_param2)
        # go to a copy
        assert {k: reg[k] for k in REG} == REG, "the caller's values were rewritten"
        div = rho if driver == "ADMM" else 1.0
        _check_calls(name, recorded, 2 * 3, **{k: REG[k] / div for k in op.weights})
        plain = host(getattr(G.rt(3), driver)(G.data(), dict(algo), None))
        assert len(recorded) == 6
        assert np.all(np.isfinite(got)) and not np.array_equal(got, plain)

    def test_osem_runs_with_the_prox_and_differs_from_the_unregularised_run(recorded):
        algo = {"iterations": 2}
        got = host(G.rt(3).OSEM(G.data(), dict(algo), dict(op.REG, **op.osem)))
        want = _call(name, op.REG, **op.osem)
        changed = [1 + op.reg_keys.index(k) for k in op.osem]
        assert len(recorded) >= 1 and all(c[i] == want[i] for c in recorded for i in changed)
        n_calls = len(recorded)
        plain = host(G.rt(3).OSEM(G.data(), dict(algo), None))
        assert len(recorded) == n_calls
        assert np.all(np.isfinite(got)) and not np.array_equal(got, plain)

    tests = {k.replace("LOW", name.lower()): v for k, v in {
        "test_ops_LOW_equals_the_oracle": test_ops_equals_the_oracle,
        "test_several_tiles_and_z_chunks": test_several_tiles_and_z_chunks,
        "test_LOW_cupy_surface": test_cupy_surface,
        "test_reserve_tv_scratch_for_LOW": test_reserve_tv_scratch,
        "test_tolerance_stops_where_the_oracle_sequence_stops": test_tolerance_stops_where_the_oracle_sequence_stops,
        "test_LOW_slabs_equal_whole_volume": test_slabs_equal_whole_volume,
        "test_LOW_slab_driver_on_one_rank_equals_LOW_cupy": test_slab_driver_on_one_rank_equals_the_cupy_function,
        "recorded": recorded,
        "test_fista_one_iteration_is_the_prox_of_the_gradient_step": test_fista_one_iteration_is_the_prox_of_the_gradient_step,
        "test_ordered_subsets_drivers_call_the_prox_every_sub_iteration": test_ordered_subsets_drivers_call_the_prox_every_sub_iteration,
        "test_osem_runs_with_LOW_and_differs_from_the_unregularised_run": test_osem_runs_with_the_prox_and_differs_from_the_unregularised_run,
    }.items()}
    if D.GHOST == 2:    # (a slab of exactly GHOST planes is tested where GHOST is two)
        tests[f"test_{name.lower()}_slab_of_exactly_two_planes"] = test_slab_of_exactly_two_planes
    return tests
