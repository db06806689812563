"""TEST INFRASTRUCTURE: the multi-process (gloo, CPU) tests of the z-slab drivers of the explicit time-marching regularisers --
tomobar_amd.slab.ndf_slab, diff4th_slab, llt_rof_slab --, written once; tests/test_ndf_slab_gloo.py,
tests/test_diff4th_slab_gloo.py and tests/test_llt_rof_slab_gloo.py each collect `suite(<operator>)`.  Every rank owns a slab of the
phantom, runs the driver with the ORACLE's single-iteration function (the `step_slab` of the operator's record,
tests/_march_oracle.py) as the compute step, and checks its slab against the oracle's whole-volume result -- bit for bit.
The pattern of tests/test_slab_gloo.py."""
import os
import socket
import sys

import numpy as np
import pytest

import torch
import torch.multiprocessing as mp

from _march_gpu import OPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ITERS = 6
# [(shape, parameter set, the schedule asked for, the case's name)].  NDF, one ghost plane: (22, 6, 10) is 11 + 11 and
# 8 + 7 + 7 planes, long enough for the overlapped schedule; (9, 7, 11) over 3 ranks is 3 + 3 + 3, the plain schedule.
# Diff4th and LLT_ROF, two: (25, 6, 10) is 13 + 12 and 9 + 8 + 8 planes, interiors of at least 4 planes, so "overlapped"
# computes the two boundary planes per interior boundary first; (7, 7, 11) over 3 ranks is 3 + 2 + 2: slabs of exactly two
# planes, no interior, the plain order whatever was asked for.
TWO_PLANE_CASES = [(shape, pname, schedule, f"{'x'.join(map(str, shape))}-{schedule}")
                   for shape, pname in [((7, 7, 11), "A"), ((25, 6, 10), "C")] for schedule in ("plain", "overlapped")]
CASES = {"NDF": [(shape, pname, "overlapped", f"{'x'.join(map(str, shape))}-{penalty}") for shape in [(9, 7, 11), (22, 6, 10)]
                 for penalty, pname in (("Huber", "A"), ("PM", "B"), ("Tukey", "C"))],
         "Diff4th": TWO_PLANE_CASES, "LLT_ROF": TWO_PLANE_CASES}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _start(rank, world, port):
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    return dist


def _worker(rank, world, port, name, shape, pname, want, overlap):
    dist = _start(rank, world, port)
    try:
        from _march_gpu import OPS
        from _tgv_oracle import phantom
        import tomobar_amd.slab as SL
        op, O = OPS[name], OPS[name].oracle
        comm = SL.SlabComm(rank, world)
        p = O.PARAMS[pname]
        vol = phantom(shape)
        z0, z1 = SL.slab_bounds(shape[0], world, rank)
        mine = torch.from_numpy(vol[z0:z1].copy())
        edges, interior = getattr(SL, op.slab)(mine, comm.has_lo, comm.has_hi, *op.slab_args(p), O.step_slab).boundary_ranges()
        calls = []
        zr_at = 8 + len(O.keys) + len(O.extra)

        def step(*args):
            calls.append(args[zr_at] if len(args) > zr_at else None)   # the plane range, None = all local planes
            O.step_slab(*args)

        got = getattr(SL, op.driver)(mine, comm, *O.call_args(p, ITERS), step_fn=step, overlap=overlap)
        assert np.array_equal(got.numpy().view(np.uint32), want[z0:z1].view(np.uint32)), (rank, np.abs(got.numpy() - want[z0:z1]).max())
        assert np.array_equal(mine.numpy(), vol[z0:z1]), "the input was written"
        # the schedule: with an interior of at least 4 planes every iteration but the last computes the edge planes first,
        # then the interior (the exchange is in flight in between); the last iteration is one call
        if overlap and interior[1] - interior[0] >= 4:
            assert calls == (list(edges) + [interior]) * (ITERS - 1) + [None], (rank, calls)
        else:
            assert calls == [None] * ITERS, (rank, calls)
        # one exchange of U^0 and one after every iteration but the last; one message each way per neighbour and exchange,
        # the ghost depth in planes of U in each
        st = comm.timing_summary()
        assert st["exchanges"] == ITERS, st
        assert st["messages"] == 2 * ITERS * (int(comm.has_lo) + int(comm.has_hi)), st
        assert st["bytes"] == ITERS * (int(comm.has_lo) + int(comm.has_hi)) * O.GHOST * shape[1] * shape[2] * 4, st
    finally:
        dist.destroy_process_group()


def _tolerance_worker(rank, world, port, name, plan):
    dist = _start(rank, world, port)
    try:
        import _march_oracle
        from _march_gpu import OPS
        from _tgv_oracle import phantom
        import tomobar_amd.slab as SL
        SL._hip_rel_change = _march_oracle.rel_change_sums   # host tensors: the float64 sums tomo_rel_change returns
        O, driver = OPS[name].oracle, getattr(SL, OPS[name].driver)
        c = O.TOL_CASE_SLAB
        p = O.PARAMS[c["pname"]]
        vol = phantom(c["shape"])
        z0, z1 = SL.slab_bounds(c["shape"][0], world, rank)
        mine = torch.from_numpy(vol[z0:z1].copy())
        comm = SL.SlabComm(rank, world)
        info = {}
        got = driver(mine, comm, *O.call_args(p, c["iterations"]), step_fn=O.step_slab, tolerance=plan["tol"], info=info)
        assert info["iterations_done"] == plan["stop"], (rank, info, plan["stop"])
        assert abs(info["rel_change"] - plan["d_stop"]) <= vol.size * 2.0 ** -53 * plan["d_stop"], (rank, info, plan["d_stop"])
        assert np.array_equal(got.numpy().view(np.uint32), plan["want_stop"][z0:z1].view(np.uint32)), rank
        info = {}
        got = driver(mine, comm, *O.call_args(p, c["iterations"]), step_fn=O.step_slab, tolerance=plan["never"], info=info)
        assert info["iterations_done"] == c["iterations"] and info["rel_change"] > plan["never"], (rank, info)
        assert np.array_equal(got.numpy().view(np.uint32), plan["want_full"][z0:z1].view(np.uint32)), rank
    finally:
        dist.destroy_process_group()


def suite(name):
    """{test name: test function} for the operator `name` of _march_gpu.OPS, to be put into the collecting module's
    namespace"""
    O = OPS[name].oracle

    @pytest.mark.parametrize("world", [2, 3])
    @pytest.mark.parametrize("shape,pname,schedule", [c[:3] for c in CASES[name]], ids=[c[3] for c in CASES[name]])
    def test_slabs_match_whole_volume(world, shape, pname, schedule):
        want = np.array(O.cached(shape, pname, (ITERS,))[ITERS])
        mp.start_processes(_worker, args=(world, _free_port(), name, shape, pname, want, schedule == "overlapped"), nprocs=world,
                           join=True, start_method="spawn")

    @pytest.mark.parametrize("world", [2, 3])
    def test_slab_tolerance_stops_where_the_whole_volume_sequence_stops(world):
        """the threshold comes from the oracle's own sequence (tolerance_plan): all ranks stop after iteration 24 with the
        whole-volume d, and hold the planes of the unsharded run of 24 iterations"""
        c = O.TOL_CASE_SLAB
        tol, stop, d_stop, seq = O.tolerance_plan(True)
        its = O.cached(c["shape"], c["pname"], (stop, c["iterations"]))
        plan = dict(tol=tol, stop=stop, d_stop=d_stop, never=0.5 * min(seq), want_stop=np.array(its[stop]),
                    want_full=np.array(its[c["iterations"]]))
        mp.start_processes(_tolerance_worker, args=(world, _free_port(), name, plan), nprocs=world, join=True, start_method="spawn")

    low = name.lower()
    return {f"test_{low}_slabs_match_whole_volume": test_slabs_match_whole_volume,
            f"test_{low}_slab_tolerance_stops_where_the_whole_volume_sequence_stops":
                test_slab_tolerance_stops_where_the_whole_volume_sequence_stops}
