"""Multi-process (gloo, CPU) tests of the LLT_ROF z-slab driver tomobar_amd.slab.llt_rof_slab: every rank owns a slab of the
phantom, runs the driver with the ORACLE's single-iteration function (tests/_llt_rof_oracle.llt_rof_step_slab) as the
compute step, and checks its slab against the oracle's whole-volume result -- bit for bit.  The pattern of
tests/test_diff4th_slab_gloo.py."""
import os
import socket
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.multiprocessing as mp  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _llt_rof_oracle as N  # noqa: E402

ITERS = 6


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


def _worker(rank, world, port, shape, pname, want, overlap):
    dist = _start(rank, world, port)
    try:
        import _llt_rof_oracle as O
        from tomobar_amd.slab import LltRofSlab, SlabComm, llt_rof_slab, slab_bounds
        comm = SlabComm(rank, world)
        p = O.PARAMS[pname]
        vol = O.phantom(shape)
        z0, z1 = slab_bounds(shape[0], world, rank)
        mine = torch.from_numpy(vol[z0:z1].copy())
        edges, interior = LltRofSlab(mine, comm.has_lo, comm.has_hi, O.llt_rof_step_slab).boundary_ranges()
        calls = []

        def step(*args):
            calls.append(args[11] if len(args) > 11 else None)   # the plane range, None = all local planes
            O.llt_rof_step_slab(*args)

        got = llt_rof_slab(mine, comm, p["lam_rof"], p["lam_llt"], ITERS, p["tau"], step_fn=step, overlap=overlap)
        assert np.array_equal(got.numpy().view(np.uint32), want[z0:z1].view(np.uint32)), (rank, np.abs(got.numpy() - want[z0:z1]).max())
        assert np.array_equal(mine.numpy(), vol[z0:z1]), "the input was written"
        # the schedule: with an interior of at least 4 planes every iteration but the last computes the edge planes first,
        # then the interior (the exchange is in flight in between); the last iteration is one call
        if overlap and interior[1] - interior[0] >= 4:
            assert calls == (list(edges) + [interior]) * (ITERS - 1) + [None], (rank, calls)
        else:
            assert calls == [None] * ITERS, (rank, calls)
        # one exchange of U^0 and one after every iteration but the last; one message each way per neighbour and exchange,
        # two planes of U in each
        st = comm.timing_summary()
        assert st["exchanges"] == ITERS, st
        assert st["messages"] == 2 * ITERS * (int(comm.has_lo) + int(comm.has_hi)), st
        assert st["bytes"] == ITERS * (int(comm.has_lo) + int(comm.has_hi)) * 2 * shape[1] * shape[2] * 4, st
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("schedule", ["plain", "overlapped"])
@pytest.mark.parametrize("shape,pname", [((7, 7, 11), "A"), ((25, 6, 10), "C")], ids=["7x7x11", "25x6x10"])
def test_llt_rof_slabs_match_whole_volume(world, schedule, shape, pname):
    """(25, 6, 10): 13 + 12 and 9 + 8 + 8 planes, interiors of at least 4 planes, so "overlapped" computes the two boundary
    planes per interior boundary first; (7, 7, 11) over 3 ranks is 3 + 2 + 2: slabs of exactly two planes, no interior, the
    plain order whatever was asked for"""
    want = np.array(N.cached(shape, pname, (ITERS,))[ITERS])
    mp.start_processes(_worker, args=(world, _free_port(), shape, pname, want, schedule == "overlapped"), nprocs=world,
                       join=True, start_method="spawn")


def _tolerance_worker(rank, world, port, plan):
    dist = _start(rank, world, port)
    try:
        import _llt_rof_oracle as O
        import tomobar_amd.slab as SL
        SL._hip_rel_change = O.rel_change_sums   # host tensors: the float64 sums tomo_rel_change returns
        c = O.TOL_CASE_SLAB
        p = O.PARAMS[c["pname"]]
        vol = O.phantom(c["shape"])
        z0, z1 = SL.slab_bounds(c["shape"][0], world, rank)
        mine = torch.from_numpy(vol[z0:z1].copy())
        comm = SL.SlabComm(rank, world)
        info = {}
        got = SL.llt_rof_slab(mine, comm, p["lam_rof"], p["lam_llt"], c["iterations"], p["tau"], step_fn=O.llt_rof_step_slab,
                          tolerance=plan["tol"], info=info)
        assert info["iterations_done"] == plan["stop"], (rank, info, plan["stop"])
        assert abs(info["rel_change"] - plan["d_stop"]) <= vol.size * 2.0 ** -53 * plan["d_stop"], (rank, info, plan["d_stop"])
        assert np.array_equal(got.numpy().view(np.uint32), plan["want_stop"][z0:z1].view(np.uint32)), rank
        info = {}
        got = SL.llt_rof_slab(mine, comm, p["lam_rof"], p["lam_llt"], c["iterations"], p["tau"], step_fn=O.llt_rof_step_slab,
                          tolerance=plan["never"], info=info)
        assert info["iterations_done"] == c["iterations"] and info["rel_change"] > plan["never"], (rank, info)
        assert np.array_equal(got.numpy().view(np.uint32), plan["want_full"][z0:z1].view(np.uint32)), rank
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_llt_rof_slab_tolerance_stops_where_the_whole_volume_sequence_stops(world):
    """the threshold comes from the oracle's own sequence (tolerance_plan): all ranks stop after iteration 24 with the
    whole-volume d, and hold the planes of the unsharded run of 24 iterations"""
    c = N.TOL_CASE_SLAB
    tol, stop, d_stop, seq = N.tolerance_plan(True)
    its = N.cached(c["shape"], c["pname"], (stop, c["iterations"]))
    plan = dict(tol=tol, stop=stop, d_stop=d_stop, never=0.5 * min(seq), want_stop=np.array(its[stop]),
                want_full=np.array(its[c["iterations"]]))
    mp.start_processes(_tolerance_worker, args=(world, _free_port(), plan), nprocs=world, join=True, start_method="spawn")
