"""Multi-process (gloo, CPU) tests of the IPC halo transport of tomobar_amd.slab.SlabComm (tomobar_amd/halo_ipc.py) on its
shared-memory provider: host tensors run the whole protocol -- tokens, acks, slot reuse, growth, several exchanges in flight,
the collective fallback and the teardown -- exactly as device tensors do over HIP IPC (tests/test_gpu_slab_ipc.py).  The
slab drivers run with the ORACLE's single-iteration functions as the compute step and must give the oracle's whole-volume
result bit for bit, as they do over the host-staged transport (tests/test_slab_gloo.py)."""
import datetime
import glob
import os
import socket
import sys
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.multiprocessing as mp  # noqa: E402

from test_slab_gloo import CASES  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = "TOMO_MI355X_HALO_TRANSPORT"


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _run_ranks(worker, world, *args, limit_s=120.0):
    """Spawn the ranks and join them with a deadline; a rank left waiting fails the test and is killed.  Returns the
    process ids of the ranks."""
    ctx = mp.start_processes(worker, args=(world, _free_port()) + args, nprocs=world, join=False, start_method="spawn")
    pids = ctx.pids()
    deadline = time.time() + limit_s
    try:
        while not ctx.join(timeout=2.0):     # raises when a rank failed
            if time.time() > deadline:
                raise AssertionError(f"{world} ranks did not finish within {limit_s:.0f} s")
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
    return pids


def _start(rank, world, port):
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.pop(ENV, None)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))   # a lost token raises
    return dist


def _segments(pid=None):
    return glob.glob(f"/dev/shm/tomo_halo_{pid if pid is not None else os.getpid()}_*")


def _check_counts(comm, world):
    st = comm.timing_summary()
    assert st["transport"] == "ipc" and "transport_note" not in st, st
    # one message each way per neighbour and exchange; tokens and acks are not counted
    assert st["messages"] == 2 * st["exchanges"] * (int(comm.has_lo) + int(comm.has_hi)), st
    return st


# ------------------------------------------------------------------------------------------------ exchanges in flight
SIZES = [((3, 3, 3, 3), (3, 2, 2, 2)), ((1, 4), (2,)), ((3, 3, 3, 3), (3, 2, 2, 2))]


def _inflight_worker(rank, world, port):
    dist = _start(rank, world, port)
    try:
        from tomobar_amd.slab import SlabComm
        comm = SlabComm(rank, world, transport="ipc")
        lo, hi = rank > 0, rank < world - 1

        def make(tag, up, down, plane=(3, 5)):
            su = [torch.full((k,) + plane, float(100 * tag + 10 * rank + i)) for i, k in enumerate(up)] if hi else []
            sd = [torch.full((k,) + plane, float(100 * tag + 10 * rank + i)) for i, k in enumerate(down)] if lo else []
            ru = [torch.zeros((k,) + plane) for k in down] if hi else []
            rd = [torch.zeros((k,) + plane) for k in up] if lo else []
            return tag, sd, rd, su, ru

        def check(tag, sd, rd, su, ru):
            for i, t in enumerate(rd):
                assert torch.all(t == float(100 * tag + 10 * (rank - 1) + i)), (rank, tag, i)
            for i, t in enumerate(ru):
                assert torch.all(t == float(100 * tag + 10 * (rank + 1) + i)), (rank, tag, i)

        sets = [make(tag, up, down) for tag, (up, down) in enumerate(SIZES)]
        handles = [comm.exchange_start(*s[1:]) for s in sets]       # three posts, nothing waited for yet
        for h in reversed(handles):                                  # ... completed out of order
            comm.exchange_wait(h)
        for s in sets:
            check(*s)
        st = _check_counts(comm, world)
        assert st["exchanges"] == 3 and comm.stats["bytes"] > 0
        tr = comm._ipc
        # three exchanges in flight took three slots: the check's region (2 slots) and one more; the sender alone decided
        assert len(tr.owned) == 2 and len(tr.mapped) == 2 * (int(lo) + int(hi)), (rank, len(tr.owned), len(tr.mapped))
        # slots come back through the acks on the neighbours' tokens: one exchange at a time needs no further region
        for tag in range(3, 9):
            s = make(tag, *SIZES[tag % 3])
            comm.exchange(*s[1:])
            check(*s)
        assert len(tr.owned) == 2, (rank, len(tr.owned))
        # a message larger than every slot: a new region on the sender's side, mapped by the receiver from the token
        s = make(9, (40, 3), (35,), plane=(7, 11))
        comm.exchange(*s[1:])
        check(*s)
        assert len(tr.owned) == 3
        _check_counts(comm, world)
        # one-way traffic across a boundary (blocks go up only): the tokens still travel both ways, so slots still return
        for tag in range(10, 16):
            up = [torch.full((2, 3, 5), float(tag + rank))] if hi else []
            rd = [torch.zeros((2, 3, 5))] if lo else []
            comm.exchange([], rd, up, [])
            assert not lo or torch.all(rd[0] == float(tag + rank - 1))
        assert len(tr.owned) == 3
        assert _segments(), "the regions are shared-memory segments of this process"
        comm.close()
        assert not _segments() and not tr.owned and not tr.mapped
        with pytest.raises(RuntimeError, match="closed"):
            comm.exchange(*sets[0][1:])
        assert comm.allreduce_sum(1.0) == world     # scalars still work
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_several_exchanges_in_flight_over_ipc(world):
    pids = _run_ranks(_inflight_worker, world)
    assert not [s for pid in pids for s in _segments(pid)], "close() unlinks every segment"


MANY = 12   # more exchanges in flight than one token carries acks for (halo_ipc.MAX_ACKS = 6)


def _many_inflight_worker(rank, world, port):
    """Posts never wait for the peer and waits never wait for a token send the peer has not confirmed: any number of exchanges
    may be in flight, completed in posting order or in reverse.  Afterwards MANY slots are due for an ack at once -- more than
    one token holds --, and all of them come back over the next tokens."""
    dist = _start(rank, world, port)
    try:
        from tomobar_amd import halo_ipc
        from tomobar_amd.slab import SlabComm
        assert MANY > halo_ipc.MAX_ACKS + 2
        comm = SlabComm(rank, world, transport="ipc")
        lo, hi = rank > 0, rank < world - 1

        def make(tag):
            su = [torch.full((2, 3, 5), float(100 * tag + rank))] if hi else []
            sd = [torch.full((1, 3, 5), float(100 * tag + rank))] if lo else []
            return sd, [torch.zeros((2, 3, 5))] if lo else [], su, [torch.zeros((1, 3, 5))] if hi else []

        def check(tag, s):
            assert all(torch.all(t == float(100 * tag + rank - 1)) for t in s[1]), (rank, tag)
            assert all(torch.all(t == float(100 * tag + rank + 1)) for t in s[3]), (rank, tag)

        tag = 0
        for order in (lambda hs: hs, reversed):
            sets = [(tag + i, make(tag + i)) for i in range(MANY)]
            tag += MANY
            handles = [comm.exchange_start(*s) for _, s in sets]
            for h in order(handles):
                comm.exchange_wait(h)
            for t, s in sets:
                check(t, s)
        tr = comm._ipc
        # the sends of all tokens the neighbours have confirmed are settled; the rest are the ones they have not spoken of yet
        assert all(len(q) <= MANY for q in tr.sends.values()), {p: len(q) for p, q in tr.sends.items()}
        regions = len(tr.owned)
        assert regions >= MANY // halo_ipc.SLOTS_PER_REGION
        for i in range(6):   # the acks of MANY slots come back six per token: no slot is lost, nothing grows
            s = make(tag + i)
            comm.exchange(*s)
            check(tag + i, s)
        assert len(tr.owned) == regions and not any(tr.acks_due[p] for p in tr.peers if len(tr.acks_due[p]) > 1)
        busy = sum(1 for o in tr.owned.values() for r in o.readers if r > 0)
        assert busy <= 2, (rank, busy)   # only the last exchange or two are still unconfirmed
        _check_counts(comm, world)
        comm.close()
        assert not _segments()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_many_exchanges_in_flight_waited_forward_and_in_reverse(world):
    _run_ranks(_many_inflight_worker, world)


# ------------------------------------------------------------------------------------------------ drivers against the oracle
def _volume(shape):
    nz, dy, dx = shape
    rng = np.random.default_rng(5)
    return (rng.random((nz, dy, dx)) * 0.3 + (np.indices((nz, dy, dx))[2] > dx // 2)).astype(np.float32)


def _tv(case, comm, vol, z0, z1):
    """(the slab driver's result over `comm`, the oracle's whole-volume result) of a case of tests/test_slab_gloo.py"""
    from oracle import tomo_oracle as O
    from tomobar_amd.slab import pd_tv_slab, rof_tv_slab
    mine = torch.from_numpy(vol[z0:z1].copy())
    if case["kind"] == "pd":
        want = O.pd_tv(vol, 0.04, case["iters"], case["mtv"], case["nn"], 8.0, case["half"])
        got = pd_tv_slab(mine, comm, 0.04, case["iters"], case["mtv"], case["nn"], 8.0, case["half"],
                         pair_fn=O.pd_pair_slab, step_fn=O.pd_step_slab)
    else:
        want = O.rof_tv(vol, 0.05, case["iters"], 0.005, case["half"])
        got = rof_tv_slab(mine, comm, 0.05, case["iters"], 0.005, case["half"], step_fn=O.rof_step_slab)
    return got.numpy(), want


def _tv_worker(rank, world, port, case):
    dist = _start(rank, world, port)
    try:
        import _cpu_backend
        _cpu_backend.install()
        from tomobar_amd.slab import SlabComm, slab_bounds
        comm = SlabComm(rank, world, transport="ipc")
        vol = _volume(case["shape"])
        z0, z1 = slab_bounds(case["shape"][0], world, rank)
        got, want = _tv(case, comm, vol, z0, z1)
        assert np.array_equal(got, want[z0:z1]), (rank, np.abs(got - want[z0:z1]).max())
        _check_counts(comm, world)
        assert comm.allreduce_max(float(rank)) == world - 1
        comm.close()
        assert not _segments()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c['kind']}-{'x'.join(map(str, c['shape']))}-h{int(c['half'])}")
def test_slab_tv_over_ipc_matches_whole_volume(world, case):
    _run_ranks(_tv_worker, world, case)


MARCH_ITERS = 6


def _march_worker(rank, world, port, shape, pname, want):
    dist = _start(rank, world, port)
    try:
        from _march_gpu import OPS
        from _tgv_oracle import phantom
        import tomobar_amd.slab as SL
        O = OPS["Diff4th"].oracle
        comm = SL.SlabComm(rank, world, transport="ipc")
        z0, z1 = SL.slab_bounds(shape[0], world, rank)
        mine = torch.from_numpy(phantom(shape)[z0:z1].copy())
        got = SL.diff4th_slab(mine, comm, *O.call_args(O.PARAMS[pname], MARCH_ITERS), step_fn=O.step_slab)
        assert np.array_equal(got.numpy().view(np.uint32), want[z0:z1].view(np.uint32)), rank
        st = _check_counts(comm, world)
        # two planes of U each way per exchange: one of U^0 and one after every iteration but the last
        assert st["exchanges"] == MARCH_ITERS, st
        assert st["bytes"] == MARCH_ITERS * (int(comm.has_lo) + int(comm.has_hi)) * 2 * shape[1] * shape[2] * 4, st
        comm.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("shape,pname", [((7, 7, 11), "A"), ((25, 6, 10), "C")], ids=["7x7x11", "25x6x10"])
def test_diff4th_slabs_over_ipc_match_whole_volume(world, shape, pname):
    """ghost depth 2; (7, 7, 11) over 3 ranks is 3 + 2 + 2 planes (the plain schedule), (25, 6, 10) overlaps"""
    from _march_gpu import OPS
    want = np.array(OPS["Diff4th"].oracle.cached(shape, pname, (MARCH_ITERS,))[MARCH_ITERS])
    _run_ranks(_march_worker, world, shape, pname, want)


# ------------------------------------------------------------------------------------------------ the collective fallback
FAULT = "injected: this rank cannot map a neighbour's region"


def _fallback_worker(rank, world, port):
    dist = _start(rank, world, port)
    try:
        import _cpu_backend
        _cpu_backend.install()
        from tomobar_amd import halo_ipc
        from tomobar_amd.slab import SlabComm, slab_bounds
        if rank == 1:   # ONE rank fails, and only when it maps a region: its own export and its tokens are fine
            def refuse(self, handle):
                raise OSError(FAULT)
            halo_ipc.ShmRegions.open = refuse
        # "ipc": a set-up failure is an error, on every rank and at once (nobody is left waiting for a token)
        t0 = time.time()
        with pytest.raises(RuntimeError, match="injected") as info:
            SlabComm(rank, world, transport="ipc")
        assert "rank 1" in str(info.value) and time.time() - t0 < 30.0, str(info.value)
        assert not _segments(), "the regions of the failed set-up are gone"
        # "auto": all ranks agree on host staging, and say why
        comm = SlabComm(rank, world, transport="auto")
        st = comm.timing_summary()
        assert st["transport"] == "staged" and FAULT in st["transport_note"] and comm._ipc is None, st
        assert not _segments()
        case = CASES[2]
        vol = _volume(case["shape"])
        z0, z1 = slab_bounds(case["shape"][0], world, rank)
        got, want = _tv(case, comm, vol, z0, z1)
        assert np.array_equal(got, want[z0:z1]), rank
        assert comm._stage_free, "the planes went through the staging buffers of the existing path"
        comm.close()   # nothing to give back
        # the variable selects the transport where none is passed, and an unknown value is refused
        os.environ[ENV] = "auto"
        assert SlabComm(rank, world).timing_summary()["transport"] == "staged"
        os.environ[ENV] = "rdma"
        with pytest.raises(ValueError, match="rdma"):
            SlabComm(rank, world)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_one_failing_rank_moves_all_ranks_to_host_staging(world):
    _run_ranks(_fallback_worker, world)


# ------------------------------------------------------------------------------------------------ the default
def _default_worker(rank, world, port):
    dist = _start(rank, world, port)
    try:
        from tomobar_amd.slab import SlabComm
        comm = SlabComm(rank, world)   # no transport, the variable unset: today's path
        assert comm._ipc is None and comm.staged and comm.transport == "staged"
        lo, hi = rank > 0, rank < world - 1
        su = [torch.full((2, 3, 5), float(rank))] if hi else []
        sd = [torch.full((1, 3, 5), float(rank))] if lo else []
        ru = [torch.zeros((1, 3, 5))] if hi else []
        rd = [torch.zeros((2, 3, 5))] if lo else []
        comm.exchange(sd, rd, su, ru)
        assert all(torch.all(t == rank - 1) for t in rd) and all(torch.all(t == rank + 1) for t in ru)
        nb = int(lo) + int(hi)
        st = comm.timing_summary()
        assert st["exchanges"] == 1 and st["messages"] == 2 * nb and st["bytes"] == 60 * (2 * int(hi) + int(lo)), st
        assert st["transport"] == "staged" and st["backend"] == "gloo" and "transport_note" not in st, st
        assert len(comm._stage_free) == 2 * nb, "one staging buffer per message, back in the pool of the existing path"
        assert not _segments()
        comm.close()
        os.environ[ENV] = "ipc"          # the same call, selected by the variable
        comm = SlabComm(rank, world)
        comm.exchange(sd, rd, su, ru)
        assert comm.timing_summary()["transport"] == "ipc" and comm._ipc.owned and not comm._stage_free
        comm.close()
    finally:
        dist.destroy_process_group()


def test_default_transport_is_the_existing_path():
    pids = _run_ranks(_default_worker, 3)
    assert not [s for pid in pids for s in _segments(pid)]
