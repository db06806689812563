"""The IPC halo transport of tomobar_amd.slab.SlabComm on the GPU: OS processes that share cuda:0 export their packed ghost
planes with HIP IPC (tomo_ipc_region_*), pack both directions with one tomo_halo_pack2 launch and pull both neighbours'
messages with one tomo_halo_pull2 launch out of the mapped regions; the tokens travel over gloo.  This is the only
device-to-device halo path that runs on a one-GPU box (RCCL refuses two ranks on one device).  What it shows: the region
calls, the two kernels and the protocol between processes ON ONE GPU -- nothing about reading a peer's region across xGMI.
The protocol itself is covered without a GPU by tests/test_slab_ipc_gloo.py.

If HIP IPC cannot be opened between two processes on a machine -- tomo_ipc_region_open returns hipIpcOpenMemHandle's error to
a rank during the collective set-up -- the tests that need it print that error and skip; every other failure, one of the
export side included, fails them.  The fallback test runs regardless."""
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

from test_gpu_slab_fista import CASES as FISTA_CASES  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = "TOMO_MI355X_HALO_TRANSPORT"
OPEN_REFUSED = "hipIpcOpenMemHandle failed"   # the text of tomo_ipc_region_open's error: the one failure that may skip


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _run_ranks(worker, world, tmp_path, *args, limit_s=120.0):
    """Spawn the ranks (at most 3, all on cuda:0) and join them with a deadline; a rank left waiting fails the test and is
    killed.  Skips -- with the error text -- if the ranks found that HIP IPC itself is refused on this machine."""
    ctx = mp.start_processes(worker, args=(world, _free_port(), str(tmp_path)) + args, nprocs=world, join=False,
                             start_method="spawn")
    deadline = time.time() + limit_s
    try:
        while not ctx.join(timeout=2.0):     # raises when a rank failed
            if time.time() > deadline:
                raise AssertionError(f"{world} ranks did not finish within {limit_s:.0f} s")
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
    refused = sorted(glob.glob(os.path.join(str(tmp_path), "ipc_refused_*.txt")))
    if refused:
        text = open(refused[0]).read()
        print(f"HIP IPC is refused between processes on this machine: {text}")
        pytest.skip(f"HIP IPC is refused between processes on this machine: {text}")


def _start(rank, world, port):
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ.pop(ENV, None)
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))   # a lost token raises
    return dist


def _ipc_comm(rank, world, tmp):
    """SlabComm(transport="ipc") on cuda:0, or None after noting the error if this rank could not OPEN a neighbour's region
    (the set-up is collective and every rank has a neighbour: where the machine refuses, every rank is refused)."""
    from tomobar_amd.slab import SlabComm
    try:
        return SlabComm(rank, world, torch.device("cuda", 0), transport="ipc")
    except RuntimeError as e:
        own = getattr(e, "own_error", None) or ""   # what THIS rank's set-up returned, not the gathered note
        if OPEN_REFUSED not in own:
            raise   # a failed export (create, handle, pack) or anything else is a failure of the code under test
        with open(os.path.join(tmp, f"ipc_refused_{rank}.txt"), "w") as f:
            f.write(own)
        return None


def _check_counts(comm):
    st = comm.timing_summary()
    assert st["transport"] == "ipc" and st["backend"] == "gloo" and "transport_note" not in st, st
    assert st["messages"] == 2 * st["exchanges"] * (int(comm.has_lo) + int(comm.has_hi)), st
    return st


# ------------------------------------------------------------------------------------------------ raw exchange
# the smallest planes that reach the three access widths of the copy kernels: 7 x 11 floats = 308 B (blocks that start 4-byte
# aligned only), 6 x 70 floats = 1680 B (16-byte path), 5 x 9 binary16 = 90 B (byte path and byte tail); block i of a message
# takes kind i % 3, so every message mixes them, and every block starts one plane into its array (an unaligned start)
PLANES = [((7, 11), torch.float32), ((6, 70), torch.float32), ((5, 9), torch.float16)]
SIZES = [((3, 3, 3, 3), (3, 2, 2, 2)), ((1, 4), (2,)), ((3, 3, 3, 3), (3, 2, 2, 2))]


def _payload(tag, rank, i, k):
    (shape, dtype) = PLANES[i % 3]
    g = torch.Generator()
    g.manual_seed(1000 * tag + 10 * rank + i)
    return torch.rand((k + 1,) + shape, generator=g).to(dtype)


def _raw_worker(rank, world, port, tmp):
    dist = _start(rank, world, port)
    try:
        comm = _ipc_comm(rank, world, tmp)
        if comm is None:
            return
        dev = torch.device("cuda", 0)
        lo, hi = rank > 0, rank < world - 1

        def make(tag, up, down):
            su = [_payload(tag, rank, i, k).to(dev)[1:] for i, k in enumerate(up)] if hi else []
            sd = [_payload(tag, rank, i, k).to(dev)[1:] for i, k in enumerate(down)] if lo else []
            ru = [torch.zeros_like(_payload(tag, rank + 1, i, k)).to(dev)[1:] for i, k in enumerate(down)] if hi else []
            rd = [torch.zeros_like(_payload(tag, rank - 1, i, k)).to(dev)[1:] for i, k in enumerate(up)] if lo else []
            return tag, sd, rd, su, ru, up, down

        def check(tag, sd, rd, su, ru, up, down):
            for i, (t, k) in enumerate(zip(rd, up)):
                assert torch.equal(t.cpu(), _payload(tag, rank - 1, i, k)[1:]), (rank, tag, "from below", i)
            for i, (t, k) in enumerate(zip(ru, down)):
                assert torch.equal(t.cpu(), _payload(tag, rank + 1, i, k)[1:]), (rank, tag, "from above", i)

        sets = [make(tag, up, down) for tag, (up, down) in enumerate(SIZES)]
        handles = [comm.exchange_start(*s[1:5]) for s in sets]      # three posts, nothing waited for yet
        for h in reversed(handles):                                  # ... completed out of order
            comm.exchange_wait(h)
        torch.cuda.synchronize()
        for s in sets:
            check(*s)
        st = _check_counts(comm)
        assert st["exchanges"] == 3, st
        comm.timing = True
        for tag in range(3, 7):   # one at a time: slots come back, no further region
            regions = len(comm._ipc.owned)
            s = make(tag, *SIZES[tag % 3])
            comm.exchange(*s[1:5])
            check(*s)
            assert tag == 3 or len(comm._ipc.owned) == regions
        assert _check_counts(comm)["wait_stream_ms"] > 0.0
        comm.close()
        assert not comm._ipc.owned and not comm._ipc.mapped
    finally:
        dist.destroy_process_group()


def test_raw_exchange_three_ranks_one_gpu(tmp_path):
    """rank 1 has two neighbours, ranks 0 and 2 an empty direction"""
    _run_ranks(_raw_worker, 3, tmp_path)


# ------------------------------------------------------------------------------------------------ TV drivers, the real HIP steps
MARCH_ITERS = 6
TV_CASES = [dict(kind="pd", shape=(19, 6, 13), iters=7, mtv=0, nn=1, half=False),
            dict(kind="pd", shape=(26, 5, 12), iters=6, mtv=0, nn=0, half=True),
            dict(kind="rof", shape=(22, 6, 10), iters=5, half=False),
            dict(kind="NDF", shape=(9, 7, 11), pname="A"),
            dict(kind="Diff4th", shape=(13, 6, 10), pname="C")]
_wants = {}


def _volume(case):
    if case["kind"] in ("NDF", "Diff4th"):
        from _tgv_oracle import phantom
        return phantom(case["shape"])
    nz, dy, dx = case["shape"]
    rng = np.random.default_rng(5)
    return (rng.random((nz, dy, dx)) * 0.3 + (np.indices((nz, dy, dx))[2] > dx // 2)).astype(np.float32)


def _want(n):
    """the oracle's whole-volume result of TV_CASES[n], computed once per session"""
    if n not in _wants:
        from oracle import tomo_oracle as O
        case = TV_CASES[n]
        vol = _volume(case)
        if case["kind"] == "pd":
            _wants[n] = O.pd_tv(vol, 0.04, case["iters"], case["mtv"], case["nn"], 8.0, case["half"])
        elif case["kind"] == "rof":
            _wants[n] = O.rof_tv(vol, 0.05, case["iters"], 0.005, case["half"])
        else:
            from _march_gpu import OPS
            _wants[n] = np.array(OPS[case["kind"]].oracle.cached(case["shape"], case["pname"], (MARCH_ITERS,))[MARCH_ITERS])
    return _wants[n]


def _drive(case, comm, rank, world):
    """this rank's slab of the case through the slab driver with the shipped HIP step, on cuda:0"""
    import tomobar_amd.slab as SL
    vol = _volume(case)
    z0, z1 = SL.slab_bounds(case["shape"][0], world, rank)
    mine = torch.from_numpy(vol[z0:z1].copy()).cuda()
    if case["kind"] == "pd":
        got = SL.pd_tv_slab(mine, comm, 0.04, case["iters"], case["mtv"], case["nn"], 8.0, case["half"])
    elif case["kind"] == "rof":
        got = SL.rof_tv_slab(mine, comm, 0.05, case["iters"], 0.005, case["half"])
    else:
        from _march_gpu import OPS
        O = OPS[case["kind"]].oracle
        got = getattr(SL, OPS[case["kind"]].driver)(mine, comm, *O.call_args(O.PARAMS[case["pname"]], MARCH_ITERS))
    torch.cuda.synchronize()
    return got.cpu().numpy(), (z0, z1)


def _tv_worker(rank, world, port, tmp, wants):
    dist = _start(rank, world, port)
    try:
        from tomobar_amd import ops
        ops.set_variant("pdtv", 22)   # PD_TV with the reference's roundings: comparable with the oracle bit for bit
        ops.set_variant("roftv", 0)
        comm = _ipc_comm(rank, world, tmp)
        if comm is None:
            return
        for case, want in zip(TV_CASES, wants):
            got, (z0, z1) = _drive(case, comm, rank, world)
            assert np.array_equal(got, want[z0:z1]), (case, rank, float(np.abs(got - want[z0:z1]).max()))
        _check_counts(comm)
        comm.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_tv_drivers_over_ipc_match_whole_volume(world, tmp_path):
    """PD_TV float32 and binary16, ROF_TV, NDF (one ghost plane) and Diff4th (two) through ONE communicator per rank: the
    exchanges differ in size from driver to driver"""
    _run_ranks(_tv_worker, world, tmp_path, [_want(n) for n in range(len(TV_CASES))])


# ------------------------------------------------------------------------------------------------ product drivers end to end
def _fista_setup(case):
    """(sinogram, the oracle's Lipschitz constant, the oracle's whole-volume reconstruction) of a case of
    tests/test_gpu_slab_fista.py, as its worker computes them"""
    from oracle import tomo_oracle as O
    nz, n, na, os_n = case["nz"], 40, 36, case["os"]
    angles = np.linspace(0, np.pi, na, endpoint=False)
    rng = np.random.default_rng(2)
    sino = np.abs(O.shepp_logan_sino(n, nz, n, angles) / n + 0.02 * rng.standard_normal((nz, na, n))).astype(np.float32)
    P = O.Projector(nz, n, n, angles, 0.0, os_n)
    L = O.power_method(P, rng.standard_normal((nz, n, n)).astype(np.float32))
    full_reg = {"regul_param": 0.001, "iterations": 150, "time_marching_step": 0.005, "PD_LipschitzConstant": 12.0,
                "methodTV": 0, **case["reg"]}
    if case["method"] == "FISTA":
        want = O.fista(P, sino, 2, L, True, full_reg, case["fid"])
    else:
        want = O.admm(P, sino, 3, L, 1.0, 1.6, False, full_reg, case["fid"])
    return sino, L, want


def _fista_worker(rank, world, port, tmp, case, sino, L, want):
    dist = _start(rank, world, port)
    try:
        from tomobar_amd import ops
        from tomobar_amd.methodsIR_CuPy import RecToolsIRCuPy
        from tomobar_amd.slab import slab_bounds
        ops.set_variant("pdtv", 22)
        comm = _ipc_comm(rank, world, tmp)
        if comm is None:
            return
        dev = torch.device("cuda", 0)
        nz, n, na, os_n = case["nz"], 40, 36, case["os"]
        angles = np.linspace(0, np.pi, na, endpoint=False)
        z0, z1 = slab_bounds(nz, world, rank)
        rt = RecToolsIRCuPy(n, 0, z1 - z0, 0.0, angles, n, 0, os_n if os_n > 1 else None)
        rt.slab = comm
        d = {"projection_data": torch.from_numpy(sino[z0:z1].copy()).to(dev),
             "data_axes_labels_order": ["detY", "angles", "detX"], "data_fidelity": case["fid"]}
        if case["method"] == "FISTA":
            got = rt.FISTA(d, {"iterations": 2, "lipschitz_const": L, "nonnegativity": True, "recon_mask_radius": None},
                           dict(case["reg"]))
        else:
            got = rt.ADMM(d, {"iterations": 3, "lipschitz_const": L, "recon_mask_radius": None}, dict(case["reg"]))
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        assert got.shape == (z1 - z0, n, n)
        assert np.array_equal(got, want[z0:z1]), (rank, float(np.abs(got - want[z0:z1]).max()))
        st = _check_counts(comm)
        assert st["exchanges"] > 0, st
        comm.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("case", [FISTA_CASES[0], FISTA_CASES[2]], ids=lambda c: f"{c['method']}-os{c['os']}-{c['fid']}-{c['reg']['method']}")
def test_two_rank_reconstruction_over_ipc_matches_whole_volume(case, tmp_path):
    _run_ranks(_fista_worker, 2, tmp_path, case, *_fista_setup(case))


# ------------------------------------------------------------------------------------------------ the fallback on the device
def _fallback_worker(rank, world, port, tmp, want):
    dist = _start(rank, world, port)
    try:
        from tomobar_amd import halo_ipc, ops
        from tomobar_amd.slab import SlabComm
        ops.set_variant("pdtv", 22)
        if rank == 1:   # this rank exports and packs, but cannot map a neighbour's region
            def refuse(self, handle):
                raise OSError("injected: hipIpcOpenMemHandle refused")
            halo_ipc.HipRegions.open = refuse
        comm = SlabComm(rank, world, torch.device("cuda", 0), transport="auto")
        st = comm.timing_summary()
        assert st["transport"] == "staged" and comm._ipc is None and comm.staged, st
        # rank 1's refusal, or -- where HIP IPC is refused altogether -- the errors of the ranks that got there first
        assert "failed its check" in st["transport_note"] and "host staging" in st["transport_note"], st
        print(f"rank {rank}: {st['transport_note']}")
        got, (z0, z1) = _drive(TV_CASES[0], comm, rank, world)
        assert np.array_equal(got, want[z0:z1]), (rank, float(np.abs(got - want[z0:z1]).max()))
        assert comm._stage_free, "the planes went through the staging buffers of the existing path"
        comm.close()
    finally:
        dist.destroy_process_group()


def test_one_failing_rank_moves_all_ranks_to_host_staging_on_the_device(tmp_path):
    _run_ranks(_fallback_worker, 3, tmp_path, _want(0))
