"""TEST INFRASTRUCTURE: what the MI355X tests of the explicit time-marching regularisers (NDF, Diff4th, LLT_ROF) share --
tests/_march_gpu_suite.py, tests/test_gpu_edge_shapes.py, tests/test_gpu_llt_rof_edges.py: the bit comparison, the
NaN-filled run of an ops function, the z-slab runner on one GPU, the set-up of the reconstruction drivers, and OPS, the table
of what differs between the operators.  OPS names tomobar_amd's functions and classes as strings, so the CPU suites
(tests/_march_oracle_suite.py, tests/_march_gloo_suite.py) read it too; nothing here touches a GPU on import."""
import types

import numpy as np
import torch

import _diff4th_oracle
from _guarded import guarded
import _llt_rof_oracle
import _ndf_oracle
from _tgv_oracle import phantom


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def same_bits(got, want, what):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, what
    if not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        raise AssertionError((what, f"{len(bad)} of {got.size} values differ, first at {tuple(bad[0])}",
                              float(np.abs(got.astype(np.float64) - want).max())))


def run_op(call, f_host):
    """call(input tensor, NaN-filled output tensor) on the GPU, both inside guard bands (tests/_guarded.py: a load from
    outside the input returns NaN); the input's bits and both arrays' bands are checked afterwards.  Returns the output on
    the host and what `call` returned."""
    x, out = guarded(f_host), guarded(f_host.shape)
    res = call(x.view, out.view)
    assert x.unchanged(), "the input was written"
    x.check(("the input", f_host.shape))
    out.check(("the output", f_host.shape))
    return out.host(), res


# ------------------------------------------------------------------------------------------------ the operators
def _penalty_id(p):
    from tomobar_amd._lib import ndf_penalty_id
    return (ndf_penalty_id(p["penalty"]),)


# oracle: the operator's record (tests/_march_oracle.Marcher); its name in lower case is the ops function and the C prefix
# cupy / slab / hip_step / driver: the names in tomobar_amd.regularisersCuPy and tomobar_amd.slab; slab_args: what the slab
#   class takes between has_hi and step_fn, from a parameter set
# slot: the operator's PLACED_SLOT_* name and number
# slab_pnames: the parameter sets of the z-slab tests (NDF: one per penalty, which names the case: slab_ids)
# good / refused / not_positive: the *_cupy error cases -- a valid set, [(change, the message)], the changes refused as
#   "positive"
# REG: the regularisation dictionary of the driver tests; reg_keys: its keys in the order of the ops call's parameters;
#   weights: the keys ADMM divides by rho; osem: the changes of the OSEM test
OPS = {
    "NDF": types.SimpleNamespace(
        oracle=_ndf_oracle.ORACLE, cupy="NDF_cupy", slab="NdfSlab", hip_step="_hip_ndf_step", driver="ndf_slab",
        slab_args=_penalty_id, slot=("PLACED_SLOT_NDF", 2), slab_pnames=("A", "B", "C"), slab_ids=("Huber", "PM", "Tukey"),
        good=dict(lam=1.0, sigma=2.0, tau=0.05, penalty="Huber"), refused=[(dict(penalty="Welsch"), "NDF penalty")],
        not_positive=(dict(lam=0.0), dict(sigma=-1.0), dict(tau=0.0)),
        REG=dict(method="NDF", regul_param=0.02, iterations=5, time_marching_step=0.04, edge_threshold=0.015, NDF_penalty="PM"),
        reg_keys=("regul_param", "edge_threshold", "time_marching_step", "NDF_penalty"), weights=("regul_param",),
        osem=dict(NDF_penalty="Tukey", edge_threshold=0.05)),
    "Diff4th": types.SimpleNamespace(
        oracle=_diff4th_oracle.ORACLE, cupy="Diff4th_cupy", slab="Diff4thSlab", hip_step="_hip_diff4th_step",
        driver="diff4th_slab", slab_args=lambda p: (), slot=("PLACED_SLOT_DIFF4TH", 3), slab_pnames=("A", "B", "C"),
        slab_ids=None,
        good=dict(lam=1.0, sigma=2.0, tau=0.005), refused=[],
        not_positive=(dict(lam=0.0), dict(sigma=-1.0), dict(tau=0.0)),
        REG=dict(method="Diff4th", regul_param=0.5, iterations=5, time_marching_step=0.01, edge_threshold=0.02),
        reg_keys=("regul_param", "edge_threshold", "time_marching_step"), weights=("regul_param",),
        osem=dict(edge_threshold=0.05)),
    "LLT_ROF": types.SimpleNamespace(
        oracle=_llt_rof_oracle.ORACLE, cupy="LLT_ROF_cupy", slab="LltRofSlab", hip_step="_hip_llt_rof_step",
        driver="llt_rof_slab", slab_args=lambda p: (), slot=("PLACED_SLOT_LLT_ROF", 4), slab_pnames=("A", "B", "C"),
        slab_ids=None,
        good=dict(lam_rof=0.3, lam_llt=0.1, tau=0.005), refused=[],
        not_positive=(dict(lam_rof=0.0), dict(lam_llt=-1.0), dict(lam_llt=0.0), dict(tau=0.0)),
        REG=dict(method="LLT_ROF", regul_param=0.5, regul_param2=0.25, iterations=5, time_marching_step=0.01),
        reg_keys=("regul_param", "regul_param2", "time_marching_step"), weights=("regul_param", "regul_param2"),
        osem=dict(regul_param2=0.05)),
}


def f32(D, p):
    return tuple(np.float32(p[k]) for k in D.keys)


def ops_fn(name):
    from tomobar_amd import ops
    return getattr(ops, name.lower())


def march(name, f_host, p, iterations, tolerance=0.0):
    """the ops function on the GPU: (the output, iterations done, d)"""
    D = OPS[name].oracle
    got, (_, done, d) = run_op(lambda x, out: ops_fn(name)(x, out, *f32(D, p), *(p[k] for k in D.extra), iterations, tolerance), f_host)
    return got, done, d


def cupy_fn(name):
    from tomobar_amd import regularisersCuPy
    return getattr(regularisersCuPy, OPS[name].cupy)


def cupy(name, x, iterations=7, pname="A", **kw):
    """the *_cupy function on GPU 0 under the parameter set `pname`"""
    D = OPS[name].oracle
    return cupy_fn(name)(x, *D.call_args(D.PARAMS[pname], iterations), 0, **kw)


# ------------------------------------------------------------------------------------------------ z-slabs on the one GPU
def copy_halos(states, it):
    """rank r's send_up -> rank r+1's recv_down; rank r+1's send_down -> rank r's recv_up (planes of iterate `it`)"""
    for r in range(len(states) - 1):
        lo, hi = states[r], states[r + 1]
        for src, dst in zip(lo.send_up(it), hi.recv_down(it)):
            dst.copy_(src)
        for src, dst in zip(hi.send_down(it), lo.recv_up(it)):
            dst.copy_(src)


def run_slabs(name, vd, bounds, schedule, pname, iters):
    """the device volume `vd` as one slab state per plane range of `bounds`, marched with the shipped step and exchanged by
    copies; the stitched result on the host"""
    from tomobar_amd import slab as S
    op = OPS[name]
    p = op.oracle.PARAMS[pname]
    states = []
    for r, (z0, z1) in enumerate(bounds):
        states.append(getattr(S, op.slab)(vd[z0:z1].contiguous(), r > 0, r < len(bounds) - 1, *op.slab_args(p),
                                          getattr(S, op.hip_step)))
        for t in states[-1].U:
            t.fill_(float("nan"))
    copy_halos(states, 0)
    args = f32(op.oracle, p)
    for it in range(iters):
        if schedule == "ranges":  # the overlapped order: boundary planes, "exchange", interior
            for s in states:
                for zr in s.boundary_ranges()[0]:
                    s.step(it, *args, zr)
            copy_halos(states, it + 1)
            for s in states:
                s.step(it, *args, s.boundary_ranges()[1])
            continue
        for s in states:
            s.step(it, *args)
        copy_halos(states, it + 1)
    return host(torch.cat([s.local(s.source(iters)) for s in states]))


def check_slabs_equal_whole_volume(name, world, schedule, pname, shape=(19, 21, 90), iters=6):
    """`world` even slabs of the phantom, stitched, against the *_cupy run of the whole volume, and that against the oracle"""
    from tomobar_amd.slab import slab_bounds
    D = OPS[name].oracle
    vd = torch.from_numpy(phantom(shape)).cuda()
    want = host(cupy(name, vd, iters, pname))
    same_bits(want, D.cached(shape, pname, (iters,))[iters], "whole volume against the oracle")
    got = run_slabs(name, vd, [slab_bounds(shape[0], world, r) for r in range(world)], schedule, pname, iters)
    same_bits(got, want, (name, shape, world, schedule, pname))


# ------------------------------------------------------------------------------------------------ drivers
NZ, NN, NA = 6, 32, 48
ANGLES = np.linspace(0, np.pi, NA, endpoint=False)


def sino():
    return torch.from_numpy(np.random.default_rng(11).random((NZ, NA, NN)).astype(np.float32)).cuda()


def data():
    return {"projection_data": sino(), "data_axes_labels_order": ["detY", "angles", "detX"]}


def rt(os_number=None):
    from tomobar_amd.methodsIR_CuPy import RecToolsIRCuPy
    return RecToolsIRCuPy(NN, 0, NZ, 0.0, ANGLES, NN, 0, os_number)
