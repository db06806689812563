"""MI355X tests of the z-march regularisers (NDF, Diff4th, TGV, ROF_TV, PD_TV) at the shapes of tests/_edge_shapes.py: the
array ends on, one before and one past the last emitting lane of a wave / the last column of a workgroup, the same in rows,
the z-chunk count changes, and a slab launch with ghost planes is z-chunked -- on noise and on the `terraces` / `scaled`
inputs that reach the zero-difference branches and the small / large operand range of the FMA-corrected sqrt and
reciprocal.  One test id is one group of about six tiny shapes.  NDF, Diff4th, TGV and ROF_TV: bit equality with their
oracles.  PD_TV: through `pd_arith` (variant 22 and binary16 duals: bit equality; the shipped float32 default: 1e-5
relative L2).  tests/test_edge_shapes.py proves on the CPU that the shapes have the properties they are here for."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _edge_shapes as E  # noqa: E402
import _march_gpu as G  # noqa: E402
import _pd_relaxed as R  # noqa: E402
import _tgv_oracle as T  # noqa: E402
from _march_gpu import same_bits  # noqa: E402

COUNTS = (1, 2, 5)   # the direct input-to-output launch and both parities of the ping-pong


def _run(call, f_host):
    """call(input tensor, NaN-filled output tensor) on the GPU; the input's bits are checked afterwards"""
    return G.run_op(call, f_host)[0]


# ------------------------------------------------------------------------------------------------ NDF, Diff4th, TGV
def _field(kind, shape):
    return T.phantom(shape) if kind == "phantom" else E.terraces(shape)


TGV_PARAMS = {"A": T.PARAMS_A, "B": T.PARAMS_B}
MARCHERS = {"ndf": "NDF", "diff4th": "Diff4th"}   # the launch names of tests/_edge_shapes.py -> the operators of _march_gpu.OPS


@functools.lru_cache(maxsize=None)
def _want(op, kind, shape, pname):
    """{n: the float32 numpy oracle after n iterations}, computed once per session and never modified"""
    f = _field(kind, shape)
    if op in MARCHERS:
        D = G.OPS[MARCHERS[op]].oracle
        res = D.many(f, D.PARAMS[pname], COUNTS)
    else:
        res = T.tgv_many(f, TGV_PARAMS[pname], COUNTS)
    for v in res.values():
        v.setflags(write=False)
    return res


def _gpu(op, pname, n):
    from tomobar_amd import ops
    if op in MARCHERS:
        D = G.OPS[MARCHERS[op]].oracle
        p = D.PARAMS[pname]
        return lambda x, out: G.ops_fn(D.name)(x, out, *G.f32(D, p), *(p[k] for k in D.extra), n)
    p = TGV_PARAMS[pname]
    return lambda x, out: ops.tgv(x, out, *T.scalars(p["lam"], p["alpha1"], p["alpha0"], p["L"]), n)


MARCH_OPS = [(op, g, p) for op, params in (("ndf", G.OPS["NDF"].oracle.PARAMS), ("diff4th", G.OPS["Diff4th"].oracle.PARAMS),
                                           ("tgv", TGV_PARAMS))
             for g in E.groups_of(op) for p in sorted(params)]


@pytest.mark.parametrize("kind", ["phantom", "terraces"])
@pytest.mark.parametrize("op,group,pname", MARCH_OPS)
def test_march_edges_equal_the_oracle(op, group, pname, kind):
    """every 2D and 3D edge shape of the group, after 1, 2 and 5 iterations, bit for bit"""
    for case in E.cases(op, group):
        f = _field(kind, case.shape)
        want = _want(op, kind, case.shape, pname)
        for n in COUNTS:
            same_bits(_run(_gpu(op, pname, n), f), want[n], (op, case, kind, pname, n))


# ------------------------------------------------------------------------------------------------ ROF_TV, PD_TV
TV_KINDS = ["noise", "terraces", "scaled"]


def _tv_inputs(kind, shape, shifted=False):
    """[(label, input)]: the noise-on-a-step input of test_pdtv_vs_oracle (shifted by -0.6 where the non-negativity clip is
    tested, as there), terraces(scale = 0.25), or that noise input times 2**-14 and 2**10"""
    if kind == "terraces":
        return [("terraces", E.terraces(shape, scale=0.25))]
    x = E.step_noise(shape, seed=5)
    x = (x - 0.6).astype(np.float32) if shifted else x
    if kind == "noise":
        return [("noise", x)]
    return [(f"noise*2^{e}", E.scaled(x, e)) for e in E.SCALE_EXPONENTS]


def _dims(x):
    return (x.shape[1], x.shape[0], 1, 2) if x.ndim == 2 else (x.shape[2], x.shape[1], x.shape[0], 3)


def _fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _oracle_rof(O, x, lam, tau, iters, half):
    """orc_roftv on the array as it is (a 3D shape is never squeezed)"""
    want = np.empty_like(x)
    assert O.lib().orc_roftv(_fptr(x), _fptr(want), *_dims(x), np.float32(lam), np.float32(tau), iters, int(half)) == 0
    return want


def _oracle_pd(O, x, scal, iters, mtv, nn, half):
    want = np.empty_like(x)
    assert O.lib().orc_pdtv(_fptr(x), _fptr(want), *_dims(x), *scal, iters, mtv, nn, int(half)) == 0
    return want


@pytest.mark.parametrize("kind", TV_KINDS)
@pytest.mark.parametrize("group", E.groups_of("rof"))
def test_roftv_edges_equal_the_oracle(oracle, group, kind):
    """the parameters of test_roftv_vs_oracle, both D types, 1 and 6 iterations, bit for bit"""
    from tomobar_amd import ops
    for case in E.cases("rof", group):
        for label, x in _tv_inputs(kind, case.shape):
            for half in (False, True):
                for iters in (1, 6):
                    want = _oracle_rof(oracle, x, 0.05, 0.005, iters, half)
                    got = _run(lambda a, out: ops.roftv(a, out, np.float32(0.05), np.float32(0.005), iters, half), x)
                    same_bits(got, want, (case, label, half, iters))


# (the two K = 2 workgroup shapes differ in rows only: their x and z shapes are run once)
PD_GROUPS, _seen = [], set()
for _name, _L in E.LAUNCHES.items():
    for _g in E.groups_of(_name) if _L.op == "PD_TV" else ():
        _shapes = tuple(k.shape for k in E.cases(_name, _g))
        if _shapes not in _seen:
            _seen.add(_shapes)
            PD_GROUPS.append((_name, _g))


@pytest.mark.parametrize("kind", TV_KINDS)
@pytest.mark.parametrize("launch,group", PD_GROUPS)
def test_pdtv_edges(oracle, pd_arith, launch, group, kind):
    """the parameters of test_pdtv_vs_oracle; 7 iterations = 3 + 2 + 2 reach the K = 3 and K = 2 marches, 1 the single-iteration
    march (2D: pd_rows2d at k = 3, 2 and 1); both dual types, both TV norms, with and without the non-negativity clip"""
    from tomobar_amd import ops
    scal = oracle.pd_scalars(0.04, 8.0)
    mark = len(R.STATS)
    for case in E.cases(launch, group):
        for nn in (0, 1):
            for label, x in _tv_inputs(kind, case.shape, shifted=bool(nn)):
                for half in (False, True):
                    for mtv in (0, 1):
                        for iters in (1, 7):
                            want = _oracle_pd(oracle, x, scal, iters, mtv, nn, half)
                            got = _run(lambda a, out: ops.pdtv(a, out, *scal, iters, mtv, nn, half), x)
                            pd_arith.check(got, want, half=half,
                                           what=f"{launch} {group} {case.shape} {label} x{iters} half={int(half)} mtv={mtv} nn={nn}")
                            if not (pd_arith.exact or half):   # the shipped default, element for element (tests/_pd_relaxed.py)
                                R.check_elementwise(got, x, R.Params(scal, iters, mtv, nn),
                                                    what=f"{launch} {group} {case.shape} {label} x{iters} mtv={mtv} nn={nn}")
    if not pd_arith.exact:
        print(R.summary(mark, f"{launch} {group} {kind}"))


# ------------------------------------------------------------------------------------------------ chunked z-slabs
# The whole-volume-equals-slabs comparisons of test_gpu_ndf / test_gpu_diff4th / test_gpu_slab at 2 m + 1 local planes per
# rank: every slab launch is z-chunked (three chunks over all local planes, the first starting at the ghost planes; the
# interior launch of the "ranges" schedule starts past the boundary planes and is still chunked).  The z-edge shapes above
# hold the whole-volume run to the oracle.
def _chunked(op, schedule):
    s = E.SLABS[op]
    for sizes in E.slab_launch_chunks(op, schedule):
        assert len(sizes) >= (3 if schedule == "plain" else 2), (op, schedule, sizes)
    return s


@pytest.mark.parametrize("schedule", ["plain", "ranges"])
@pytest.mark.parametrize("penalty", ["Huber", "PM", "Tukey"])
def test_ndf_chunked_slabs_equal_whole_volume(schedule, penalty):
    s = _chunked("NDF", schedule)
    G.check_slabs_equal_whole_volume("NDF", s.world, schedule, {"Huber": "A", "PM": "B", "Tukey": "C"}[penalty], shape=s.shape)


@pytest.mark.parametrize("schedule", ["plain", "ranges"])
def test_diff4th_chunked_slabs_equal_whole_volume(schedule):
    s = _chunked("Diff4th", schedule)
    G.check_slabs_equal_whole_volume("Diff4th", s.world, schedule, "A", shape=s.shape)


@pytest.mark.parametrize("half", [False, True])
def test_roftv_chunked_slabs_equal_whole_volume(half):
    """(run_roftv_slabs alternates the two schedules: even iterations over all local planes, odd ones in ranges)"""
    import test_gpu_slab as G
    _chunked("ROF_TV", "plain")
    s = _chunked("ROF_TV", "ranges")
    G.run_roftv_slabs(s.world, half, shape=s.shape)


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("variant", [0, 22, "ranges"])
def test_pdtv_chunked_slabs_equal_whole_volume(variant, half):
    """(variant "ranges": the shipped default in the overlapped schedule, as in test_pdtv_slabs_equal_whole_volume)"""
    import test_gpu_slab as G
    s = _chunked("PD_TV", "ranges" if variant == "ranges" else "plain")
    G.run_pdtv_slabs(s.world, half, variant, shape=s.shape)
