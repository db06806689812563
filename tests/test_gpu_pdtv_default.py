"""The shipped float32 PD_TV (relaxed arithmetic, variant 0: the kernel bench.py times) element for element on the MI355X,
against the relaxed model of the oracle (oracle.pd_tv_relaxed; tests/_pd_relaxed.py says what the three tiers are and
tests/test_pd_relaxed_oracle.py proves the helper and the inputs on the CPU):

  * anisotropic TV, and isotropic TV on inputs whose duals never leave the unit ball: the model has no hardware-dependent
    operation, so every family -- tomo_pdtv in 3D (pd_zmarch_xk FIRST and steady, pd_zmarch_x2 at 2 x 4 waves, pd_zmarch2) and
    in 2D (pd_rows2d at k = 3, 2, 1), and tomo_pdtv_slices -- must equal it BIT FOR BIT at the edge shapes of
    tests/_edge_shapes.py, with 1, 2, 3, 5, 6 and 7 iterations (tests/_pd_relaxed.py: ITERS) and both settings of nonneg;
  * isotropic TV where duals saturate, 3D: one explicit step (tomo_pdtv_iter_slab) is replayed with the reciprocal square
    roots the hardware itself used (read back from the duals it returned) and must then equal the model bit for bit; chained,
    that is an exact trajectory which tomo_pdtv and the fused launches of tomo_pdtv_multi_slab_range must reproduce bit for bit;
  * isotropic TV where duals saturate, 2D and slice-wise (no explicit-state entry point): within 4 B of the model, B the
    envelope of the family of offset patterns, computed from the model alone."""
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
import _slicewise_cases as S  # noqa: E402
from _guarded import guarded  # noqa: E402
from _march_gpu import same_bits  # noqa: E402
from oracle import tomo_oracle as O  # noqa: E402

# every relaxed launch of a whole-volume prox and the groups of its edge shapes
FAMILIES = [(name, g) for name, L in E.LAUNCHES.items() if L.op == "PD_TV" and name != "pd_x2_exact" for g in E.groups_of(name)]
SLICE_SHAPES = sorted({s for s, _ in S.PD_CASES})


def _default():
    from tomobar_amd import ops
    ops.set_variant("pdtv", 0)   # the autouse fixture only resets afterwards
    assert ops.get_variant("pdtv") == 0
    return ops


def _prox(x, p):
    """the shipped prox on the GPU, input and output inside guard bands"""
    ops = _default()
    if p.slices:
        return G.run_op(lambda a, out: ops.pdtv_slices(a, out, *p.scal, p.iters, p.methodTV, p.nonneg, False), x)[0]
    return G.run_op(lambda a, out: ops.pdtv(a, out, *p.scal, p.iters, p.methodTV, p.nonneg, False), x)[0]


def _bit_for_bit(make, shapes, mtv, slices=False):
    n = 0
    for shape in shapes:
        x = make(shape)
        assert (x < 0).any(), shape   # nonneg = 0 runs the clipping instantiation with a threshold of -inf
        for nn in (0, 1):
            for iters in R.ITERS:
                p = R.Params(O.pd_scalars(R.LAM, 8.0), iters, mtv, nn, slices)
                want, c = R.model(x, p, counts=True)
                assert mtv or c["saturated"] == 0, (shape, p)
                same_bits(_prox(x, p), want, (shape, f"x{iters} methodTV={mtv} nonneg={nn} slices={slices}"))
                n += 1
    return n


# ------------------------------------------------------------------------------------------------ tier 1: bit for bit
@pytest.mark.parametrize("launch,group", FAMILIES)
def test_anisotropic_equals_the_relaxed_model_bit_for_bit(launch, group):
    """on `mixed`: most anisotropic duals are clamped, about half the iterates clipped"""
    _bit_for_bit(R.mixed, [c.shape for c in E.cases(launch, group)], 1)


@pytest.mark.parametrize("launch,group", FAMILIES)
def test_isotropic_unsaturated_equals_the_relaxed_model_bit_for_bit(launch, group):
    _bit_for_bit(R.quiet, [c.shape for c in E.cases(launch, group)], 0)


@pytest.mark.parametrize("mtv", [1, 0], ids=["anisotropic", "unsaturated"])
def test_slicewise_equals_the_relaxed_model_bit_for_bit(mtv):
    _bit_for_bit(R.mixed if mtv else R.quiet, SLICE_SHAPES, mtv, slices=True)


# ------------------------------------------------------------------------------------------------ tier 2: one step, exactly
def _gpu_step(p, k=1):
    """step_fn of R.replay: k iterations in one launch on explicit (U, P) with no ghost planes -- tomo_pdtv_iter_slab
    (k = 1) or tomo_pdtv_multi_slab_range over [0, nz) (k = 2, 3) --, guard bands round all nine arrays"""
    def step(x, U, P):
        from tomobar_amd import slab
        _default()
        nz, dy, dx = x.shape
        ins = [guarded(a) for a in (x, U, *P)]
        outs = [guarded(x.shape) for _ in range(4)]
        gi, gu, gp = ins[0].view, ins[1].view, [g.view for g in ins[2:]]
        go, gq = outs[0].view, [g.view for g in outs[1:]]
        if k == 1:
            slab._hip_pd_step(gi, gu, go, gp, gq, dx, dy, nz, 0, 0, *p.scal, p.methodTV, p.nonneg, False)
        else:
            slab._hip_pd_pair(gi, gu, go, gp, gq, dx, dy, nz, 0, 0, *p.scal, p.methodTV, p.nonneg, False, zr=(0, nz), k=k)
        torch.cuda.synchronize()
        for i, g in enumerate(ins):
            g.check(("input array", i, x.shape), read_only=True)
        for i, g in enumerate(outs):
            g.check(("output array", i, x.shape))
        return outs[0].host(), [g.host() for g in outs[1:]]
    return step


def _params(nn, iters=1):
    return R.Params(O.pd_scalars(R.LAM, 8.0), iters, 0, nn, False)


@pytest.mark.parametrize("nn", [0, 1])
@pytest.mark.parametrize("start", ["first step", "after four iterations"])
@pytest.mark.parametrize("shape", R.STEP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_one_saturated_step_equals_the_model_under_the_hardwares_offsets(shape, start, nn):
    x = R.mixed(shape)
    p = _params(nn)
    U, P = x.copy(), [np.zeros_like(x) for _ in range(3)]
    if start != "first step":
        for _ in range(4):
            U, P, _ = O.pd_step_relaxed(x, U, P, *p.scal, 0, nn)
    t = R.replay(x, p, 1, _gpu_step(p), state=(U, P), what=(shape, start, nn))   # raises unless every voxel has a candidate
    share = float(t.saturated[0].mean())
    assert 0.10 <= share <= 0.90, share
    print(f"one step {shape} {start} nonneg={nn}: {share:.3f} saturated, offsets {R.offset_histogram(t)}")


# ------------------------------------------------------------------------------------------------ tier 2: the chain
@functools.lru_cache(maxsize=None)
def _trajectory(shape, nn):
    x = R.mixed(shape)
    x.setflags(write=False)
    p = _params(nn)
    return x, R.replay(x, p, max(R.CHAIN_COUNTS), _gpu_step(p), what=("chain", shape, nn))


def _same_state(got, want, what):
    same_bits(got[0], want[0], (what, "U"))
    for c in range(3):
        same_bits(got[1][c], want[1][c], (what, "P", c))


@pytest.mark.parametrize("nn", [0, 1])
@pytest.mark.parametrize("shape", R.CHAIN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_prox_and_fused_launches_reproduce_the_replayed_trajectory(shape, nn):
    x, t = _trajectory(shape, nn)
    # the whole prox: 7 = 3 (FIRST) + 2 + 2, 5 = 3 + 2, and the other plans (6 = 3 + 3: the steady K = 3 form), whose trajectory
    # is a prefix of the same one
    for n in sorted(set(R.CHAIN_COUNTS) | set(R.ITERS)):
        same_bits(_prox(x, _params(nn, n)), t.states[n][0], (shape, nn, f"tomo_pdtv x{n}"))
    # the same trajectory in fused launches on explicit state: 3 + 2 + 2 and 3 + 2 from the start, 2 + 3 after the first step
    p = _params(nn)
    for at, plan in ((0, (3, 2, 2)), (0, (3, 2)), (1, (2, 3))):
        state = t.states[at]
        for k in plan:
            state = _gpu_step(p, k)(x, *state)
            at += k
            _same_state(state, t.states[at], (shape, nn, f"fused k={k} up to step {at}"))


def test_offset_history_of_v_rsq_f32():
    """the share of -1 / 0 / +1 ulp (relative to RN(1 / sqrt(x)) formed in double) over all saturated voxel-steps of the
    chains: the first measurement of this instruction's accuracy in the project"""
    hist = R.offset_histogram([_trajectory(s, nn)[1] for s in R.CHAIN_SHAPES for nn in (0, 1)])
    total = sum(hist.values())
    assert total > 0 and set(hist) <= set(range(-R.WIDTH, R.WIDTH + 1))
    print("v_rsq_f32 against RN(1/sqrt(x)), %d saturated voxel-steps: %s"
          % (total, ", ".join(f"{o:+d} ulp {100.0 * hist.get(o, 0) / total:.2f} %" for o in sorted(hist))))


# ------------------------------------------------------------------------------------------------ tier 3: the envelope
def _within_envelope(shapes, slices):
    mark = len(R.STATS)
    for shape in shapes:
        x = R.mixed(shape)
        for nn in (0, 1):
            for iters in R.ITERS:
                p = R.Params(O.pd_scalars(R.LAM, 8.0), iters, 0, nn, slices)
                R.check_elementwise(_prox(x, p), x, p, what=f"{shape} x{iters} nonneg={nn} slices={slices}")
    print(R.summary(mark, "slice-wise" if slices else "2D"))


def test_isotropic_saturated_2d_lies_within_the_envelope():
    _within_envelope(R.sat_2d_shapes(), False)


def test_isotropic_saturated_slicewise_lies_within_the_envelope():
    _within_envelope(R.sat_slice_shapes(), True)
