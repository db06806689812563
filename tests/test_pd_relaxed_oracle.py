"""CPU tests of the relaxed PD_TV model (oracle.pd_tv_relaxed / pd_step_relaxed) and of tests/_pd_relaxed.py, before any GPU
test relies on them: the model is a sane restatement of the reference, the envelope B is exactly zero where the model has no
hardware-dependent operation, the inputs the GPU tests call saturated / unsaturated are, the new check rejects what the
rel-L2 rule of `pd_arith` accepts, and deduce_offsets / replay recover a known offset pattern and refuse an unknown one."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _edge_shapes as E  # noqa: E402
import _pd_relaxed as R  # noqa: E402
import conftest  # noqa: E402
from oracle import tomo_oracle as O  # noqa: E402


def old_rule_accepts(got, want, what):
    """the rel-L2 assertion of `pd_arith` for the default arithmetic (its bit statistics are a log of GPU runs: not kept)"""
    n = len(conftest.PD_BITSTATS)
    conftest.PdArith("default").check(got, want, what=what)
    del conftest.PD_BITSTATS[n:]


def rel_l2(a, b):
    return float(np.linalg.norm(a.astype(np.float64).ravel() - b.astype(np.float64).ravel()) / np.linalg.norm(b.astype(np.float64).ravel()))


def _shares(x, p):
    _, c = R.model(x, p, counts=True)
    total = c["saturated"] + c["unsaturated"]
    return c["saturated"] / total, c["clipped"] / total


SAT_3D = sorted(set(R.STEP_SHAPES + R.CHAIN_SHAPES))


# ------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("shape,iters,mtv", [((20, 24, 40), 7, 0), ((20, 24, 40), 30, 0), ((12, 30, 70), 7, 1),
                                             ((40, 60, 100), 11, 0), ((24, 40), 7, 0)])
@pytest.mark.parametrize("nn", [0, 1])
def test_model_lies_within_1e_6_of_the_reference_roundings(shape, iters, mtv, nn):
    """a sanity bar on the model, not on any kernel (measured: 1.4-2.2e-7)"""
    x = (E.step_noise(shape) - np.float32(0.6 * nn)).astype(np.float32)
    m = R.model(x, R.params(R.LAM, iters, mtv, nn))
    want = O.pd_tv(x, R.LAM, iters, mtv, nn).reshape(m.shape)
    r = rel_l2(m, want)
    print(f"{shape} x{iters} mtv={mtv} nn={nn}: model vs reference rel-L2 {r:.3e}, max {R._dist(m, want) / np.abs(want).max():.3e} of max|want|")
    assert r < 1e-6


@pytest.mark.parametrize("shape", SAT_3D + [(9, 59), (3, 9, 59)])
def test_model_at_the_gpu_tests_inputs(shape):
    for kind in (R.mixed, R.quiet):
        for iters in R.ITERS:
            for nn in (0, 1):
                x = kind(shape)
                m = R.model(x, R.params(R.LAM, iters, 0, nn))
                want = O.pd_tv(x, R.LAM, iters, 0, nn)
                if want.shape != m.shape:   # pd_tv squeezes; none of these shapes has a singleton axis
                    want = want.reshape(m.shape)
                assert rel_l2(m, want) < 1e-6, (kind.__name__, shape, iters, nn)


def test_step_chain_equals_the_whole_run():
    """pd_step_relaxed chained = pd_tv_relaxed, bit for bit, under all-zero, all -1 and all +1 offsets"""
    shape = (6, 9, 13)
    x = R.mixed(shape)
    for nn in (0, 1):
        p = R.params(R.LAM, 5, 0, nn)
        for mode, off in (("model", 0), ("down", -1), ("up", 1)):
            U, P = x.copy(), [np.zeros_like(x) for _ in range(3)]
            for _ in range(p.iters):
                U, P, _ = O.pd_step_relaxed(x, U, P, *p.scal, 0, nn, offsets=np.full(shape, off, np.int8))
            assert np.array_equal(U, R._run(x, p, mode)), (nn, mode)
    # and the anisotropic step
    p = R.params(R.LAM, 3, 1, 1)
    U, P = x.copy(), [np.zeros_like(x) for _ in range(3)]
    for _ in range(3):
        U, P, sat = O.pd_step_relaxed(x, U, P, *p.scal, 1, 1)
        assert not sat.any()
    assert np.array_equal(U, R.model(x, p))


def test_slices_are_2d_runs():
    x = R.mixed((3, 9, 59))
    p = R.params(R.LAM, 4, 0, 1, slices=True)
    m = R.model(x, p)
    for k in range(3):
        assert np.array_equal(m[k], R.model(x[k], p._replace(slices=False)))
    assert not np.array_equal(m, R.model(x, p._replace(slices=False)))


# ------------------------------------------------------------------------------------------------ B = 0 where it must be
@pytest.mark.parametrize("shape", [(145, 9, 11), (4, 17, 121), (9, 59), (3, 9, 59), (1, 9, 11), (2, 2, 2)])
def test_anisotropic_family_is_one_point(shape):
    for x in (R.mixed(shape), E.step_noise(shape) - np.float32(0.6), E.terraces(shape, scale=0.25), R.quiet(shape)):
        x = x.astype(np.float32)
        for nn in (0, 1):
            for slices in ((False, True) if len(shape) == 3 else (False,)):
                p = R.params(R.LAM, 7, 1, nn, slices=slices)
                m, members = R.family(x, p)   # the members are RUN here, not short-cut
                assert all(np.array_equal(v.view(np.uint32), m.view(np.uint32)) for v in members)
                assert R.envelope(x, p) == 0.0


def _unsaturated_cases():
    out = []
    for name, L in E.LAUNCHES.items():
        if L.op == "PD_TV" and name != "pd_x2_exact":
            out += [c.shape for c in E.cases(name)]
    import _slicewise_cases as S
    return sorted(set(out)), sorted({s for s, _ in S.PD_CASES})


def test_unsaturated_inputs_never_leave_the_unit_ball():
    """`quiet` at every shape the bit-exact GPU tests run, 3D / 2D and slice-wise, the largest iteration count"""
    shapes, slice_shapes = _unsaturated_cases()
    for shape, slices in [(s, False) for s in shapes] + [(s, True) for s in slice_shapes]:
        x = R.quiet(shape)
        assert (x < 0).mean() > 0.3 or x.size < 16
        for nn in (0, 1):
            p = R.params(R.LAM, max(R.ITERS), 0, nn, slices=slices)
            _, c = R.model(x, p, counts=True)
            assert c["saturated"] == 0, (shape, slices, nn, c)
            assert R.envelope(x, p) == 0.0
    # not short-cut: the members equal the model
    x = R.quiet((4, 17, 121))
    m, members = R.family(x, R.params(R.LAM, 7, 0, 1))
    assert all(np.array_equal(v, m) for v in members)


# ------------------------------------------------------------------------------------------------ the saturated inputs
@pytest.mark.parametrize("nn", [0, 1])
def test_branch_shares_of_the_saturated_inputs(nn):
    cases = [(s, False) for s in SAT_3D + R.sat_2d_shapes()] + [(s, True) for s in R.sat_slice_shapes()]
    for shape, slices in cases:
        for iters in R.ITERS:
            sat, clip = _shares(R.mixed(shape), R.params(R.LAM, iters, 0, nn, slices=slices))
            assert 0.10 <= sat <= 0.90, (shape, slices, iters, sat)
            assert clip >= 0.01 if nn else clip == 0.0, (shape, slices, iters, clip)
    # and the states the one-step test starts from
    for shape in R.STEP_SHAPES:
        x = R.mixed(shape)
        p = R.params(R.LAM, 1, 0, nn)
        U, P = x.copy(), [np.zeros_like(x) for _ in range(3)]
        for i in range(5):
            Un, Pn, s = O.pd_step_relaxed(x, U, P, *p.scal, 0, nn)
            if i in (0, 4):
                assert 0.10 <= s.mean() <= 0.90, (shape, i, s.mean())
                assert not nn or (U < 0).mean() >= 0.01
            U, P = Un, Pn


def test_envelope_is_a_few_ulp():
    """B in ulp of max|model| where the family is not a point (the figures of docs/kernels/pd_tv.md)"""
    for shape, slices in [(s, False) for s in SAT_3D + [(9, 59), (9, 117)]] + [((3, 9, 59), True)]:
        x = R.mixed(shape)
        for iters in (1, 7):
            B, m = R.envelope(x, R.params(R.LAM, iters, 0, 1, slices=slices), with_model=True)
            print(f"{shape} slices={slices} x{iters}: B = {B / R.ulp_of_max(m):.1f} ulp of max|model|")
            assert 0 < B <= 16 * R.ulp_of_max(m)


# ------------------------------------------------------------------------------------------------ sensitivity
@pytest.mark.parametrize("mtv", [0, 1])
def test_one_voxel_off_passes_the_l2_rule_and_fails_the_new_check(mtv):
    shape = (23, 37, 150)
    x = R.mixed(shape)
    p = R.params(R.LAM, 7, mtv, 1)
    B, m = R.envelope(x, p, with_model=True)
    assert (B == 0.0) == bool(mtv)
    delta = 16 * B if B else 16 * R.ulp_of_max(m)
    want = O.pd_tv(x, R.LAM, 7, mtv, 1)
    at = (11, 18, 75)
    got = m.copy()
    got[at] += np.float32(delta)
    assert got[at] != m[at]
    old_rule_accepts(got, want, "sensitivity")
    R.check_elementwise(m, x, p)                                # the model itself passes
    with pytest.raises(AssertionError):
        R.check_elementwise(got, x, p)


def test_a_skipped_clip_fails_the_new_check():
    shape = (23, 37, 150)
    x = R.mixed(shape)
    p = R.params(R.LAM, 7, 0, 1)
    m = R.model(x, p)
    # a voxel whose iterate is slightly negative when iteration 3 starts
    U = R.model(x, p._replace(iters=3))
    neg = np.argwhere((U < -2e-4) & (U > -1e-3))
    at = tuple(neg[len(neg) // 2])
    wrong = R.model(x, p, fault=(int(np.ravel_multi_index(at, shape)), 3))
    assert not np.array_equal(wrong, m)
    # ... which the rel-L2 rule of `pd_arith` does not see
    old_rule_accepts(wrong, O.pd_tv(x, R.LAM, 7, 0, 1), "skipped clip")
    with pytest.raises(AssertionError):
        R.check_elementwise(wrong, x, p)


# ------------------------------------------------------------------------------------------------ deduce_offsets, replay
def _stand_in(p, seed, plus_two_at=None):
    """a "GPU" that is the model under a seeded offset pattern"""
    state = {"i": 0}

    def step(x, U, P):
        rng = np.random.default_rng([seed, state["i"]])
        offs = rng.integers(-1, 2, size=x.shape).astype(np.int8)
        if plus_two_at is not None and state["i"] == plus_two_at[0]:
            offs[plus_two_at[1]] = 2
        state.setdefault("offs", []).append(offs)
        state["i"] += 1
        u, pp, _ = O.pd_step_relaxed(x, U, P, *p.scal, 0, p.nonneg, offsets=offs)
        return u, pp
    return step, state


@pytest.mark.parametrize("nn", [0, 1])
def test_replay_recovers_a_seeded_pattern(nn):
    shape = (6, 17, 61)
    x = R.mixed(shape)
    p = R.params(R.LAM, 7, 0, nn)
    step, st = _stand_in(p, 17)
    t = R.replay(x, p, 7, step)
    assert len(t.states) == 8 and len(t.offsets) == 7
    U, P = x.copy(), [np.zeros_like(x) for _ in range(3)]
    mattered = 0
    for i in range(7):
        # the replayed state is the stand-in's, bit for bit
        U, P, sat = O.pd_step_relaxed(x, U, P, *p.scal, 0, nn, offsets=st["offs"][i])
        assert np.array_equal(U, t.states[i + 1][0]) and all(np.array_equal(a, b) for a, b in zip(P, t.states[i + 1][1]))
        assert np.array_equal(sat, t.saturated[i])
        assert not t.offsets[i][sat == 0].any()       # an unsaturated voxel gets 0
        # where the offset matters (the three candidates give three different triples) it is recovered
        cands = [O.pd_step_relaxed(x, t.states[i][0], t.states[i][1], *p.scal, 0, nn, offsets=np.full(shape, o, np.int8))[1]
                 for o in (-1, 0, 1)]
        differ = np.ones(shape, bool)
        for a, b in ((0, 1), (1, 2), (0, 2)):
            differ &= np.any([cands[a][c] != cands[b][c] for c in range(3)], axis=0)
        assert not (differ & (sat == 0)).any()
        assert np.array_equal(t.offsets[i][differ], st["offs"][i][differ])
        mattered += int(differ.sum())
    assert mattered > 0.05 * 7 * x.size
    h = R.offset_histogram(t)
    assert set(h) == {-1, 0, 1} and sum(h.values()) == sum(int(s.sum()) for s in t.saturated)


def test_an_offset_of_two_is_refused_where_it_was_made():
    shape = (6, 17, 61)
    x = R.mixed(shape)
    p = R.params(R.LAM, 3, 0, 1)
    # a voxel that saturates in step 1 and at which +2 gives bits that none of -1, 0, +1 gives
    U, P, _ = O.pd_step_relaxed(x, x, [np.zeros_like(x)] * 3, *p.scal, 0, 1)
    c = {o: O.pd_step_relaxed(x, U, P, *p.scal, 0, 1, offsets=np.full(shape, o, np.int8)) for o in (-1, 0, 1, 2)}
    odd = c[0][2] != 0
    for o in (-1, 0, 1):
        odd &= np.any([c[2][1][k] != c[o][1][k] for k in range(3)], axis=0)
    at = tuple(np.argwhere(odd)[len(np.argwhere(odd)) // 2])
    step, _ = _stand_in(p, 5, plus_two_at=(1, at))
    with pytest.raises(AssertionError) as err:
        R.replay(x, p, 3, step)
    assert tuple(int(i) for i in at) in err.value.args[0][2] and len(err.value.args[0][2]) == 1
    # the wider candidate set finds it
    step, _ = _stand_in(p, 5, plus_two_at=(1, at))
    t = R.replay(x, p, 3, step, width=2)
    assert t.offsets[1][at] == 2
