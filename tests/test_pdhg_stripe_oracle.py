"""No GPU: what the restatement of PDHG with the stripe variable (tests/_pdhg_stripe_oracle.py, the specification of
docs/kernels/pdhg.md) shows on the recorded inputs of tests/_pdhg_stripe_cases.py -- the steps are valid, the float32 form
holds the project's bar against the same algorithm in double, the joint objective falls, and the variable does what it is for:
it takes the planted offsets, all of them and nothing else, and the image is better for it."""
import functools

import numpy as np
import pytest

import _pdhg_cases as K
import _pdhg_diag_oracle as D
import _pdhg_oracle as P
import _pdhg_stripe_cases as SC
import _pdhg_stripe_oracle as S


# ------------------------------------------------------------------------------------------------ the two updates
def test_segment_sums_and_the_update_follow_the_specification():
    f = np.float32
    rng = np.random.default_rng(3)
    y = rng.standard_normal((2, 130, 5)).astype(f)
    part = S.segment_sums(y)
    assert part.shape == (3, 2, 5) and part.dtype == f and S.n_seg(130) == 3 and S.n_seg(64) == 1 and S.n_seg(65) == 2
    acc = f(0)
    for a in range(64, 128):
        acc = f(acc + y[1, a, 2])
    assert part[1, 1, 2] == acc and part[2, 0, 0] == f(f(0) + y[0, 128, 0]) + y[0, 129, 0]
    # the soft threshold as comparisons: +-theta itself is inside the dead zone, whose value is +0
    s = np.array([[1.0, -1.0, 0.25, 0.5, -0.5, 2.0]], f)
    sn, sbar = S.stripe_update(s, np.zeros((1, 1, 6), f), f(0.1), f(0.5))
    assert np.array_equal(sn, [[0.5, -0.5, 0.0, 0.0, 0.0, 1.5]]) and not np.signbit(sn[sn == 0]).any()
    assert np.array_equal(sbar, (sn + sn) - s)
    sn, _ = S.stripe_update(s, np.ones((2, 1, 6), f), f(0.25), f(0.5))      # c = 2, w = s - 0.5
    assert np.array_equal(sn, [[0.0, -1.0, 0.0, 0.0, -0.5, 1.0]])


def test_host_scalars_are_float32_and_follow_the_specification():
    f = np.float32
    L_A = K.lipschitz()
    assert S.lipschitz(L_A, 24, 3, "TV") == (f(L_A) + f(24)) + f(12) and S.lipschitz(L_A, 24, 2, "TGV") == (f(L_A) + f(24)) + f(12)
    assert S.lipschitz(L_A, 24, 3, "TGV") == (f(L_A) + f(24)) + f(16) and S.lipschitz(L_A, 24, 3, None) == f(L_A) + f(24)
    assert type(S.lipschitz(L_A, 24, 3, "TV")) is np.float32 and S.threshold(f(0.3), 3.0) == f(0.3) * f(3)
    sigma, tau, tau_s = S.diag_stripe_steps(K.matched(), (K.NZ, K.NA, K.NU), (K.NZ, K.N, K.N), 3, True, 4.0)
    a, t, _, w = D.host_scalars(3, True, 4.0)
    R = K.matched().fp(np.ones((K.NZ, K.N, K.N), f))
    assert sigma.dtype == tau.dtype == f and type(tau_s) is f and tau_s == t / f(K.NA)
    assert np.array_equal(sigma, a / (R + f(1))) and (R + f(1) >= 1).all()          # the guard never acts: a row of [A S] sums to >= 1


# ------------------------------------------------------------------------------------------------ step validity
def _dense_K(tv=True):
    A = K.dense().A
    return S.joint_matrix(A, K.NA, K.NU, (1, K.N, K.N), tv)


@pytest.mark.parametrize("tv", [True, False], ids=["TV", "no TV"])
def test_scalar_steps_satisfy_sigma_tau_norm_below_one(tv):
    """sigma tau |K|^2 < 1 for the dense K = [[A, S], [grad, 0]] of the 32 x 32 2D case, and the bound L_A + na (+ 4 nd) holds"""
    norm2 = float(np.linalg.norm(_dense_K(tv), 2) ** 2)
    L_K = S.lipschitz(K.lipschitz(), K.NA, 2, "TV" if tv else None, np.float64)
    sigma, tau = P.scalars(None, 2, dtype=np.float64, L_K=L_K)
    print(f"PDHG stripe, TV {tv}: |K|^2 = {norm2:.3f}, bound L_K = {L_K:.3f}, sigma tau |K|^2 = {sigma * tau * norm2:.4f}")
    assert norm2 <= L_K and sigma * tau * norm2 < 1.0


@pytest.mark.parametrize("tv", [True, False], ids=["TV", "no TV"])
@pytest.mark.parametrize("ratio", [1.0, 4.0])
def test_diagonal_steps_satisfy_the_sum_condition_and_the_norm_bound(ratio, tv):
    """Pock and Chambolle 2011, lemma 2 with alpha = 1: sigma_i sum_j |K_ij| <= a for every row, tau_j sum_i |K_ij| <= t for every
    column, hence |Sigma^(1/2) K T^(1/2)|^2 <= a t = 0.9025; both asserted on the dense K"""
    shape, sino_shape = (1, K.N, K.N), (1, K.NA, K.NU)
    Kd = _dense_K(tv)
    sigma, tau, tau_s = S.diag_stripe_steps(K.dense(), sino_shape, shape, 2, tv, ratio, np.float64)
    a, t, sigma_G, _ = D.host_scalars(2, tv, ratio, np.float64)
    row_steps = np.concatenate([sigma.ravel()] + ([np.full(Kd.shape[0] - sigma.size, sigma_G)] if tv else []))
    col_steps = np.concatenate([tau.ravel(), np.full(K.NU, tau_s)])
    assert row_steps.size == Kd.shape[0] and col_steps.size == Kd.shape[1]
    rows, cols = row_steps * np.abs(Kd).sum(axis=1), col_steps * np.abs(Kd).sum(axis=0)
    assert (rows <= a * (1 + 1e-12)).all() and (cols <= t * (1 + 1e-12)).all(), (rows.max() / a, cols.max() / t)
    M = np.sqrt(row_steps)[:, None] * Kd * np.sqrt(col_steps)[None, :]
    norm2 = float(np.linalg.norm(M, 2) ** 2)
    print(f"PDHG stripe diagonal steps, ratio {ratio}, TV {tv}: |Sigma^1/2 K T^1/2|^2 = {norm2:.6f}")
    assert norm2 <= 0.9025 * (1 + 1e-9), norm2


# ------------------------------------------------------------------------------------------------ float32 against float64
@pytest.mark.parametrize("name", list(SC.CASES))
def test_float32_against_float64(name):
    """the float32 arithmetic the kernels reproduce holds the project's parity bar against the same algorithm in double, for
    the image and for the pair (x, s) (the values seen are recorded in docs/kernels/pdhg.md)"""
    f32, f64 = SC.run(name, "float32", K.COUNTS), SC.run(name, "float64", K.COUNTS)
    for n in K.COUNTS:
        (x32, s32), (x64, s64) = f32[n], f64[n]
        assert x32.dtype == s32.dtype == np.float32 and x64.dtype == s64.dtype == np.float64
        assert x32.shape == (K.NZ, K.N, K.N) and s32.shape == (K.NZ, K.NU)
        rx = P.rel_l2(x32, x64)
        rj = P.rel_l2(np.concatenate([x32.ravel(), s32.ravel()]), np.concatenate([x64.ravel(), s64.ravel()]))
        print(f"PDHG stripe {name} after {n}: float32 vs float64 rel-L2 = {rx:.2e} (x), {rj:.2e} (x and s); max|s| = {np.abs(s64).max():.3f}")
        assert rx <= 1e-5 and rj <= 1e-5, (name, n, rx, rj)
    assert np.abs(f64[K.COUNTS[-1]][1]).max() > 0, "the stripe variable never moved"


# ------------------------------------------------------------------------------------------------ the joint objective
@functools.lru_cache(maxsize=None)
def _objectives(name):
    kw, positive = SC.CASES[name]
    b = SC.sinogram(positive=positive)
    state, out = {}, []
    its = S.pdhg_stripe_iterates(K.dense(), b, K.lipschitz(), iterations=K.CHECKPOINTS[-1], dtype=np.float64, state=state, **kw)
    for n, x in enumerate(its, 1):
        if n in K.CHECKPOINTS:
            out.append(S.objective(K.dense(), x, state["s"], b, kw["mu"], kw["fidelity"], kw["regulariser"], kw["lam"],
                                   v=state.get("v"), alpha1=kw.get("alpha1", 1.0), alpha0=kw.get("alpha0", 2.0)))
    return out


@pytest.mark.parametrize("name", list(SC.CASES))
def test_joint_objective_falls(name):
    at = _objectives(name)
    print(f"PDHG stripe {name}: F(Ax + Ss) + lambda R + mu |s|_1 at {K.CHECKPOINTS} = {['%.8g' % v for v in at]}")
    assert all(np.isfinite(at)) and all(later < earlier for earlier, later in zip(at, at[1:])), at


# ------------------------------------------------------------------------------------------------ the striped case
def test_the_variable_takes_the_planted_offsets_and_the_image_is_better_for_it():
    """conditions on the float64 oracle, on recorded inputs: with the variable the error lies below the least error of the
    lambda grid without it; {|s| > half the smallest planted amplitude} is the planted set; on the sinogram without offsets
    no |s| reaches that half"""
    res = SC.stripe_errors()
    err, s, plain = res["striped"]
    best = min(plain.values())
    print(f"PDHG stripe, striped sinogram: error with s {err:.4f}; LS + TV alone " + ", ".join(f"{v:.4f}" for v in plain.values())
          + f" for lambda = {SC.PLAIN_LAMBDAS}; ratio to the best {err / best:.3f}")
    assert err < best, (err, plain)
    assert tuple(np.flatnonzero(np.abs(s[0]) > SC.STRIPE_HALF)) == SC.STRIPE_COLUMNS, s
    assert all(np.sign(s[0, c]) == np.sign(v) for c, v in zip(SC.STRIPE_COLUMNS, SC.STRIPE_OFFSETS))
    err0, s0, plain0 = res["clean"]
    print(f"PDHG stripe, sinogram without offsets: error with s {err0:.4f}, max|s| = {np.abs(s0).max():.4f}; LS + TV alone at "
          f"lambda = {SC.STRIPE_LAMBDA}: {plain0[SC.STRIPE_LAMBDA]:.4f}")
    assert np.abs(s0).max() < SC.STRIPE_HALF
