"""TEST INFRASTRUCTURE: numpy restatement of the nonlinear-diffusion (NDF) regulariser of docs/kernels/ndf.md (the
specification; there is no reference implementation to compare with -- formula-level parity, unpinned).  This file holds
the formula; tests/_march_oracle.py runs it (ORACLE below).  Shared by tests/test_ndf_oracle.py,
tests/test_ndf_slab_gloo.py (CPU) and tests/test_gpu_ndf.py (MI355X).

Arrays are indexed [z][y][x]; component 1 <-> x (the fastest axis), 2 <-> y, 3 <-> z; 2D drops component 3.  With
dtype = float32 every operation below is one float32 rounding in the order the parentheses give (numpy never contracts to
FMA, and its / is the correctly rounded division), which is what the kernel reproduces bit for bit; dtype = float64 is the
same algorithm in double."""
import numpy as np

import _march_oracle

GHOST = 1   # ghost planes of U per interior boundary of a z-slab
PENALTIES = ("Huber", "PM", "Tukey")
PARAMS = {
    "A": dict(penalty="Huber", lam=1.0, sigma=2.0, tau=0.05),
    "B": dict(penalty="PM", lam=1.0, sigma=2.0, tau=0.05),
    "C": dict(penalty="Tukey", lam=1.0, sigma=4.0, tau=0.05),
    "D": dict(penalty="Huber", lam=3.0, sigma=0.5, tau=0.02),
}


def flux(t, sigma, penalty):
    """g(t), element-wise, in t's dtype"""
    one = t.dtype.type(1.0)
    inside = np.abs(t) <= sigma
    with np.errstate(over="ignore", invalid="ignore"):
        if penalty == "Huber":
            return np.where(inside, t / sigma, np.copysign(one, t))
        if penalty == "PM":
            r = t / sigma
            return t / (one + r * r)
        if penalty == "Tukey":
            r = t / sigma
            w = one - r * r
            return np.where(inside, t * (w * w), t.dtype.type(0.0))
    raise ValueError(f"unknown NDF penalty {penalty!r}")


def _dp(U, ax):
    """U[i + e] - U[i] where the neighbour exists, exactly 0 on the last index"""
    out = np.zeros_like(U)
    n = U.shape[ax]
    hi, lo = [slice(None)] * U.ndim, [slice(None)] * U.ndim
    hi[ax], lo[ax] = slice(1, n), slice(0, n - 1)
    out[tuple(lo)] = U[tuple(hi)] - U[tuple(lo)]
    return out


def _dm(U, ax):
    """U[i - e] - U[i] where the neighbour exists, exactly 0 on the first index"""
    out = np.zeros_like(U)
    n = U.shape[ax]
    hi, lo = [slice(None)] * U.ndim, [slice(None)] * U.ndim
    hi[ax], lo[ax] = slice(1, n), slice(0, n - 1)
    out[tuple(hi)] = U[tuple(lo)] - U[tuple(hi)]
    return out


def step(U, f, lam, sigma, tau, penalty, stats=None):
    """one iteration: U' = U + tau (lam S - (U - f)), S summed in the order x+, x-, y+, y-, z+, z-.  `stats` (a dict)
    receives stats["above"]: the share of forward differences (neighbour present) whose magnitude exceeds sigma, and
    stats["zero"]: the share that is exactly zero (the `t == 0` rule of the turned flux)."""
    nd = U.ndim
    S = None
    above = zero = total = 0
    for d in range(1, nd + 1):
        ax = nd - d
        dp = _dp(U, ax)
        if stats is not None and U.shape[ax] > 1:
            sl = [slice(None)] * nd
            sl[ax] = slice(0, U.shape[ax] - 1)
            above += int(np.count_nonzero(np.abs(dp[tuple(sl)]) > sigma))
            zero += int(np.count_nonzero(dp[tuple(sl)] == 0))
            total += dp[tuple(sl)].size
        gp = flux(dp, sigma, penalty)
        S = gp if S is None else S + gp
        S = S + flux(_dm(U, ax), sigma, penalty)
    if stats is not None:
        stats["above"] = above / max(total, 1)
        stats["zero"] = zero / max(total, 1)
    return U + tau * (lam * S - (U - f))


def _step_slab(inp, u_in, u_out, dx, dy, nzl, lo, hi, lam, sigma, tau, penalty, zr=None, ghost=GHOST):
    """the step_fn of tomobar_amd.slab.ndf_slab (_march_oracle.slab_step): `penalty` is a name or its TOMO_NDF_* number"""
    name = penalty if isinstance(penalty, str) else PENALTIES[int(penalty)]
    _march_oracle.slab_step(step, inp, u_in, u_out, dx, dy, nzl, lo, hi, (lam, sigma, tau), zr, ghost, penalty=name)


TOL_CASE = dict(shape=(7, 13, 37), pname="A", iterations=66, j=4)
TOL_CASE_SLAB = dict(shape=(9, 7, 11), pname="A", iterations=66, j=4)
# `stats`: step's figures of the LAST iteration run
ORACLE = _march_oracle.Marcher("NDF", step, PARAMS, ("lam", "sigma", "tau"), GHOST, TOL_CASE, TOL_CASE_SLAB, stats_each=False,
                               step_slab=_step_slab)
