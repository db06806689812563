"""TEST INFRASTRUCTURE: numpy restatement of the nonlinear-diffusion (NDF) regulariser of docs/kernels/ndf.md (the
specification; there is no reference implementation to compare with -- formula-level parity, unpinned).  Shared by
tests/test_ndf_oracle.py, tests/test_ndf_slab_gloo.py (CPU) and tests/test_gpu_ndf.py (MI355X).

Arrays are indexed [z][y][x]; component 1 <-> x (the fastest axis), 2 <-> y, 3 <-> z; 2D drops component 3.  With
dtype = float32 every operation below is one float32 rounding in the order the parentheses give (numpy never contracts to
FMA, and its / is the correctly rounded division), which is what the kernel reproduces bit for bit; dtype = float64 is the
same algorithm in double."""
import functools

import numpy as np

from _tgv_oracle import phantom, rel_d, rel_l2  # noqa: F401  (the phantom and the two norms are shared with TGV)

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


def ndf_iterates(f, penalty, lam, sigma, tau, iterations=1, dtype=np.float32, stats=None):
    """yields U after every iteration (a fresh array each time); `stats`: see step, for the LAST iteration run"""
    t = dtype
    f = np.asarray(f).astype(t)
    assert f.ndim in (2, 3)
    lam, sigma, tau = t(lam), t(sigma), t(tau)
    U = f
    for n in range(iterations):
        U = step(U, f, lam, sigma, tau, penalty, stats if n == iterations - 1 else None)
        yield U


def ndf(f, penalty, lam, sigma, tau, iterations=1, dtype=np.float32, stats=None):
    """U after `iterations` iterations (a copy of the input, as `dtype`, for 0)"""
    out = np.asarray(f).astype(dtype)
    for out in ndf_iterates(f, penalty, lam, sigma, tau, iterations, dtype, stats):
        pass
    return out


def ndf_many(f, params, counts, dtype=np.float32):
    """{n: U after n iterations} for every n of `counts`, from ONE run"""
    counts = sorted(set(counts))
    out = {}
    for n, U in enumerate(ndf_iterates(f, iterations=counts[-1], dtype=dtype, **params), 1):
        if n in counts:
            out[n] = U
    return out


@functools.lru_cache(maxsize=None)
def cached(shape, pname, counts, dtype_name="float32"):
    """ndf_many of the phantom of `shape` under parameter set "A".."D": computed once per session, never modified"""
    res = ndf_many(phantom(shape), PARAMS[pname], counts, np.dtype(dtype_name).type)
    for v in res.values():
        v.setflags(write=False)
    return res


# ------------------------------------------------------------------------------------------------ z-slabs
def _as_numpy(t):
    return t.numpy() if hasattr(t, "numpy") else np.asarray(t)


def ndf_step_slab(inp, u_in, u_out, dx, dy, nzl, lo, hi, lam, sigma, tau, penalty, zr=None):
    """One iteration on ghosted slab arrays [lo + nzl + hi][dy][dx] (host torch tensors or numpy arrays), the step_fn of
    tomobar_amd.slab.ndf_slab: a ghost plane exists exactly where a z-neighbour exists, so the plain whole-array step on the
    ghosted array gives the right z differences on every LOCAL plane; only the local planes [z0, z1) of `u_out` are written.
    `penalty` is a name or its TOMO_NDF_* number."""
    z0, z1 = zr if zr is not None else (0, nzl)
    name = penalty if isinstance(penalty, str) else PENALTIES[int(penalty)]
    f, U, out = _as_numpy(inp), _as_numpy(u_in), _as_numpy(u_out)
    assert U.shape == (lo + nzl + hi, dy, dx) and U.dtype == np.float32
    a, b = max(lo + z0 - 1, 0), min(lo + z1 + 1, U.shape[0])    # the output planes and one plane either side
    new = step(U[a:b], f[a:b], np.float32(lam), np.float32(sigma), np.float32(tau), name)
    out[lo + z0:lo + z1] = new[lo + z0 - a:lo + z1 - a]


def ndf_by_slabs(f, params, iterations, world):
    """the whole volume run as `world` ghosted slabs exchanged by hand after every iteration, stitched"""
    f = np.asarray(f, np.float32)
    nz = f.shape[0]
    base, extra = divmod(nz, world)
    bounds, z = [], 0
    for r in range(world):
        bounds.append((z, z + base + (1 if r < extra else 0)))
        z = bounds[-1][1]
    U = f.copy()
    for _ in range(iterations):
        new = np.empty_like(U)
        for r, (z0, z1) in enumerate(bounds):
            lo, hi = int(r > 0), int(r < world - 1)
            g_in = np.ascontiguousarray(U[z0 - lo:z1 + hi])
            g_f = np.ascontiguousarray(f[z0 - lo:z1 + hi])
            g_out = np.full_like(g_in, np.nan)
            ndf_step_slab(g_f, g_in, g_out, f.shape[2], f.shape[1], z1 - z0, lo, hi, params["lam"], params["sigma"],
                          params["tau"], params["penalty"])
            new[z0:z1] = g_out[lo:lo + z1 - z0]
        U = new
    return U


# ------------------------------------------------------------------------------------------------ the tolerance rule
TOL_INTERVAL, TOL_MIN_SAVED = 6, 3
TOL_CASE = dict(shape=(7, 13, 37), pname="A", iterations=66, j=4)
TOL_CASE_SLAB = dict(shape=(9, 7, 11), pname="A", iterations=66, j=4)


def rel_change_sums(x, ref, keep=None):
    """CPU stand-in for tomo_rel_change at the slab driver's seam (tomobar_amd.slab._hip_rel_change): (sum (x - ref)^2,
    sum x^2) in float64 from the float32 values; with `keep`, keep[...] = x afterwards"""
    x64, r64 = _as_numpy(x).astype(np.float64).ravel(), _as_numpy(ref).astype(np.float64).ravel()
    num, den = float(np.sum((x64 - r64) ** 2)), float(np.sum(x64 ** 2))
    if keep is not None:
        keep.copy_(x.view(keep.shape))
    return num, den


@functools.lru_cache(maxsize=None)
def tolerance_plan(slab=False):
    """(tol, n the oracle's sequence stops after, the d it stops on, the whole sequence) of TOL_CASE (TOL_CASE_SLAB with
    `slab`): d_n compares iterate n with iterate n - 6 (iterate 0 = the input) after every 6th iteration that leaves at
    least 3; tol is the geometric mean of the (j-1)-th and j-th values, as tests/_tgv_oracle.py chooses its threshold"""
    c = TOL_CASE_SLAB if slab else TOL_CASE
    points = [n for n in range(TOL_INTERVAL, c["iterations"] + 1, TOL_INTERVAL) if c["iterations"] - n >= TOL_MIN_SAVED]
    its = cached(c["shape"], c["pname"], tuple(points))
    prev, seq = phantom(c["shape"]), []
    for n in points:
        seq.append(rel_d(its[n], prev))
        prev = its[n]
    j = c["j"]
    tol = float(np.sqrt(seq[j - 2] * seq[j - 1]))
    assert all(abs(v - tol) >= 0.01 * tol for v in seq), ("a value of the sequence is too close to the threshold", tol, seq)
    assert next(i for i, v in enumerate(seq, 1) if v < tol) == j, ("the target is not the first value below the threshold", seq)
    return tol, points[j - 1], seq[j - 1], tuple(seq)
