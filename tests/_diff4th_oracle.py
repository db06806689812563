"""TEST INFRASTRUCTURE: numpy restatement of the Diff4th regulariser (anisotropic fourth-order diffusion, explicit in time) of
docs/kernels/diff4th.md (the specification; there is no reference implementation to compare with -- formula-level parity,
unpinned).  Shared by tests/test_diff4th_oracle.py, tests/test_diff4th_slab_gloo.py (CPU) and tests/test_gpu_diff4th.py
(MI355X).

Arrays are indexed [z][y][x]; component 1 <-> x (the fastest axis), 2 <-> y, 3 <-> z; 2D drops component 3.  Every neighbour
index is clamped per axis into the array.  With dtype = float32 every operation below is one float32 rounding in the order
the parentheses give (numpy never contracts to FMA, and its / is the correctly rounded division), which is what the kernel
reproduces bit for bit; dtype = float64 is the same algorithm in double."""
import functools

import numpy as np

from _ndf_oracle import phantom, rel_change_sums, rel_d, rel_l2  # noqa: F401  (shared with NDF)

GHOST = 2   # ghost planes of U per interior boundary of a z-slab
# Chosen on the CPU (tests/test_diff4th_oracle.py asserts it): on (7, 13, 37) and (13, 37) between 10 % and 90 % of the
# voxels have G / s2 > 1 at the first and the last of 40 iterations, and tau (1 + 16 nd^2 lam) <= 1 with nd = 3.
PARAMS = {
    "A": dict(lam=1.0, sigma=3.2, tau=0.005),
    "B": dict(lam=0.25, sigma=3.5, tau=0.02),
    "C": dict(lam=3.0, sigma=3.3, tau=0.002),
}


def stable(lam, tau, nd=3):
    """the stability bound of the explicit scheme: tau (1 + 16 nd^2 lam) <= 1"""
    return tau * (1.0 + 16.0 * nd * nd * lam) <= 1.0


def _sh(U, ax, s):
    """U[i + s e_ax], the index clamped into the array"""
    n = U.shape[ax]
    return np.take(U, np.clip(np.arange(n) + s, 0, n - 1), axis=ax)


def weighted(U, s2, stats=None):
    """stage 1: the weighted second derivative W at every voxel.  `stats` (a dict) receives stats["active"]: the share of
    voxels with G / s2 > 1, and stats["g_zero"]: the share with G == 0 (the masked branch of Q / G)."""
    t = U.dtype.type
    nd = U.ndim
    half, quarter, one, two = t(0.5), t(0.25), t(1.0), t(2.0)
    c = U
    g, h = {}, {}
    for d in range(1, nd + 1):
        p, m = _sh(U, nd - d, 1), _sh(U, nd - d, -1)
        g[d] = half * (p - m)
        h[d] = (p + m) - (c + c)

    def k(d, e):
        Up, Um = _sh(U, nd - d, 1), _sh(U, nd - d, -1)
        return quarter * ((_sh(Up, nd - e, 1) - _sh(Up, nd - e, -1)) - (_sh(Um, nd - e, 1) - _sh(Um, nd - e, -1)))

    G = g[1] * g[1] + g[2] * g[2]
    L = h[1] + h[2]
    Q = (h[1] * (g[1] * g[1]) + h[2] * (g[2] * g[2])) + two * ((g[1] * g[2]) * k(1, 2))
    if nd == 3:
        G = G + g[3] * g[3]
        L = L + h[3]
        Q = Q + ((h[3] * (g[3] * g[3]) + two * ((g[1] * g[3]) * k(1, 3))) + two * ((g[2] * g[3]) * k(2, 3)))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        eta = np.where(G > 0, Q / np.where(G > 0, G, one), t(0.0))
        r = G / s2
        cw = one / (one + r)
        W = (cw * cw) * eta + cw * (L - eta)
    if stats is not None:
        stats["active"] = float(np.count_nonzero(r > one)) / r.size
        stats["g_zero"] = float(np.count_nonzero(G == 0)) / G.size
    return W


def step(U, f, lam, sigma, tau, stats=None):
    """one iteration: U' = c - tau (lam B + (c - f)), B the clamped Laplacian of W"""
    nd = U.ndim
    W = weighted(U, sigma * sigma, stats)
    B = None
    for d in range(1, nd + 1):
        b = (_sh(W, nd - d, 1) + _sh(W, nd - d, -1)) - (W + W)
        B = b if B is None else B + b
    return U - tau * (lam * B + (U - f))


def diff4th_iterates(f, lam, sigma, tau, iterations=1, dtype=np.float32, stats=None):
    """yields U after every iteration (a fresh array each time); `stats` (a dict) receives stats[n] = the share of voxels
    with G / s2 > 1 in iteration n (1-based) and stats["g_zero", n] = the share with G == 0"""
    t = dtype
    f = np.asarray(f).astype(t)
    assert f.ndim in (2, 3)
    lam, sigma, tau = t(lam), t(sigma), t(tau)
    U = f
    for n in range(iterations):
        s = {} if stats is not None else None
        U = step(U, f, lam, sigma, tau, s)
        if stats is not None:
            stats[n + 1] = s["active"]
            stats["g_zero", n + 1] = s["g_zero"]
        yield U


def diff4th(f, lam, sigma, tau, iterations=1, dtype=np.float32, stats=None):
    """U after `iterations` iterations (a copy of the input, as `dtype`, for 0)"""
    out = np.asarray(f).astype(dtype)
    for out in diff4th_iterates(f, lam, sigma, tau, iterations, dtype, stats):
        pass
    return out


def diff4th_many(f, params, counts, dtype=np.float32):
    """{n: U after n iterations} for every n of `counts`, from ONE run"""
    counts = sorted(set(counts))
    out = {}
    for n, U in enumerate(diff4th_iterates(f, iterations=counts[-1], dtype=dtype, **params), 1):
        if n in counts:
            out[n] = U
    return out


@functools.lru_cache(maxsize=None)
def cached(shape, pname, counts, dtype_name="float32"):
    """diff4th_many of the phantom of `shape` under parameter set "A".."C": computed once per session, never modified"""
    res = diff4th_many(phantom(shape), PARAMS[pname], counts, np.dtype(dtype_name).type)
    for v in res.values():
        v.setflags(write=False)
    return res


# ------------------------------------------------------------------------------------------------ z-slabs
def _as_numpy(t):
    return t.numpy() if hasattr(t, "numpy") else np.asarray(t)


def diff4th_step_slab(inp, u_in, u_out, dx, dy, nzl, lo, hi, lam, sigma, tau, zr=None):
    """One iteration on ghosted slab arrays [lo + nzl + hi][dy][dx] (host torch tensors or numpy arrays), the step_fn of
    tomobar_amd.slab.diff4th_slab: two ghost planes exist exactly where a z-neighbour exists, so the plain whole-array step
    on the ghosted array clamps in z only at the global faces and is right on every LOCAL plane; only the local planes
    [z0, z1) of `u_out` are written."""
    z0, z1 = zr if zr is not None else (0, nzl)
    f, U, out = _as_numpy(inp), _as_numpy(u_in), _as_numpy(u_out)
    assert lo in (0, GHOST) and hi in (0, GHOST)
    assert U.shape == (lo + nzl + hi, dy, dx) and U.dtype == np.float32
    a, b = max(lo + z0 - GHOST, 0), min(lo + z1 + GHOST, U.shape[0])    # the output planes and two planes either side
    new = step(U[a:b], f[a:b], np.float32(lam), np.float32(sigma), np.float32(tau))
    out[lo + z0:lo + z1] = new[lo + z0 - a:lo + z1 - a]


def slab_bounds(nz, world):
    base, extra = divmod(nz, world)
    bounds, z = [], 0
    for r in range(world):
        bounds.append((z, z + base + (1 if r < extra else 0)))
        z = bounds[-1][1]
    return bounds


def diff4th_by_slabs(f, params, iterations, world, bounds=None):
    """the whole volume run as `world` ghosted slabs (`bounds`: their plane ranges, an even split by default) exchanged by
    hand after every iteration, stitched"""
    f = np.asarray(f, np.float32)
    bounds = bounds or slab_bounds(f.shape[0], world)
    U = f.copy()
    for _ in range(iterations):
        new = np.empty_like(U)
        for r, (z0, z1) in enumerate(bounds):
            lo, hi = GHOST * int(r > 0), GHOST * int(r < len(bounds) - 1)
            g_in = np.ascontiguousarray(U[z0 - lo:z1 + hi])
            g_f = np.ascontiguousarray(f[z0 - lo:z1 + hi])
            g_out = np.full_like(g_in, np.nan)
            diff4th_step_slab(g_f, g_in, g_out, f.shape[2], f.shape[1], z1 - z0, lo, hi, params["lam"], params["sigma"],
                              params["tau"])
            new[z0:z1] = g_out[lo:lo + z1 - z0]
        U = new
    return U


# ------------------------------------------------------------------------------------------------ the tolerance rule
TOL_INTERVAL, TOL_MIN_SAVED = 6, 3
TOL_CASE = dict(shape=(7, 13, 37), pname="B", iterations=66, j=4)
TOL_CASE_SLAB = dict(shape=(9, 7, 11), pname="B", iterations=66, j=4)


@functools.lru_cache(maxsize=None)
def tolerance_plan(slab=False):
    """(tol, n the oracle's sequence stops after, the d it stops on, the whole sequence) of TOL_CASE (TOL_CASE_SLAB with
    `slab`): d_n compares iterate n with iterate n - 6 (iterate 0 = the input) after every 6th iteration that leaves at
    least 3; tol is the geometric mean of the (j-1)-th and j-th values, as tests/_ndf_oracle.py chooses its threshold"""
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
