"""TEST INFRASTRUCTURE: numpy restatement of the LLT_ROF regulariser (ROF total variation plus the fourth-order
Lysaker-Lundervold-Tai term, explicit in time) of docs/kernels/llt_rof.md (the specification; there is no reference
implementation to compare with -- formula-level parity, unpinned).  Shared by tests/test_llt_rof_oracle.py,
tests/test_llt_rof_slab_gloo.py (CPU), tests/test_gpu_llt_rof.py and tests/test_gpu_llt_rof_edges.py (MI355X).

Arrays are indexed [z][y][x]; component 1 <-> x (the fastest axis), 2 <-> y, 3 <-> z; 2D drops component 3.  Every neighbour
index of U is clamped per axis into the array.  With dtype = float32 every operation below is one float32 rounding in the
order the parentheses give (numpy never contracts to FMA, and its / and sqrt are the correctly rounded ones), which is what
the kernel reproduces bit for bit; dtype = float64 is the same algorithm in double."""
import functools

import numpy as np

from _ndf_oracle import phantom, rel_change_sums, rel_d, rel_l2  # noqa: F401  (shared with NDF, Diff4th)

GHOST = 2   # ghost planes of U per interior boundary of a z-slab
EPS = np.float32(1e-8)
# Chosen on the CPU (tests/test_llt_rof_oracle.py asserts it): on (7, 13, 37) and (13, 37) float32 stays within 5e-6 of
# float64 over 40 iterations, and both terms change the result in the first and in the 40th iteration.
PARAMS = {
    "A": dict(lam_rof=0.3, lam_llt=0.1, tau=0.02),
    "B": dict(lam_rof=0.05, lam_llt=0.15, tau=0.01),
    "C": dict(lam_rof=1.0, lam_llt=0.02, tau=0.005),
}


def _sh(U, ax, s):
    """U[i + s e_ax], the index clamped into the array"""
    n = U.shape[ax]
    return np.take(U, np.clip(np.arange(n) + s, 0, n - 1), axis=ax)


def _back0(R, ax):
    """R[i - e_ax], zero where i - e_ax lies outside the array"""
    out = np.zeros_like(R)
    dst, src = [slice(None)] * R.ndim, [slice(None)] * R.ndim
    dst[ax], src[ax] = slice(1, None), slice(0, -1)
    out[tuple(dst)] = R[tuple(src)]
    return out


def step(U, f, lam_rof, lam_llt, tau, stats=None):
    """one iteration: U' = c - tau ((lam_llt B - lam_rof V) + (c - f)).  `stats` (a dict) receives stats["s_zero"]: the
    share of voxels with s == 0, and stats["h1_tiny"]: the share with |h1| < 1e-6."""
    t = U.dtype.type
    nd = U.ndim
    eps = t(EPS)
    c = U
    a, h = {}, {}
    for d in range(1, nd + 1):
        p, m = _sh(U, nd - d, 1), _sh(U, nd - d, -1)
        a[d] = p - c
        h[d] = (p + m) - (c + c)
    s = a[1] * a[1] + a[2] * a[2]
    if nd == 3:
        s = s + a[3] * a[3]
    n = np.sqrt(s + eps)
    V = B = None
    for d in range(1, nd + 1):
        ax = nd - d
        R = a[d] / n
        v = R - _back0(R, ax)
        E = h[d] / (np.abs(h[d]) + eps)
        b = (_sh(E, ax, 1) + _sh(E, ax, -1)) - (E + E)
        V = v if V is None else V + v
        B = b if B is None else B + b
    if stats is not None:
        stats["s_zero"] = float(np.count_nonzero(s == 0)) / s.size
        stats["h1_tiny"] = float(np.count_nonzero(np.abs(h[1]) < 1e-6)) / s.size
    return c - tau * ((lam_llt * B - lam_rof * V) + (c - f))


def llt_rof_iterates(f, lam_rof, lam_llt, tau, iterations=1, dtype=np.float32, stats=None):
    """yields U after every iteration (a fresh array each time); `stats` (a dict) receives stats["s_zero", n] and
    stats["h1_tiny", n]: the shares of voxels with s == 0 and |h1| < 1e-6 entering iteration n (1-based)"""
    t = dtype
    f = np.asarray(f).astype(t)
    assert f.ndim in (2, 3)
    lam_rof, lam_llt, tau = t(np.float32(lam_rof)), t(np.float32(lam_llt)), t(np.float32(tau))
    U = f
    for n in range(iterations):
        s = {} if stats is not None else None
        U = step(U, f, lam_rof, lam_llt, tau, s)
        if stats is not None:
            stats["s_zero", n + 1] = s["s_zero"]
            stats["h1_tiny", n + 1] = s["h1_tiny"]
        yield U


def llt_rof(f, lam_rof, lam_llt, tau, iterations=1, dtype=np.float32, stats=None):
    """U after `iterations` iterations (a copy of the input, as `dtype`, for 0)"""
    out = np.asarray(f).astype(dtype)
    for out in llt_rof_iterates(f, lam_rof, lam_llt, tau, iterations, dtype, stats):
        pass
    return out


def llt_rof_many(f, params, counts, dtype=np.float32):
    """{n: U after n iterations} for every n of `counts`, from ONE run"""
    counts = sorted(set(counts))
    out = {}
    for n, U in enumerate(llt_rof_iterates(f, iterations=counts[-1], dtype=dtype, **params), 1):
        if n in counts:
            out[n] = U
    return out


@functools.lru_cache(maxsize=None)
def cached(shape, pname, counts, dtype_name="float32"):
    """llt_rof_many of the phantom of `shape` under parameter set "A".."C": computed once per session, never modified"""
    res = llt_rof_many(phantom(shape), PARAMS[pname], counts, np.dtype(dtype_name).type)
    for v in res.values():
        v.setflags(write=False)
    return res


# ------------------------------------------------------------------------------------------------ z-slabs
def _as_numpy(t):
    return t.numpy() if hasattr(t, "numpy") else np.asarray(t)


def llt_rof_step_slab(inp, u_in, u_out, dx, dy, nzl, lo, hi, lam_rof, lam_llt, tau, zr=None, ghost=GHOST):
    """One iteration on ghosted slab arrays [lo + nzl + hi][dy][dx] (host torch tensors or numpy arrays), the step_fn of
    tomobar_amd.slab.llt_rof_slab: two ghost planes exist exactly where a z-neighbour exists, so the plain whole-array step
    on the ghosted array clamps in z -- and drops the backward neighbour of R3 -- only at the global faces and is right on
    every LOCAL plane; only the local planes [z0, z1) of `u_out` are written.  (`ghost` = 1 exists for the test that shows
    one plane is not enough.)"""
    z0, z1 = zr if zr is not None else (0, nzl)
    f, U, out = _as_numpy(inp), _as_numpy(u_in), _as_numpy(u_out)
    assert lo in (0, ghost) and hi in (0, ghost)
    assert U.shape == (lo + nzl + hi, dy, dx) and U.dtype == np.float32
    a, b = max(lo + z0 - ghost, 0), min(lo + z1 + ghost, U.shape[0])    # the output planes and the ghost depth either side
    new = step(U[a:b], f[a:b], np.float32(lam_rof), np.float32(lam_llt), np.float32(tau))
    out[lo + z0:lo + z1] = new[lo + z0 - a:lo + z1 - a]


def slab_bounds(nz, world):
    base, extra = divmod(nz, world)
    bounds, z = [], 0
    for r in range(world):
        bounds.append((z, z + base + (1 if r < extra else 0)))
        z = bounds[-1][1]
    return bounds


def llt_rof_by_slabs(f, params, iterations, world, bounds=None, ghost=GHOST):
    """the whole volume run as `world` ghosted slabs (`bounds`: their plane ranges, an even split by default) exchanged by
    hand after every iteration, stitched"""
    f = np.asarray(f, np.float32)
    bounds = bounds or slab_bounds(f.shape[0], world)
    U = f.copy()
    for _ in range(iterations):
        new = np.empty_like(U)
        for r, (z0, z1) in enumerate(bounds):
            lo, hi = ghost * int(r > 0), ghost * int(r < len(bounds) - 1)
            g_in = np.ascontiguousarray(U[z0 - lo:z1 + hi])
            g_f = np.ascontiguousarray(f[z0 - lo:z1 + hi])
            g_out = np.full_like(g_in, np.nan)
            llt_rof_step_slab(g_f, g_in, g_out, f.shape[2], f.shape[1], z1 - z0, lo, hi, params["lam_rof"],
                              params["lam_llt"], params["tau"], ghost=ghost)
            new[z0:z1] = g_out[lo:lo + z1 - z0]
        U = new
    return U


# ------------------------------------------------------------------------------------------------ the tolerance rule
TOL_INTERVAL, TOL_MIN_SAVED = 6, 3
TOL_CASE = dict(shape=(7, 13, 37), pname="A", iterations=66, j=4)
TOL_CASE_SLAB = dict(shape=(9, 7, 11), pname="A", iterations=66, j=4)


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
