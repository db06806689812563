"""TEST INFRASTRUCTURE: numpy restatement of the second-order TGV prox of docs/kernels/tgv.md (the specification; there
is no reference implementation to compare with -- formula-level parity, unpinned).  Shared by tests/test_tgv_oracle.py (CPU)
and tests/test_gpu_tgv.py (MI355X).

Arrays are indexed [z][y][x]; component 1 <-> x (the fastest axis), 2 <-> y, 3 <-> z; 2D drops component 3 and Q13, Q23,
Q33.  With dtype = float32 every operation below is one float32 rounding in the order the parentheses give (numpy never
contracts to FMA), which is what the kernels reproduce bit for bit; dtype = float64 is the same algorithm in double."""
import functools

import numpy as np

PARAMS_A = dict(lam=5.0, alpha1=1.0, alpha0=2.0, L=12.0)
PARAMS_B = dict(lam=0.5, alpha1=1.0, alpha0=0.1, L=12.0)


def phantom(shape):
    """ramp + a step with a different slope beyond x > nx / 2 + Gaussian noise, times 40, float32"""
    coords = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    x, nx = coords[-1], shape[-1]
    vol = sum(0.03 * (k + 1) * c for k, c in enumerate(coords))
    vol = vol + np.where(x > nx / 2, 0.5 - 0.02 * x, 0.0)
    vol = vol + 0.05 * np.random.default_rng(3).standard_normal(shape)
    return np.ascontiguousarray((40.0 * vol).astype(np.float32))


def scalars(lam, alpha1, alpha0, L, dtype=np.float32):
    """(lambda, alpha1, alpha0, tau, sigma) in `dtype`, formed as TGV_cupy forms them"""
    t = dtype
    tau = t(t(1.0) / np.sqrt(t(L)))
    return t(lam), t(alpha1), t(alpha0), tau, tau


def _axis(nd, d):
    """numpy axis of component d (1 = x = the last axis)"""
    return nd - d


def _F(a, ax):
    """forward difference: a[i + e] - a[i], exactly 0 on the last index"""
    out = np.zeros_like(a)
    n = a.shape[ax]
    hi = [slice(None)] * a.ndim
    lo = [slice(None)] * a.ndim
    hi[ax], lo[ax] = slice(1, n), slice(0, n - 1)
    out[tuple(lo)] = a[tuple(hi)] - a[tuple(lo)]
    return out


def _B(a, ax):
    """backward difference: a[i] - a[i - e], a[i] on the first index"""
    out = a.copy()
    n = a.shape[ax]
    hi = [slice(None)] * a.ndim
    lo = [slice(None)] * a.ndim
    hi[ax], lo[ax] = slice(1, n), slice(0, n - 1)
    out[tuple(hi)] = a[tuple(hi)] - a[tuple(lo)]
    return out


def tgv_iterates(f, lam, alpha1, alpha0, L=12.0, iterations=1, dtype=np.float32, stats=None):
    """yields U after every iteration (a fresh array each time).  `stats` (a dict) receives, for the LAST iteration run, the
    fractions of voxels whose P / Q projection was active: stats["n_gt_1"], stats["m_gt_1"]."""
    t = dtype
    f = np.asarray(f).astype(t)
    nd = f.ndim
    assert nd in (2, 3)
    lam, a1, a0, tau, sigma = scalars(lam, alpha1, alpha0, L, t)
    half, two = t(0.5), t(2.0)
    comps = list(range(1, nd + 1))
    pairs = [(d, e) for d in comps for e in comps if d < e]          # (1,2), (1,3), (2,3)
    ax = {d: _axis(nd, d) for d in comps}
    U, Ub = f.copy(), f.copy()
    V = {d: np.zeros_like(f) for d in comps}
    Vb = {d: np.zeros_like(f) for d in comps}
    P = {d: np.zeros_like(f) for d in comps}
    Q = {(d, d): np.zeros_like(f) for d in comps}
    Q.update({pr: np.zeros_like(f) for pr in pairs})
    for _ in range(iterations):
        # 1. dual P
        for d in comps:
            P[d] = P[d] + sigma * (_F(Ub, ax[d]) - Vb[d])
        s = P[1] * P[1] + P[2] * P[2]
        if nd == 3:
            s = s + P[3] * P[3]
        n = np.sqrt(s) / a1
        act_n = n > 1
        for d in comps:
            P[d] = np.where(act_n, P[d] / np.where(act_n, n, t(1.0)), P[d])
        # 2. dual Q
        for d in comps:
            Q[d, d] = Q[d, d] + sigma * _F(Vb[d], ax[d])
        for d, e in pairs:
            Q[d, e] = Q[d, e] + sigma * (half * (_F(Vb[d], ax[e]) + _F(Vb[e], ax[d])))
        sd = Q[1, 1] * Q[1, 1] + Q[2, 2] * Q[2, 2]
        so = Q[1, 2] * Q[1, 2]
        if nd == 3:
            sd = sd + Q[3, 3] * Q[3, 3]
            so = (so + Q[1, 3] * Q[1, 3]) + Q[2, 3] * Q[2, 3]
        m = np.sqrt(sd + two * so) / a0
        act_m = m > 1
        for k in Q:
            Q[k] = np.where(act_m, Q[k] / np.where(act_m, m, t(1.0)), Q[k])
        if stats is not None:
            stats["n_gt_1"], stats["m_gt_1"] = float(act_n.mean()), float(act_m.mean())
        # 3. primal U
        div = _B(P[1], ax[1]) + _B(P[2], ax[2])
        if nd == 3:
            div = div + _B(P[3], ax[3])
        Un = (lam * (U + tau * div) + tau * f) / (lam + tau)
        Ub = two * Un - U
        U = Un
        # 4. primal V
        for d in comps:
            acc = P[d] + _B(Q[d, d], ax[d])
            for e in comps:
                if e != d:
                    acc = acc + _B(Q[min(d, e), max(d, e)], ax[e])
            Vn = V[d] + tau * acc
            Vb[d] = two * Vn - V[d]
            V[d] = Vn
        yield U


def tgv(f, lam, alpha1, alpha0, L=12.0, iterations=1, dtype=np.float32, stats=None):
    """U after `iterations` iterations (the input itself, as `dtype`, for 0)"""
    out = np.asarray(f).astype(dtype)
    for out in tgv_iterates(f, lam, alpha1, alpha0, L, iterations, dtype, stats):
        pass
    return out


def tgv_many(f, params, counts, dtype=np.float32):
    """{n: U after n iterations} for every n of `counts`, from ONE run"""
    counts = sorted(set(counts))
    out = {}
    for n, U in enumerate(tgv_iterates(f, iterations=counts[-1], dtype=dtype, **params), 1):
        if n in counts:
            out[n] = U
    return out


@functools.lru_cache(maxsize=None)
def cached(shape, pname, counts, dtype_name="float32"):
    """tgv_many of the phantom of `shape` under parameter set "A" / "B": computed once per session, never modified"""
    res = tgv_many(phantom(shape), PARAMS_A if pname == "A" else PARAMS_B, counts, np.dtype(dtype_name).type)
    for v in res.values():
        v.setflags(write=False)
    return res


def rel_l2(a, b):
    a64, b64 = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a64 - b64) / max(np.linalg.norm(b64), 1e-300))


# ------------------------------------------------------------------------------------------------ the tolerance rule
TOL_INTERVAL, TOL_MIN_SAVED = 6, 3
TOL_CASE = dict(shape=(7, 13, 37), pname="A", iterations=66, j=4)   # (the 2nd and 3rd values lie within 2 % of each other)


def rel_d(v, ref):
    """d = sqrt(sum (v - ref)^2 / sum v^2) in float64 from the float32 values"""
    v64, r64 = np.asarray(v, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    return float(np.sqrt(np.sum((v64 - r64) ** 2) / np.sum(v64 ** 2)))


@functools.lru_cache(maxsize=None)
def tolerance_plan():
    """(tol, n the oracle's sequence stops after, the d it stops on, the whole sequence) of TOL_CASE: d_n compares iterate n
    with iterate n - 6 (iterate 0 = the input) after every 6th iteration that leaves at least 3; tol is the geometric mean
    of the (j-1)-th and j-th values, as tests/_tolerance_cases.py chooses its thresholds"""
    c = TOL_CASE
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
