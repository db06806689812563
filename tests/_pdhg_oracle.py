"""TEST INFRASTRUCTURE: numpy restatement of PDHG as docs/kernels/pdhg.md states it (the specification; there is no reference
implementation to compare with -- formula-level parity, unpinned).  Shared by tests/test_pdhg_oracle.py (CPU) and
tests/test_gpu_pdhg.py (MI355X).

Volumes are [nz][ny][nx] arrays, indexed [z][y][x]; component 1 <-> x (the fastest axis), 2 <-> y, 3 <-> z; nd = 3 if
nz > 1 else 2, and nd = 2 has no component 3.  With dtype = float32 every operation below is one float32 rounding in the
order the parentheses give (numpy never contracts to FMA), which is what the kernels reproduce bit for bit; dtype = float64
is the same algorithm in double.  The clamps are written as comparisons (``where``), as the kernels write them: the sign of
a zero and a NaN pass through the same way on both sides.

The float32 form runs on an operator pair with ``fp`` / ``bp`` -- tests/_matched_bp_oracle.MatchedProjector: the C oracle's
forward projector and the float32 restatement of its exact transpose --, the float64 form on `Dense64`, the dense float64
matrix of the same forward projector and its transpose."""
import functools

import numpy as np

import _matched_bp_oracle as M
from _tgv_oracle import _B, _F, rel_l2  # noqa: F401  (the stencils of docs/kernels/tgv.md, vectorised; rel_l2 re-exported)

FIDELITIES = ("LS", "L1", "KL")


def nd_of(shape):
    return 3 if shape[0] > 1 else 2


def scalars(L_A, nd, tv=True, ratio=1.0, dtype=np.float32, L_K=None):
    """(sigma, tau) in `dtype`: L_K = L_A + 4 nd (L_A without TV), s = 0.95 / sqrt(L_K), sigma = s rho, tau = s / rho.
    `L_K` given: taken as it is (the z-constant check gives the 3D and the 2D run the same one)."""
    t = dtype
    if L_K is None:
        L_K = t(L_A) + t(4 * nd) if tv else t(L_A)
    s = t(0.95) / np.sqrt(t(L_K))
    rho = t(ratio)
    return t(s * rho), t(s / rho)


# ------------------------------------------------------------------------------------------------ the three updates
def sino_dual(y, r, b, fidelity, sigma):
    """step 2: y <- prox_{sigma F*}(y + sigma r), element-wise; the dtype is that of `y`"""
    t = y.dtype.type
    sigma = t(sigma)
    if fidelity == "LS":
        return (y + sigma * (r - b)) / (t(1) + sigma)
    if fidelity == "L1":
        v = y + sigma * (r - b)
        v = np.where(v < t(-1), t(-1), v)
        return np.where(v > t(1), t(1), v)
    if fidelity == "KL":
        c4 = t(4) * sigma
        v = y + sigma * r
        tt = v - t(1)
        bp = np.where(b > t(0), b, t(0))
        return t(0.5) * ((t(1) + v) - np.sqrt(tt * tt + c4 * bp))
    raise ValueError(fidelity)


def _axes(nd):
    """numpy axis of component d of a [z][y][x] array: 1 -> 2, 2 -> 1, 3 -> 0"""
    return {d: 3 - d for d in range(1, nd + 1)}


def tv_dual(xbar, q, sigma, lam, methodTV, stats=None):
    """step 4: q_d <- q_d + sigma F_d(x-bar), projected.  `q`: list of nd arrays; returns the new list.  `stats` (a dict)
    receives the share of voxels on which the projection changed q: stats["active"]."""
    t = xbar.dtype.type
    sigma, lam = t(sigma), t(lam)
    nd = len(q)
    ax = _axes(nd)
    q = [q[d - 1] + sigma * _F(xbar, ax[d]) for d in range(1, nd + 1)]
    if methodTV:
        out = []
        for c in q:
            v = np.where(c < -lam, -lam, c)
            out.append(np.where(v > lam, lam, v))
        if stats is not None:
            stats["active"] = float(np.mean(np.any([np.abs(c) > lam for c in q], axis=0)))
        return out
    m = q[0] * q[0] + q[1] * q[1]
    if nd == 3:
        m = m + q[2] * q[2]
    n = np.sqrt(m) / lam
    act = n > t(1)
    if stats is not None:
        stats["active"] = float(act.mean())
    den = np.where(act, n, t(1))
    return [c / den for c in q]


def primal(x, g, q, tau, nonneg):
    """step 5: returns (x', x-bar').  `q` empty: no TV block, div = 0."""
    t = x.dtype.type
    tau = t(tau)
    if q:
        ax = _axes(len(q))
        div = _B(q[0], ax[1]) + _B(q[1], ax[2])
        if len(q) == 3:
            div = div + _B(q[2], ax[3])
    else:
        div = np.zeros_like(x)
    xn = x - tau * (g - div)
    if nonneg:
        xn = np.where(xn < t(0), t(0), xn)
    return xn, (xn + xn) - x


def march_steps(x0, g, sigma, tau, lam, methodTV, nonneg, counts, nd=None, stats=None):
    """steps 4 and 5 alone, on a fixed `g`: {n: (x, x-bar, q) after n steps} for every n of `counts`, from x = x-bar = x0,
    q = 0 (the kernel tests).  `lam` None: no TV block.  `stats`: the projection's share after the FIRST step."""
    x = np.array(x0)
    xbar = x.copy()
    nd = nd_of(x.shape) if nd is None else nd
    q = [np.zeros_like(x) for _ in range(nd)] if lam is not None else []
    out = {}
    for n in range(1, max(counts) + 1):
        if q:
            q = tv_dual(xbar, q, sigma, lam, methodTV, stats if n == 1 else None)
        x, xbar = primal(x, g, q, tau, nonneg)
        if n in counts:
            out[n] = (x, xbar, list(q))
    return out


# ------------------------------------------------------------------------------------------------ the loop
def pdhg_iterates(P, b, L_A, fidelity="LS", lam=None, methodTV=0, nonneg=False, ratio=1.0, x0=None, iterations=1,
                  dtype=np.float32, nd=None, L_K=None, state=None):
    """yields x after every iteration (a fresh array each time).  `P`: the operator pair (fp, bp) on [nz, n, n] volumes;
    `lam` None: no TV block.  `nd`, `L_K`: overrides (else from the volume and L_A).  `state` (a dict) receives the arrays
    of the last iteration run: y, q, xbar."""
    t = dtype
    b = np.asarray(b).astype(t)
    shape = (b.shape[0], P.n, P.n)
    nd = nd_of(shape) if nd is None else nd
    tv = lam is not None
    sigma, tau = scalars(L_A, nd, tv, ratio, t, L_K)
    x = np.zeros(shape, t) if x0 is None else np.asarray(x0).astype(t)
    xbar = x.copy()
    y = np.zeros_like(b)
    q = [np.zeros(shape, t) for _ in range(nd)] if tv else []
    for _ in range(iterations):
        r = np.asarray(P.fp(xbar)).astype(t, copy=False)
        y = sino_dual(y, r, b, fidelity, sigma)
        g = np.asarray(P.bp(y)).astype(t, copy=False)
        if tv:
            q = tv_dual(xbar, q, sigma, lam, methodTV)
        x, xbar = primal(x, g, q, tau, nonneg)
        if state is not None:
            state.update(y=y, q=q, xbar=xbar)
        yield x


def pdhg(P, b, L_A, iterations, **kw):
    """x after `iterations` iterations"""
    out = None
    for out in pdhg_iterates(P, b, L_A, iterations=iterations, **kw):
        pass
    return out


def pdhg_many(P, b, L_A, counts, **kw):
    """{n: x after n iterations} for every n of `counts`, from ONE run"""
    counts = sorted(set(counts))
    out = {}
    for n, x in enumerate(pdhg_iterates(P, b, L_A, iterations=counts[-1], **kw), 1):
        if n in counts:
            out[n] = x
    return out


# ------------------------------------------------------------------------------------------------ the float64 operator
class Dense64:
    """The forward projector as a dense float64 matrix (tests/_matched_bp_oracle.fp_matrix64: orc_fp3d restated in float64)
    and its exact transpose, slice by slice."""

    def __init__(self, n, nu, angles, cor=0.0):
        self.n, self.nu, self.na = int(n), int(nu), len(angles)
        self.A = _matrix(self.n, self.nu, tuple(float(a) for a in angles), float(cor))

    def fp(self, vol):
        vol = np.asarray(vol, np.float64)
        return (vol.reshape(vol.shape[0], -1) @ self.A.T).reshape(vol.shape[0], self.na, self.nu)

    def bp(self, sino):
        sino = np.asarray(sino, np.float64)
        return (sino.reshape(sino.shape[0], -1) @ self.A).reshape(sino.shape[0], self.n, self.n)

    def norm2(self):
        """L_A = the largest eigenvalue of A^T A"""
        return float(np.linalg.norm(self.A, 2) ** 2)


@functools.lru_cache(maxsize=None)
def _matrix(n, nu, angles, cor):
    A = M.fp_matrix64(n, nu, np.asarray(angles), cor)
    A.setflags(write=False)
    return A


# ------------------------------------------------------------------------------------------------ the objective (float64)
def tv_seminorm(x, methodTV=0):
    x = np.asarray(x, np.float64)
    nd = nd_of(x.shape)
    F = [_F(x, ax) for ax in _axes(nd).values()]
    if methodTV:
        return float(sum(np.abs(f).sum() for f in F))
    return float(np.sqrt(sum(f * f for f in F)).sum())


def data_term(ax, b, fidelity):
    """F(Ax) in float64: 1/2 |Ax - b|^2, |Ax - b|_1 or sum(Ax - max(b, 0) log Ax) (+inf where Ax <= 0 meets b > 0)"""
    ax, b = np.asarray(ax, np.float64), np.asarray(b, np.float64)
    if fidelity == "LS":
        return 0.5 * float(((ax - b) ** 2).sum())
    if fidelity == "L1":
        return float(np.abs(ax - b).sum())
    bp = np.maximum(b, 0.0)
    if np.any((ax <= 0.0) & (bp > 0.0)) or np.any(ax < 0.0):
        return float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        return float((ax - np.where(bp > 0.0, bp * np.log(ax), 0.0)).sum())


def objective(P64, x, b, fidelity, lam=None, methodTV=0):
    """F(Ax) + lambda TV(x) in float64 on the dense operator"""
    value = data_term(P64.fp(x), b, fidelity)
    return value + (float(lam) * tv_seminorm(x, methodTV) if lam is not None else 0.0)


# ------------------------------------------------------------------------------------------------ Moreau
def prox_primal(w, b, fidelity, gamma):
    """prox_{gamma F}(w) in float64, element-wise: the closed forms of the three data terms (KL: the positive root of
    u^2 + (gamma - w) u - gamma max(b, 0) = 0)"""
    w, b = np.asarray(w, np.float64), np.asarray(b, np.float64)
    if fidelity == "LS":
        return (w + gamma * b) / (1.0 + gamma)
    if fidelity == "L1":
        return b + np.sign(w - b) * np.maximum(np.abs(w - b) - gamma, 0.0)
    bp = np.maximum(b, 0.0)
    return 0.5 * ((w - gamma) + np.sqrt((w - gamma) ** 2 + 4.0 * gamma * bp))
