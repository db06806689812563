"""TEST INFRASTRUCTURE: numpy restatement of PDHG with the diagonal preconditioner (Pock and Chambolle 2011, alpha = 1) as
docs/kernels/pdhg.md states it (the specification; formula-level parity, unpinned).  Shared by
tests/test_pdhg_diag_oracle.py (CPU) and tests/test_gpu_pdhg_diag.py (MI355X).

The conventions, the stencils, the TV dual (step 4), the float64 operator and the objective are those of
tests/_pdhg_oracle.py; what changes is where the steps come from -- sigma_i = a / max((A 1)_i, eps) per sample,
tau_j = t / max((A^T 1)_j + w, eps) per voxel, sigma_G = a / 2 for the TV block, no operator norm -- and that steps 2 and 5
read theirs from those arrays.  With dtype = float32 every operation is one float32 rounding in the order the parentheses
give; the guard is the comparison ``v < eps ? eps : v``."""
import numpy as np

import _pdhg_oracle as P
from _pdhg_oracle import Dense64, _axes, _B, _F, nd_of, objective, rel_l2, tv_dual  # noqa: F401  (re-exported)
from _matched_bp_oracle import MatchedProjector  # noqa: F401  (the float32 operator pair the float32 form runs on)

EPS = 2.0 ** -10
C = 0.95


def host_scalars(nd, tv=True, ratio=1.0, dtype=np.float32):
    """(a, t, sigma_G, w) in `dtype`: c = 0.95, a = c rho, t = c / rho, sigma_G = a / 2, w = 2 nd with TV, else 0"""
    f = dtype
    c, rho = f(C), f(ratio)
    a = f(c * rho)
    return a, f(c / rho), f(a / f(2)), f(2 * nd) if tv else f(0)


def diag_steps(sums, numer, add=0.0):
    """numer / max(sums + add, eps), element-wise, in the dtype of `sums`"""
    f = sums.dtype.type
    v = sums + f(add)
    eps = f(EPS)
    return f(numer) / np.where(v < eps, eps, v)


def step_arrays(op, sino_shape, vol_shape, nd, tv=True, ratio=1.0, dtype=np.float32):
    """(sigma [the sinogram's shape], tau [the volume's], sigma_G): the set-up, two projector calls"""
    a, t, sigma_G, w = host_scalars(nd, tv, ratio, dtype)
    R = np.asarray(op.fp(np.ones(vol_shape, dtype))).astype(dtype, copy=False)
    Cs = np.asarray(op.bp(np.ones(sino_shape, dtype))).astype(dtype, copy=False)
    return diag_steps(R, a), diag_steps(Cs, t, w), sigma_G


# ------------------------------------------------------------------------------------------------ the two updates
def sino_dual(y, r, b, fidelity, sigma):
    """step 2 with sigma_i: `sigma` is an array like `y`"""
    f = y.dtype.type
    assert sigma.dtype == y.dtype and sigma.shape == y.shape
    if fidelity == "LS":
        return (y + sigma * (r - b)) / (f(1) + sigma)
    if fidelity == "L1":
        v = y + sigma * (r - b)
        v = np.where(v < f(-1), f(-1), v)
        return np.where(v > f(1), f(1), v)
    if fidelity == "KL":
        v = y + sigma * r
        u = v - f(1)
        bp = np.where(b > f(0), b, f(0))
        return f(0.5) * ((f(1) + v) - np.sqrt(u * u + (f(4) * sigma) * bp))
    raise ValueError(fidelity)


def primal(x, g, q, tau, nonneg):
    """step 5 with tau_j: `tau` is an array like `x`; returns (x', x-bar').  `q` empty: no TV block, div = 0."""
    f = x.dtype.type
    assert tau.dtype == x.dtype and tau.shape == x.shape
    if q:
        ax = _axes(len(q))
        div = _B(q[0], ax[1]) + _B(q[1], ax[2])
        if len(q) == 3:
            div = div + _B(q[2], ax[3])
    else:
        div = np.zeros_like(x)
    xn = x - tau * (g - div)
    if nonneg:
        xn = np.where(xn < f(0), f(0), xn)
    return xn, (xn + xn) - x


def march_steps(x0, g, sigma_G, tau, lam, methodTV, nonneg, counts, nd=None):
    """steps 4 and 5 alone, on a fixed `g` and a step field `tau`: {n: (x, x-bar, q) after n steps} for every n of `counts`,
    from x = x-bar = x0, q = 0 (the kernel tests).  `lam` None: no TV block."""
    x = np.array(x0)
    xbar = x.copy()
    nd = nd_of(x.shape) if nd is None else nd
    q = [np.zeros_like(x) for _ in range(nd)] if lam is not None else []
    out = {}
    for n in range(1, max(counts) + 1):
        if q:
            q = tv_dual(xbar, q, sigma_G, lam, methodTV)
        x, xbar = primal(x, g, q, tau, nonneg)
        if n in counts:
            out[n] = (x, xbar, list(q))
    return out


# ------------------------------------------------------------------------------------------------ the loop
def pdhg_iterates(op, b, fidelity="LS", lam=None, methodTV=0, nonneg=False, ratio=1.0, x0=None, iterations=1,
                  dtype=np.float32, vol_shape=None, state=None):
    """yields x after every iteration (a fresh array each time).  `op`: the operator pair (fp, bp); `vol_shape` defaults to
    (b.shape[0], op.n, op.n) (an operator whose sinograms are not [nz, angles, nu] arrays gives it).  `lam` None: no TV
    block.  `state` (a dict) receives sigma and tau at set-up and the arrays of the last iteration run: y, q, xbar."""
    f = dtype
    b = np.asarray(b).astype(f)
    shape = (b.shape[0], op.n, op.n) if vol_shape is None else tuple(vol_shape)
    nd = nd_of(shape)
    tv = lam is not None
    sigma, tau, sigma_G = step_arrays(op, b.shape, shape, nd, tv, ratio, f)
    if state is not None:
        state.update(sigma=sigma, tau=tau, sigma_G=sigma_G)
    x = np.zeros(shape, f) if x0 is None else np.asarray(x0).astype(f)
    xbar = x.copy()
    y = np.zeros_like(b)
    q = [np.zeros(shape, f) for _ in range(nd)] if tv else []
    for _ in range(iterations):
        r = np.asarray(op.fp(xbar)).astype(f, copy=False)
        y = sino_dual(y, r, b, fidelity, sigma)
        g = np.asarray(op.bp(y)).astype(f, copy=False)
        if tv:
            q = tv_dual(xbar, q, sigma_G, lam, methodTV)
        x, xbar = primal(x, g, q, tau, nonneg)
        if state is not None:
            state.update(y=y, q=q, xbar=xbar)
        yield x


def pdhg(op, b, iterations, **kw):
    """x after `iterations` iterations"""
    out = None
    for out in pdhg_iterates(op, b, iterations=iterations, **kw):
        pass
    return out


def pdhg_many(op, b, counts, **kw):
    """{n: x after n iterations} for every n of `counts`, from ONE run"""
    counts = sorted(set(counts))
    out = {}
    for n, x in enumerate(pdhg_iterates(op, b, iterations=counts[-1], **kw), 1):
        if n in counts:
            out[n] = x
    return out


# ------------------------------------------------------------------------------------------------ the dense K = [A; grad]
def gradient_matrix(shape):
    """the F_d of a [nz, ny, nx] volume as one dense float64 matrix [nd * nvox, nvox], component 1 first"""
    nvox = int(np.prod(shape))
    basis = np.eye(nvox).reshape((nvox,) + tuple(shape))
    rows = [_F(basis, 1 + ax).reshape(nvox, nvox).T for ax in _axes(nd_of(shape)).values()]
    return np.vstack(rows)
