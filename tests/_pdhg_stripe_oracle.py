"""TEST INFRASTRUCTURE: numpy restatement of PDHG with the stripe variable (``_data_["stripe_lambda"]``) as
docs/kernels/pdhg.md states it (the specification; there is no reference implementation to compare with -- formula-level
parity, unpinned).  Shared by tests/test_pdhg_stripe_oracle.py, tests/test_pdhg_stripe_surface.py (CPU) and
tests/test_gpu_pdhg_stripe.py (MI355X).

    min_{x, s}  F(A x + S s; b) + lambda R(x) + mu |s|_1,        s[z, u] one offset per detector pixel, (S s)[z, a, u] = s[z, u]

The conventions, the data terms, the stencils and the float64 operator are those of tests/_pdhg_oracle.py, the diagonal steps
those of tests/_pdhg_diag_oracle.py, the TGV block that of tests/_pdhg_tgv_oracle.py; steps 1 and 3-5 of an iteration are
theirs, untouched.  What is new is step 2 on e = r + s-bar, the sum of the new y along the angles in segments of 64 rows, and
step 6.  With dtype = float32 every operation below is one float32 rounding in the order the parentheses give, which is what
the kernels reproduce bit for bit; dtype = float64 is the same algorithm, segments included, in double."""
import numpy as np

import _pdhg_diag_oracle as D
import _pdhg_oracle as P
import _pdhg_tgv_oracle as G
from _pdhg_oracle import Dense64, nd_of, rel_l2  # noqa: F401  (re-exported)

SEG = 64   # the segment length G of the specification


def n_seg(na):
    return (int(na) + SEG - 1) // SEG


# ------------------------------------------------------------------------------------------------ the two launches
def segment_sums(y):
    """part[k][z][u]: acc = +0; acc = acc + y[z][a][u] for a ascending over segment k.  `y`: [nz, na, nu]"""
    nz, na, nu = y.shape
    part = np.zeros((n_seg(na), nz, nu), y.dtype)
    for k in range(part.shape[0]):
        acc = np.zeros((nz, nu), y.dtype)
        for a in range(k * SEG, min((k + 1) * SEG, na)):
            acc = acc + y[:, a, :]
        part[k] = acc
    return part


def sino_dual_stripe(y, r, b, sbar, fidelity, sigma):
    """step 2 with the stripe variable: e = r + s-bar (one rounding), then the prox of tests/_pdhg_oracle.sino_dual (`sigma` a
    scalar) or tests/_pdhg_diag_oracle.sino_dual (`sigma` an array like `y`) on e in place of r.  Returns (y', part)."""
    assert sbar.dtype == y.dtype and sbar.shape == (y.shape[0], y.shape[2])
    e = r + sbar[:, None, :]
    yn = D.sino_dual(y, e, b, fidelity, sigma) if isinstance(sigma, np.ndarray) else P.sino_dual(y, e, b, fidelity, sigma)
    return yn, segment_sums(yn)


def stripe_update(s, part, tau_s, theta):
    """step 6: c = +0, c = c + part[k] for k ascending; w = s - tau_s c; s' = w > theta ? w - theta : (w < -theta ? w + theta
    : +0).  Returns (s', s-bar' = (s' + s') - s)."""
    t = s.dtype.type
    tau_s, theta = t(tau_s), t(theta)
    c = np.zeros_like(s)
    for k in range(part.shape[0]):
        c = c + part[k]
    w = s - tau_s * c
    sn = np.where(w > theta, w - theta, np.where(w < -theta, w + theta, t(0)))
    return sn, (sn + sn) - s


# ------------------------------------------------------------------------------------------------ the host scalars
def lipschitz(L_A, na, nd, regulariser, dtype=np.float32):
    """L_K = f(L_A) + f(na), then + f(4 nd) with TV or + L_R (12 for nd = 2, 16 for nd = 3) with TGV, in that order"""
    t = dtype
    L_K = t(L_A) + t(na)
    if regulariser == "TV":
        L_K = L_K + t(4 * nd)
    elif regulariser == "TGV":
        L_K = L_K + t(16 if nd == 3 else 12)
    return t(L_K)


def threshold(tau_s, mu, dtype=np.float32):
    """theta = tau_s mu, one product"""
    return dtype(dtype(tau_s) * dtype(mu))


def diag_stripe_steps(op, sino_shape, vol_shape, nd, regularised, ratio=1.0, dtype=np.float32):
    """(sigma [the sinogram's shape], tau [the volume's], tau_s): sigma_i = a / max(R_i + 1, eps) -- a row of [A S] gains one
    entry 1 --, tau_j as without the stripe variable, tau_s = t / f(na) -- a column of S sums to na"""
    a, t, _, w = D.host_scalars(nd, regularised, ratio, dtype)
    R = np.asarray(op.fp(np.ones(vol_shape, dtype))).astype(dtype, copy=False)
    Cs = np.asarray(op.bp(np.ones(sino_shape, dtype))).astype(dtype, copy=False)
    return D.diag_steps(R, a, 1.0), D.diag_steps(Cs, t, w), dtype(t / dtype(sino_shape[1]))


# ------------------------------------------------------------------------------------------------ the loop
def pdhg_stripe_iterates(op, b, L_A=None, mu=1.0, fidelity="LS", regulariser=None, lam=None, methodTV=0, alpha1=1.0, alpha0=2.0,
                         nonneg=False, ratio=1.0, x0=None, iterations=1, dtype=np.float32, diagonal=False, state=None):
    """yields x after every iteration (a fresh array each time).  `op`: the operator pair (fp, bp) on [nz, n, n] volumes and
    [nz, na, nu] sinograms; `regulariser`: None, "TV" (`lam`, `methodTV`) or "TGV" (`lam`, `alpha1`, `alpha0`); `diagonal`: the
    diagonal preconditioner (L_A is not read).  `state` (a dict) receives the scalars at set-up (sigma, tau, tau_s, theta) and
    the arrays of the last iteration run: y, xbar, s, sbar, part (and q, or p, q, v, vbar)."""
    t = dtype
    b = np.asarray(b).astype(t)
    nz, na, nu = b.shape
    shape = (nz, op.n, op.n)
    nd = nd_of(shape)
    assert regulariser in (None, "TV", "TGV")
    tv, tgv = regulariser == "TV", regulariser == "TGV"
    if diagonal:
        sigma, tau, tau_s = diag_stripe_steps(op, b.shape, shape, nd, tv or tgv, ratio, t)
        sigma_G = D.host_scalars(nd, True, ratio, t)[2]
        if tgv:
            sigma_p, sigma_q, tau_v = G.diag_scalars(nd, ratio, t)
    else:
        L_K = lipschitz(L_A, na, nd, regulariser, t)
        sigma, tau = P.scalars(None, nd, dtype=t, ratio=ratio, L_K=L_K)
        sigma_G = sigma_p = sigma_q = sigma
        tau_s = tau_v = tau
    theta = threshold(tau_s, mu, t)
    if tgv:
        r1, r0 = G.radii(lam, alpha1, alpha0, t)
    if state is not None:
        state.update(sigma=sigma, tau=tau, tau_s=tau_s, theta=theta)
    x = np.zeros(shape, t) if x0 is None else np.asarray(x0).astype(t)
    xbar = x.copy()
    y = np.zeros_like(b)
    s = np.zeros((nz, nu), t)
    sbar = s.copy()
    zeros = lambda count: [np.zeros(shape, t) for _ in range(count)]  # noqa: E731
    q = zeros(nd) if tv else []
    if tgv:
        p, q, v, vbar = zeros(nd), zeros(len(G.qkeys(nd))), zeros(nd), zeros(nd)
    for _ in range(iterations):
        r = np.asarray(op.fp(xbar)).astype(t, copy=False)
        y, part = sino_dual_stripe(y, r, b, sbar, fidelity, sigma)
        s, sbar = stripe_update(s, part, tau_s, theta)
        g = np.asarray(op.bp(y)).astype(t, copy=False)
        if tgv:
            p, q = G.tgv_dual(xbar, vbar, p, q, sigma_p, sigma_q, r1, r0)
            x, xbar, v, vbar = G.tgv_primal(x, g, v, p, q, tau, tau_v, nonneg)
        else:
            if tv:
                q = P.tv_dual(xbar, q, sigma_G, lam, methodTV)
            x, xbar = D.primal(x, g, q, tau, nonneg) if diagonal else P.primal(x, g, q, tau, nonneg)
        if state is not None:
            state.update(y=y, xbar=xbar, s=s, sbar=sbar, part=part, q=q)
            if tgv:
                state.update(p=p, v=v, vbar=vbar)
        yield x


def pdhg_stripe(op, b, L_A, iterations, **kw):
    """x after `iterations` iterations (the stripe variable: state["s"])"""
    out = None
    for out in pdhg_stripe_iterates(op, b, L_A, iterations=iterations, **kw):
        pass
    return out


def pdhg_stripe_many(op, b, L_A, counts, **kw):
    """{n: (x, s) after n iterations} for every n of `counts`, from ONE run"""
    counts = sorted(set(counts))
    state = kw.pop("state", None)
    state = {} if state is None else state
    out = {}
    for n, x in enumerate(pdhg_stripe_iterates(op, b, L_A, iterations=counts[-1], state=state, **kw), 1):
        if n in counts:
            out[n] = (x, state["s"])
    return out


# ------------------------------------------------------------------------------------------------ the objective (float64)
def objective(P64, x, s, b, mu, fidelity, regulariser=None, lam=None, methodTV=0, v=None, alpha1=1.0, alpha0=2.0):
    """F(A x + S s; b) + lambda R(x) + mu |s|_1 in float64 on the dense operator (TGV: at the given v)"""
    s = np.asarray(s, np.float64)
    value = P.data_term(P64.fp(x) + s[:, None, :], b, fidelity) + float(mu) * float(np.abs(s).sum())
    if regulariser == "TV":
        value += float(lam) * P.tv_seminorm(x, methodTV)
    elif regulariser == "TGV":
        value += float(lam) * G.tgv_term(x, v, alpha1, alpha0)
    return value


# ------------------------------------------------------------------------------------------------ the dense K = [[A, S], [grad, 0]]
def stripe_matrix(na, nu):
    """S of one slice as a dense float64 matrix [na nu, nu]: (S s)[a][u] = s[u]"""
    return np.tile(np.eye(nu), (na, 1))


def joint_matrix(A, na, nu, vol_shape, tv=True):
    """K = [[A, S], [grad, 0]] (without TV: [A, S]) of a 2D case, dense float64, on (x, s)"""
    top = np.hstack([A, stripe_matrix(na, nu)])
    if not tv:
        return top
    Gm = D.gradient_matrix(vol_shape)
    return np.vstack([top, np.hstack([Gm, np.zeros((Gm.shape[0], nu))])])
