"""TEST INFRASTRUCTURE: numpy restatement of PDHG with the second-order TGV term in its dual ("PD_TGV") as
docs/kernels/pdhg.md states it (the specification; there is no reference implementation to compare with -- formula-level
parity, unpinned).  Shared by tests/test_pdhg_tgv_oracle.py (CPU) and tests/test_gpu_pdhg_tgv.py (MI355X).

The conventions, the stencils, the sinogram dual and the float64 operator are those of tests/_pdhg_oracle.py (volumes are
[nz][ny][nx] arrays; component 1 <-> x, 2 <-> y, 3 <-> z; nd = 3 if nz > 1 else 2), the diagonal steps those of
tests/_pdhg_diag_oracle.py.  With dtype = float32 every operation below is one float32 rounding in the order the parentheses
give, which is what the kernels reproduce bit for bit; dtype = float64 is the same algorithm in double.  The Q fields travel
as a list in the order of the C-ABI: Q11, Q22, Q12 (, Q33, Q13, Q23)."""
import numpy as np

import _pdhg_diag_oracle as D
import _pdhg_oracle as P
from _pdhg_oracle import _axes, _B, _F, nd_of, rel_l2  # noqa: F401  (re-exported)

QKEYS = ((1, 1), (2, 2), (1, 2), (3, 3), (1, 3), (2, 3))


def qkeys(nd):
    return QKEYS[:6 if nd == 3 else 3]


def radii(lam, alpha1, alpha0, dtype=np.float32):
    """(r1, r0) = (lambda alpha1, lambda alpha0), one product each"""
    t = dtype
    return t(t(lam) * t(alpha1)), t(t(lam) * t(alpha0))


def scalars(L_A, nd, ratio=1.0, dtype=np.float32, L_K=None):
    """(sigma_P, sigma_Q, tau_x, tau_v) in `dtype` with scalar steps: L_K = L_A + L_R, L_R = 12 (nd = 2) or 16 (nd = 3),
    s = 0.95 / sqrt(L_K), sigma = s rho, tau = s / rho.  `L_K` given: taken as it is."""
    t = dtype
    if L_K is None:
        L_K = t(L_A) + t(16 if nd == 3 else 12)
    s = t(0.95) / np.sqrt(t(L_K))
    rho = t(ratio)
    sigma, tau = t(s * rho), t(s / rho)
    return sigma, sigma, tau, tau


def diag_scalars(nd, ratio=1.0, dtype=np.float32):
    """(sigma_P, sigma_Q, tau_v) of the diagonal preconditioner: a / 3, a / 2, t / (2 nd + 1)"""
    t = dtype
    a, tt, sigma_q, _ = D.host_scalars(nd, True, ratio, t)
    return t(a / t(3)), sigma_q, t(tt / t(2 * nd + 1))


# ------------------------------------------------------------------------------------------------ the two updates
def tgv_dual(xbar, vbar, p, q, sigma_p, sigma_q, r1, r0, stats=None):
    """step 4: returns the new (p, q).  `stats` (a dict) receives the shares of voxels on which the two projections changed
    their field: stats["n_gt_1"], stats["m_gt_1"]."""
    t = xbar.dtype.type
    sigma_p, sigma_q, r1, r0 = t(sigma_p), t(sigma_q), t(r1), t(r0)
    nd = len(p)
    ax = _axes(nd)
    comps = list(range(1, nd + 1))
    p = [p[d - 1] + sigma_p * (_F(xbar, ax[d]) - vbar[d - 1]) for d in comps]
    s = p[0] * p[0] + p[1] * p[1]
    if nd == 3:
        s = s + p[2] * p[2]
    n = np.sqrt(s) / r1
    act_n = n > t(1)
    den = np.where(act_n, n, t(1))
    p = [c / den for c in p]
    Q = dict(zip(qkeys(nd), q))
    for d, e in qkeys(nd):
        if d == e:
            Q[d, d] = Q[d, d] + sigma_q * _F(vbar[d - 1], ax[d])
        else:
            Q[d, e] = Q[d, e] + sigma_q * (t(0.5) * (_F(vbar[d - 1], ax[e]) + _F(vbar[e - 1], ax[d])))
    sd = Q[1, 1] * Q[1, 1] + Q[2, 2] * Q[2, 2]
    so = Q[1, 2] * Q[1, 2]
    if nd == 3:
        sd = sd + Q[3, 3] * Q[3, 3]
        so = (so + Q[1, 3] * Q[1, 3]) + Q[2, 3] * Q[2, 3]
    m = np.sqrt(sd + t(2) * so) / r0
    act_m = m > t(1)
    den = np.where(act_m, m, t(1))
    if stats is not None:
        stats["n_gt_1"], stats["m_gt_1"] = float(act_n.mean()), float(act_m.mean())
    return p, [Q[k] / den for k in qkeys(nd)]


def tgv_primal(x, g, v, p, q, tau_x, tau_v, nonneg):
    """step 5: returns (x', x-bar', v', v-bar').  `tau_x`: a scalar or an array like `x`."""
    t = x.dtype.type
    tau_x = tau_x if isinstance(tau_x, np.ndarray) else t(tau_x)
    if isinstance(tau_x, np.ndarray):
        assert tau_x.dtype == x.dtype and tau_x.shape == x.shape
    tau_v = t(tau_v)
    nd = len(p)
    ax = _axes(nd)
    comps = list(range(1, nd + 1))
    div = _B(p[0], ax[1]) + _B(p[1], ax[2])
    if nd == 3:
        div = div + _B(p[2], ax[3])
    xn = x - tau_x * (g - div)
    if nonneg:
        xn = np.where(xn < t(0), t(0), xn)
    xb = (xn + xn) - x
    Q = dict(zip(qkeys(nd), q))
    vn, vb = [], []
    for d in comps:
        acc = p[d - 1] + _B(Q[d, d], ax[d])
        for e in comps:
            if e != d:
                acc = acc + _B(Q[min(d, e), max(d, e)], ax[e])
        new = v[d - 1] + tau_v * acc
        vn.append(new)
        vb.append((new + new) - v[d - 1])
    return xn, xb, vn, vb


def march_steps(x0, g, state0, sigma_p, sigma_q, tau_x, tau_v, r1, r0, nonneg, counts, stats=None):
    """steps 4 and 5 alone, on a fixed `g`: {n: dict(x, xbar, v, vbar, p, q) after n steps} for every n of `counts`, from
    x = x-bar = x0 and `state0` = dict(v, vbar, p, q) (the kernel tests start from non-zero fields).  `stats`: the
    projections' shares in the FIRST step."""
    x = np.array(x0)
    xbar = x.copy()
    v, vbar, p, q = (list(state0[k]) for k in ("v", "vbar", "p", "q"))
    out = {}
    for n in range(1, max(counts) + 1):
        p, q = tgv_dual(xbar, vbar, p, q, sigma_p, sigma_q, r1, r0, stats if n == 1 else None)
        x, xbar, v, vbar = tgv_primal(x, g, v, p, q, tau_x, tau_v, nonneg)
        if n in counts:
            out[n] = dict(x=x, xbar=xbar, v=list(v), vbar=list(vbar), p=list(p), q=list(q))
    return out


# ------------------------------------------------------------------------------------------------ the loop
def pdhg_tgv_iterates(op, b, L_A=None, fidelity="LS", lam=0.001, alpha1=1.0, alpha0=2.0, nonneg=False, ratio=1.0, x0=None,
                      iterations=1, dtype=np.float32, nd=None, L_K=None, diagonal=False, state=None):
    """yields x after every iteration (a fresh array each time).  `op`: the operator pair (fp, bp) on [nz, n, n] volumes.
    `nd`, `L_K`: overrides (else from the volume and L_A).  `diagonal`: the diagonal preconditioner (L_A is not read).
    `state` (a dict) receives the arrays of the last iteration run: y, xbar, v, vbar, p, q (and sigma, tau at set-up)."""
    t = dtype
    b = np.asarray(b).astype(t)
    shape = (b.shape[0], op.n, op.n)
    nd = nd_of(shape) if nd is None else nd
    r1, r0 = radii(lam, alpha1, alpha0, t)
    if diagonal:
        sigma, tau_x, _ = D.step_arrays(op, b.shape, shape, nd, True, ratio, t)
        sigma_p, sigma_q, tau_v = diag_scalars(nd, ratio, t)
        if state is not None:
            state.update(sigma=sigma, tau=tau_x)
    else:
        sigma_p, sigma_q, tau_x, tau_v = scalars(L_A, nd, ratio, t, L_K)
        sigma = sigma_p
    x = np.zeros(shape, t) if x0 is None else np.asarray(x0).astype(t)
    xbar = x.copy()
    y = np.zeros_like(b)
    zeros = lambda count: [np.zeros(shape, t) for _ in range(count)]  # noqa: E731
    p, q, v, vbar = zeros(nd), zeros(len(qkeys(nd))), zeros(nd), zeros(nd)
    for _ in range(iterations):
        r = np.asarray(op.fp(xbar)).astype(t, copy=False)
        y = D.sino_dual(y, r, b, fidelity, sigma) if diagonal else P.sino_dual(y, r, b, fidelity, sigma)
        g = np.asarray(op.bp(y)).astype(t, copy=False)
        p, q = tgv_dual(xbar, vbar, p, q, sigma_p, sigma_q, r1, r0)
        x, xbar, v, vbar = tgv_primal(x, g, v, p, q, tau_x, tau_v, nonneg)
        if state is not None:
            state.update(y=y, xbar=xbar, v=v, vbar=vbar, p=p, q=q)
        yield x


def pdhg_tgv(op, b, L_A, iterations, **kw):
    """x after `iterations` iterations"""
    out = None
    for out in pdhg_tgv_iterates(op, b, L_A, iterations=iterations, **kw):
        pass
    return out


def pdhg_tgv_many(op, b, L_A, counts, **kw):
    """{n: x after n iterations} for every n of `counts`, from ONE run"""
    counts = sorted(set(counts))
    out = {}
    for n, x in enumerate(pdhg_tgv_iterates(op, b, L_A, iterations=counts[-1], **kw), 1):
        if n in counts:
            out[n] = x
    return out


# ------------------------------------------------------------------------------------------------ the objective (float64)
def tgv_term(x, v, alpha1, alpha0):
    """alpha1 sum |grad x - v|_2 + alpha0 sum |E v|_F in float64, the off-diagonal components of E v counted twice"""
    x = np.asarray(x, np.float64)
    nd = len(v)
    ax = _axes(nd)
    first = np.sqrt(sum((_F(x, ax[d]) - np.asarray(v[d - 1], np.float64)) ** 2 for d in range(1, nd + 1))).sum()
    sq = 0.0
    for d, e in qkeys(nd):
        vd, ve = np.asarray(v[d - 1], np.float64), np.asarray(v[e - 1], np.float64)
        sq = sq + (_F(vd, ax[d]) ** 2 if d == e else 2.0 * (0.5 * (_F(vd, ax[e]) + _F(ve, ax[d]))) ** 2)
    return float(alpha1 * first + alpha0 * np.sqrt(sq).sum())


def objective(P64, x, v, b, fidelity, lam, alpha1, alpha0):
    """F(Ax) + lambda (alpha1 |grad x - v| + alpha0 |E v|) in float64 on the dense operator"""
    return P.data_term(P64.fp(x), b, fidelity) + float(lam) * tgv_term(x, v, alpha1, alpha0)


# ------------------------------------------------------------------------------------------------ the dense block
def block_matrix(shape):
    """the regulariser block [[grad, -I], [0, E]] of a [nz, ny, nx] volume as one dense float64 matrix on (x, v_1 .. v_nd):
    the rows P_1 .. P_nd, then Q_de for every ORDERED pair (d, e) -- Q_de and Q_ed are the two rows the one stored field
    stands for, which is how the Frobenius norm counts it twice"""
    nd = nd_of(shape)
    nvox = int(np.prod(shape))
    G = D.gradient_matrix(shape)
    F = {d: G[(d - 1) * nvox:d * nvox] for d in range(1, nd + 1)}
    eye, zero = np.eye(nvox), np.zeros((nvox, nvox))
    rows = []
    for d in range(1, nd + 1):
        rows.append(np.hstack([F[d]] + [-eye if c == d else zero for c in range(1, nd + 1)]))
    for d in range(1, nd + 1):
        for e in range(1, nd + 1):
            cols = [zero] + [zero.copy() for _ in range(nd)]
            cols[d] = cols[d] + 0.5 * F[e]
            cols[e] = cols[e] + 0.5 * F[d]
            rows.append(np.hstack(cols))
    return np.vstack(rows)


def norm2(M):
    """the squared spectral norm, from the smaller Gram matrix"""
    gram = M.T @ M if M.shape[1] <= M.shape[0] else M @ M.T
    return float(np.linalg.eigvalsh(gram)[-1])
