"""TEST INFRASTRUCTURE: numpy restatement of SPDHG as docs/kernels/spdhg.md states it (the specification; there is no
reference implementation to compare with -- formula-level parity, unpinned).  Shared by tests/test_spdhg_oracle.py (CPU) and
tests/test_gpu_spdhg.py (MI355X).

The conventions are those of tests/_pdhg_oracle.py, from which the dual updates (``sino_dual``, ``tv_dual``), the axis map
and the objective are imported, not copied; ``_B`` / ``_F`` are the stencils of tests/_tgv_oracle.py.  With dtype = float32
every operation below is one float32 rounding in the order the parentheses give, which is what the kernels reproduce bit for
bit; dtype = float64 is the same algorithm in double.

The float32 form runs on ``MatchedProjector(..., os_number=m).fp / .bp(..., subset=j)``, the float64 form on `Subsets64`:
row blocks of the dense float64 matrix of the same forward projector."""
import numpy as np

import _matched_bp_oracle as M
from _pdhg_oracle import Dense64, _axes, nd_of, objective, rel_l2, sino_dual, tv_dual  # noqa: F401  (objective, rel_l2 re-exported)
from _tgv_oracle import _B, _F  # noqa: F401  (_F: what tv_dual applies; re-exported for the hand-written checks)


def n_blocks(m, tv):
    """E: the block updates of one epoch"""
    return 2 * m if tv else m


def draws(seed, m, tv, iterations):
    """the block sequence of a run: a value j < m selects subset j, a value j >= m the TV block"""
    E = n_blocks(m, tv)
    return np.random.default_rng(seed).integers(0, E, size=iterations * E)


def scalars(L, nd, m, tv=True, ratio=1.0, dtype=np.float32):
    """(sigma_A, sigma_G, tau, w_A, w_G) in `dtype`, formed as the specification forms them"""
    t = dtype
    E = n_blocks(m, tv)
    c, gamma = t(0.95), t(ratio)
    n_A, n_G = np.sqrt(t(L)), np.sqrt(t(4 * nd))
    sigma_A, sigma_G = (c * gamma) / n_A, (c * gamma) / n_G
    w_A, w_G = t(E), t(2)
    tau_A, tau_G = (c / gamma) / (w_A * n_A), (c / gamma) / (w_G * n_G)
    tau = min(tau_A, tau_G) if tv else tau_A
    return t(sigma_A), t(sigma_G), t(tau), w_A, w_G


# ------------------------------------------------------------------------------------------------ the two block updates
def sino_step(y, r, b, fidelity, sigma):
    """subset step 2: (the new y_j, d = its change)"""
    v = sino_dual(y, r, b, fidelity, sigma)
    return v, v - y


def primal_step(x, z, delta, tau, w, nonneg):
    """subset step 4: (x', z')"""
    t = x.dtype.type
    zn = z + delta
    zb = zn + t(w) * delta
    xn = x - t(tau) * zb
    if nonneg:
        xn = np.where(xn < t(0), t(0), xn)
    return xn, zn


def tv_dual_step(x, q, sigma, lam, methodTV, stats=None):
    """TV step 1: (the new q, e = its change), lists of nd arrays"""
    p = tv_dual(x, q, sigma, lam, methodTV, stats)
    return p, [pd - qd for pd, qd in zip(p, q)]


def divergence(e):
    """(B_1(e1) + B_2(e2)) + B_3(e3); for nd = 2 the first two"""
    ax = _axes(len(e))
    div = _B(e[0], ax[1]) + _B(e[1], ax[2])
    if len(e) == 3:
        div = div + _B(e[2], ax[3])
    return div


def tv_primal_step(x, z, e, tau, w, nonneg):
    """TV steps 2 and 3: (x', z')"""
    t = x.dtype.type
    div = divergence(e)
    zn = z - div
    zb = zn - t(w) * div
    xn = x - t(tau) * zb
    if nonneg:
        xn = np.where(xn < t(0), t(0), xn)
    return xn, zn


def tv_steps(x0, z0, sigma, tau, lam, methodTV, nonneg, counts, w=2.0, stats=None):
    """TV updates alone, from q = 0: {n: (x, z, q, e) after n updates} for every n of `counts` (the kernel tests).
    `stats`: the projection's share in the FIRST update."""
    x, z = np.array(x0), np.array(z0)
    q = [np.zeros_like(x) for _ in range(nd_of(x.shape))]
    out = {}
    for n in range(1, max(counts) + 1):
        q, e = tv_dual_step(x, q, sigma, lam, methodTV, stats if n == 1 else None)
        x, z = tv_primal_step(x, z, e, tau, w, nonneg)
        if n in counts:
            out[n] = (x, z, list(q), list(e))
    return out


# ------------------------------------------------------------------------------------------------ the loop
def spdhg_iterates(P, b, L, m, fidelity="LS", lam=None, methodTV=0, nonneg=False, ratio=1.0, x0=None, iterations=1, seed=0,
                   dtype=np.float32, state=None):
    """yields x after every epoch (a fresh array each time).  `P`: an operator pair with fp(x, subset=j), bp(d, subset=j)
    and the list `subsets` of angle-index arrays, for m subsets; `b`: the full sinogram [nz, angles, nu]; `lam` None: no TV
    block.  `state` (a dict) receives the arrays after the last epoch run -- y (a list), q, z -- and the counts of subset
    and TV updates so far: "block_updates"."""
    t = dtype
    b = np.asarray(b).astype(t)
    assert len(P.subsets) == m
    shape = (b.shape[0], P.n, P.n)
    nd = nd_of(shape)
    tv = lam is not None
    E = n_blocks(m, tv)
    sigma_A, sigma_G, tau, w_A, w_G = scalars(L, nd, m, tv, ratio, t)
    seq = draws(seed, m, tv, iterations)
    bs = [np.ascontiguousarray(b[:, idx, :]) for idx in P.subsets]
    x = np.zeros(shape, t) if x0 is None else np.asarray(x0).astype(t)
    if nonneg:
        x = np.where(x < t(0), t(0), x)       # SPDHG's first primal step with z-bar = 0
    z = np.zeros(shape, t)
    y = [np.zeros_like(bj) for bj in bs]
    q = [np.zeros(shape, t) for _ in range(nd)] if tv else []
    done = [0, 0]
    for epoch in range(iterations):
        for j in seq[epoch * E:(epoch + 1) * E]:
            if j < m:
                r = np.asarray(P.fp(x, subset=j)).astype(t, copy=False)
                y[j], d = sino_step(y[j], r, bs[j], fidelity, sigma_A)
                delta = np.asarray(P.bp(d, subset=j)).astype(t, copy=False)
                x, z = primal_step(x, z, delta, tau, w_A, nonneg)
            else:
                q, e = tv_dual_step(x, q, sigma_G, lam, methodTV)
                x, z = tv_primal_step(x, z, e, tau, w_G, nonneg)
            done[int(j >= m)] += 1
        if state is not None:
            state.update(y=list(y), q=list(q), z=z, block_updates=tuple(done))
        yield x


def spdhg(P, b, L, m, iterations, **kw):
    """x after `iterations` epochs"""
    out = None
    for out in spdhg_iterates(P, b, L, m, iterations=iterations, **kw):
        pass
    return out


def spdhg_many(P, b, L, m, counts, **kw):
    """{n: x after n epochs} for every n of `counts`, from ONE run"""
    counts = sorted(set(counts))
    out = {}
    for n, x in enumerate(spdhg_iterates(P, b, L, m, iterations=counts[-1], **kw), 1):
        if n in counts:
            out[n] = x
    return out


# ------------------------------------------------------------------------------------------------ the operators
def matched(nz, n, nu, angles, m, cor=0.0):
    """the float32 pair: the C oracle's forward projector and the float32 restatement of its exact transpose, m subsets"""
    return M.MatchedProjector(nz, n, nu, angles, cor, m)


class Subsets64:
    """Row blocks of a `Dense64`: subset j is the rows of its angles (the interleaved table of the oracle, trim included)."""

    def __init__(self, dense: Dense64, m):
        self.dense, self.n, self.nu = dense, dense.n, dense.nu
        self.subsets = list(M.O.os_indices(dense.na, m)[2]) if m > 1 else [np.arange(dense.na, dtype=np.int64)]
        self.blocks = [dense.A[(idx[:, None] * self.nu + np.arange(self.nu)[None, :]).ravel()] for idx in self.subsets]

    def fp(self, vol, subset):
        vol = np.asarray(vol, np.float64)
        return (vol.reshape(vol.shape[0], -1) @ self.blocks[subset].T).reshape(vol.shape[0], len(self.subsets[subset]), self.nu)

    def bp(self, sino, subset):
        sino = np.asarray(sino, np.float64)
        return (sino.reshape(sino.shape[0], -1) @ self.blocks[subset]).reshape(sino.shape[0], self.n, self.n)

    def norm2(self, subset):
        """the largest eigenvalue of A_j^T A_j"""
        return float(np.linalg.norm(self.blocks[subset], 2) ** 2)
