"""TEST INFRASTRUCTURE: numpy restatement of the Diff4th regulariser (anisotropic fourth-order diffusion, explicit in time) of
docs/kernels/diff4th.md (the specification; there is no reference implementation to compare with -- formula-level parity,
unpinned).  This file holds the formula; tests/_march_oracle.py runs it (ORACLE below).  Shared by
tests/test_diff4th_oracle.py, tests/test_diff4th_slab_gloo.py (CPU) and tests/test_gpu_diff4th.py (MI355X).

Arrays are indexed [z][y][x]; component 1 <-> x (the fastest axis), 2 <-> y, 3 <-> z; 2D drops component 3.  Every neighbour
index is clamped per axis into the array.  With dtype = float32 every operation below is one float32 rounding in the order
the parentheses give (numpy never contracts to FMA, and its / is the correctly rounded division), which is what the kernel
reproduces bit for bit; dtype = float64 is the same algorithm in double."""
import numpy as np

from _march_oracle import Marcher, _sh

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


TOL_CASE = dict(shape=(7, 13, 37), pname="B", iterations=66, j=4)
TOL_CASE_SLAB = dict(shape=(9, 7, 11), pname="B", iterations=66, j=4)
# `stats`: stats["active", n] and stats["g_zero", n] = weighted's shares in iteration n (1-based)
ORACLE = Marcher("Diff4th", step, PARAMS, ("lam", "sigma", "tau"), GHOST, TOL_CASE, TOL_CASE_SLAB)
