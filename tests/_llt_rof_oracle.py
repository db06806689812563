"""TEST INFRASTRUCTURE: numpy restatement of the LLT_ROF regulariser (ROF total variation plus the fourth-order
Lysaker-Lundervold-Tai term, explicit in time) of docs/kernels/llt_rof.md (the specification; there is no reference
implementation to compare with -- formula-level parity, unpinned).  This file holds the formula; tests/_march_oracle.py runs it (ORACLE below).
Shared by tests/test_llt_rof_oracle.py, tests/test_llt_rof_slab_gloo.py (CPU), tests/test_gpu_llt_rof.py and
tests/test_gpu_llt_rof_edges.py (MI355X).

Arrays are indexed [z][y][x]; component 1 <-> x (the fastest axis), 2 <-> y, 3 <-> z; 2D drops component 3.  Every neighbour
index of U is clamped per axis into the array.  With dtype = float32 every operation below is one float32 rounding in the
order the parentheses give (numpy never contracts to FMA, and its / and sqrt are the correctly rounded ones), which is what
the kernel reproduces bit for bit; dtype = float64 is the same algorithm in double."""
import numpy as np

from _march_oracle import Marcher, _sh

GHOST = 2   # ghost planes of U per interior boundary of a z-slab
EPS = np.float32(1e-8)
# Chosen on the CPU (tests/test_llt_rof_oracle.py asserts it): on (7, 13, 37) and (13, 37) float32 stays within 5e-6 of
# float64 over 40 iterations, and both terms change the result in the first and in the 40th iteration.
PARAMS = {
    "A": dict(lam_rof=0.3, lam_llt=0.1, tau=0.02),
    "B": dict(lam_rof=0.05, lam_llt=0.15, tau=0.01),
    "C": dict(lam_rof=1.0, lam_llt=0.02, tau=0.005),
}


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


TOL_CASE = dict(shape=(7, 13, 37), pname="A", iterations=66, j=4)
TOL_CASE_SLAB = dict(shape=(9, 7, 11), pname="A", iterations=66, j=4)
# `stats`: stats["s_zero", n] and stats["h1_tiny", n] = step's shares entering iteration n (1-based); the scalars pass
# through float32 whatever the dtype (narrow)
ORACLE = Marcher("LLT_ROF", step, PARAMS, ("lam_rof", "lam_llt", "tau"), GHOST, TOL_CASE, TOL_CASE_SLAB, narrow=True)
