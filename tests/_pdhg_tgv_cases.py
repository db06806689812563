"""TEST INFRASTRUCTURE shared by tests/test_pdhg_tgv_oracle.py (CPU) and tests/test_gpu_pdhg_tgv.py (MI355X): the inputs of
the PD_TGV tests on the geometry of tests/_pdhg_cases.py and the oracle's runs on them, computed once per session and never
modified.  Nothing here is a tolerance: the cases are inputs, chosen before the code under test existed and recorded with
what the float64 oracle gives on them (docs/kernels/pdhg.md carries the figures)."""
import functools

import numpy as np

import _pdhg_cases as K
import _pdhg_oracle as P
import _pdhg_tgv_oracle as G

# name -> the keyword arguments of pdhg_tgv_iterates and whether the data are clamped positive
CASES = {
    "LS+TGV": (dict(fidelity="LS", lam=0.5, alpha1=1.0, alpha0=2.0), False),
    "L1+TGV": (dict(fidelity="L1", lam=0.5, alpha1=1.0, alpha0=2.0), False),
    "KL+TGV": (dict(fidelity="KL", lam=0.05, alpha1=1.0, alpha0=2.0, nonneg=True), True),
}


@functools.lru_cache(maxsize=None)
def run(name, dtype_name, counts, diagonal=False):
    """({n: x after n iterations}, the state after the last) of a case in float32 (on the C oracle's fp and the float32
    A^T) or float64 (dense)"""
    kw, positive = CASES[name]
    op = K.matched() if dtype_name == "float32" else K.dense()
    state = {}
    res = G.pdhg_tgv_many(op, K.sinogram(positive=positive), K.lipschitz(), counts, dtype=np.dtype(dtype_name).type,
                          diagonal=diagonal, state=state, **kw)
    for v in res.values():
        v.setflags(write=False)
    return res, state


# ------------------------------------------------------------------------------------------------ the staircase case
STAIR_TGV = dict(lam=0.25, alpha1=1.0, alpha0=2.0)
STAIR_TV_LAMBDAS = (0.05, 0.1, 0.25, 0.5, 1.0)
STAIR_ITERATIONS = 1000


def stair_phantom(n=K.N):
    """piecewise affine, 2D: inside the inscribed disc a ramp along x on the left half, a plateau on the upper right and a
    ramp along y on the lower right; float64 [1, n, n]"""
    yy, xx = np.mgrid[:n, :n]
    disc = (xx - n / 2 + 0.5) ** 2 + (yy - n / 2 + 0.5) ** 2 <= (0.45 * n) ** 2
    plane = np.where(xx < n // 2, 0.2 + 1.6 * xx / n, np.where(yy < n // 2, 0.6, 1.4 - 1.6 * (yy - n // 2) / n))
    return (plane * disc)[None]


@functools.lru_cache(maxsize=None)
def stair_sinogram(noise=0.1, seed=24):
    b = K.dense().fp(stair_phantom()) + noise * np.random.default_rng(seed).standard_normal((1, K.NA, K.NU))
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def stair_errors():
    """(relative error of LS + TGV, {lambda: relative error of LS + TV}) against the phantom after 1000 float64 iterations"""
    truth, b = stair_phantom(), stair_sinogram()
    tgv = G.pdhg_tgv(K.dense(), b, K.lipschitz(), STAIR_ITERATIONS, dtype=np.float64, **STAIR_TGV)
    tv = {lam: K.rel_error(P.pdhg(K.dense(), b, K.lipschitz(), STAIR_ITERATIONS, fidelity="LS", lam=lam, dtype=np.float64), truth)
          for lam in STAIR_TV_LAMBDAS}
    return K.rel_error(tgv, truth), tv


# ------------------------------------------------------------------------------------------------ scalar against diagonal steps
RATE_REFERENCE, RATE_LIMIT = 6000, 2500


@functools.lru_cache(maxsize=None)
def iterations_to_one_percent(name):
    """(scalar steps, diagonal steps): the first iteration of the 2D float64 run of a case whose iterate lies within 1 %
    (relative L2) of the iterate after 6000 iterations with scalar steps; None where 2500 iterations do not get there"""
    kw, positive = CASES[name]
    b = K.sinogram(1, positive=positive)
    ref = G.pdhg_tgv(K.dense(), b, K.lipschitz(), RATE_REFERENCE, dtype=np.float64, **kw)
    out = []
    for diagonal in (False, True):
        its = G.pdhg_tgv_iterates(K.dense(), b, K.lipschitz(), iterations=RATE_LIMIT, dtype=np.float64, diagonal=diagonal, **kw)
        out.append(next((n for n, x in enumerate(its, 1) if G.rel_l2(x, ref) <= 0.01), None))
    return tuple(out)


# ------------------------------------------------------------------------------------------------ the kernel tests
# steps 4 and 5 on a fixed g (tests/test_gpu_pdhg_tgv.py) on K.MARCH_SHAPES.  Four different steps: a swap changes bits.
MARCH_SIGMA_P, MARCH_SIGMA_Q = np.float32(0.25), np.float32(0.3125)
MARCH_TAU_X, MARCH_TAU_V = np.float32(0.2), np.float32(0.15)
# noise: both projections change between 10 % and 90 % of the voxels in the first step
MARCH_RADII = {"noise": (np.float32(0.09), np.float32(0.18)), "terraces": (np.float32(1.0), np.float32(2.0))}


def nq_of(nd):
    return 6 if nd == 3 else 3


def march_state(shape):
    """seeded non-zero v, v-bar, P, Q: the first step exercises every term"""
    rng = np.random.default_rng(11)
    nd = P.nd_of(shape)
    field = lambda scale: (scale * rng.standard_normal(shape)).astype(np.float32)  # noqa: E731
    return dict(v=[field(0.1) for _ in range(nd)], vbar=[field(0.1) for _ in range(nd)],
                p=[field(0.05) for _ in range(nd)], q=[field(0.05) for _ in range(nq_of(nd))])


def march_tau(shape):
    """a seeded step field spanning 0.05 ... 0.5"""
    tau = np.random.default_rng(10).uniform(0.05, 0.5, shape).astype(np.float32)
    tau.flat[-2:] = 0.05, 0.5
    return tau


@functools.lru_cache(maxsize=None)
def march_oracle(kind, shape, nonneg, per_voxel):
    """({n: the fields after n steps}, the shares of voxels the two projections changed in the first step)"""
    stats = {}
    r1, r0 = MARCH_RADII[kind]
    tau_x = march_tau(shape) if per_voxel else MARCH_TAU_X
    res = G.march_steps(K.march_input(kind, shape), K.march_g(shape), march_state(shape), MARCH_SIGMA_P, MARCH_SIGMA_Q, tau_x,
                        MARCH_TAU_V, r1, r0, nonneg, K.MARCH_COUNTS, stats=stats)
    for fields in res.values():
        for arr in (fields["x"], fields["xbar"], *fields["v"], *fields["vbar"], *fields["p"], *fields["q"]):
            arr.setflags(write=False)
    return res, (stats["n_gt_1"], stats["m_gt_1"])
