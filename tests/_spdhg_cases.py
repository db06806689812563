"""TEST INFRASTRUCTURE shared by tests/test_spdhg_oracle.py (CPU) and tests/test_gpu_spdhg.py (MI355X): the inputs of the
SPDHG tests -- those of tests/_pdhg_cases.py (phantom, sinograms, lambdas, march shapes), the subset counts and seeds -- and
the oracle's runs on them, computed once per session and never modified.  Nothing here is a tolerance: the cases are inputs,
recorded with what the float64 oracle gives on them (docs/kernels/spdhg.md carries the figures)."""
import functools

import numpy as np

import _pdhg_cases as K
import _spdhg_oracle as S

COUNTS = (10, 100)              # epochs: float32 against float64, and the objective
SEED = 0
# name (a case of _pdhg_cases.CASES) -> the number of subsets its runs use
SUBSETS = {"LS+TV": 8, "L1+TV": 8, "KL+TV": 4, "LS": 8}


@functools.lru_cache(maxsize=None)
def matched(m, nz=K.NZ):
    return S.matched(nz, K.N, K.NU, K.ANGLES, m)


@functools.lru_cache(maxsize=None)
def dense(m):
    return S.Subsets64(K.dense(), m)


@functools.lru_cache(maxsize=None)
def subset_norms(m):
    """|A_j|^2 of every subset: the largest eigenvalues of the row blocks of the dense float64 matrix"""
    return tuple(dense(m).norm2(j) for j in range(m))


def lipschitz(m):
    """L: the largest of them"""
    return max(subset_norms(m))


@functools.lru_cache(maxsize=None)
def run(name, dtype_name, m=None, counts=COUNTS, seed=SEED):
    """({n: x after n epochs}, the state after the last) of a case in float32 (on the C oracle's fp and the float32 A^T) or
    float64 (row blocks of the dense matrix)"""
    kw, positive = K.CASES[name]
    m = SUBSETS[name] if m is None else m
    op = matched(m) if dtype_name == "float32" else dense(m)
    state = {}
    res = S.spdhg_many(op, K.sinogram(positive=positive), lipschitz(m), m, counts, dtype=np.dtype(dtype_name).type, seed=seed,
                       state=state, **kw)
    for v in res.values():
        v.setflags(write=False)
    return res, state


# ------------------------------------------------------------------------------------------------ the kernel tests
# the TV pair on the shapes, inputs, lambdas and step sizes of the PDHG marches (same tile); z starts as seeded noise
TV_W = np.float32(2)
PRIMAL_WEIGHTS = (np.float32(4), np.float32(24))


def tv_z0(shape):
    return (0.5 * np.random.default_rng(9).standard_normal(shape)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def tv_oracle(kind, shape, methodTV, nonneg):
    """({n: (x, z, q, e) after n TV updates}, the share of voxels the projection changed in the first)"""
    stats = {}
    res = S.tv_steps(K.march_input(kind, shape), tv_z0(shape), K.MARCH_SIGMA, K.MARCH_TAU, K.MARCH_LAMBDA[kind], methodTV,
                     nonneg, K.MARCH_COUNTS, TV_W, stats)
    for x, z, q, e in res.values():
        for arr in (x, z, *q, *e):
            arr.setflags(write=False)
    return res, stats["active"]
