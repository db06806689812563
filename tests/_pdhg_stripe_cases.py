"""TEST INFRASTRUCTURE shared by tests/test_pdhg_stripe_oracle.py (CPU) and tests/test_gpu_pdhg_stripe.py (MI355X): the inputs
of the tests of PDHG's stripe variable on the geometry of tests/_pdhg_cases.py and the oracle's runs on them, computed once
per session and never modified.  Nothing here is a tolerance: the cases are inputs, recorded with what the float64 oracle
gives on them (docs/kernels/pdhg.md carries the figures)."""
import functools

import numpy as np

import _pdhg_cases as K
import _pdhg_oracle as P
import _pdhg_stripe_oracle as S

MU = 3.0

# ------------------------------------------------------------------------------------------------ float32 against float64
# the 32^2 x 3 sinograms of tests/_pdhg_cases.py with three offsets planted per plane (positive, so that the KL data stay so)
PLANTED_COLUMNS, PLANTED_OFFSETS = (5, 14, 23), (2.0, 3.0, 4.0)


def planted(nz=K.NZ, nu=K.NU):
    s = np.zeros((nz, nu))
    for z in range(nz):
        for c, v in zip(PLANTED_COLUMNS, PLANTED_OFFSETS):
            s[z, c + z] = v
    return s


@functools.lru_cache(maxsize=None)
def sinogram(nz=K.NZ, positive=False):
    b = np.ascontiguousarray((K.sinogram(nz, positive=positive) + planted(nz)[:, None, :]).astype(np.float32))
    b.setflags(write=False)
    return b


# name -> the keyword arguments of pdhg_stripe_iterates and whether the data are clamped positive.  mu: the derivative of the
# KL term in a sample, 1 - b / (Ax + s), is below 1 in size where the other two terms' grows with the offset, so the weight
# at which the variable still takes a planted offset is smaller there
CASES = {
    "LS+TV": (dict(mu=MU, fidelity="LS", regulariser="TV", lam=0.5), False),
    "L1+TV": (dict(mu=MU, fidelity="L1", regulariser="TV", lam=0.5), False),
    "KL+TV": (dict(mu=0.3, fidelity="KL", regulariser="TV", lam=0.05, nonneg=True), True),
    "LS+TGV": (dict(mu=MU, fidelity="LS", regulariser="TGV", lam=0.5, alpha1=1.0, alpha0=2.0), False),
}


@functools.lru_cache(maxsize=None)
def run(name, dtype_name, counts, diagonal=False):
    """{n: (x, s) after n iterations} of a case in float32 (on the C oracle's fp and the float32 A^T) or float64 (dense)"""
    kw, positive = CASES[name]
    op = K.matched() if dtype_name == "float32" else K.dense()
    res = S.pdhg_stripe_many(op, sinogram(positive=positive), K.lipschitz(), counts, dtype=np.dtype(dtype_name).type,
                             diagonal=diagonal, **kw)
    for x, s in res.values():
        x.setflags(write=False)
        s.setflags(write=False)
    return res


# ------------------------------------------------------------------------------------------------ the striped case
# 32^2, a detector of 48 pixels, 24 angles, Gaussian noise of 0.3, four offsets planted; LS + TV, lambda = 0.5, mu = 3,
# 1000 float64 iterations, against LS + TV without the variable over a grid of lambda
STRIPE_NU = 48
STRIPE_COLUMNS, STRIPE_OFFSETS = (9, 20, 27, 38), (2.0, -3.0, 4.0, -2.5)
STRIPE_HALF = 0.5 * min(abs(v) for v in STRIPE_OFFSETS)   # half the smallest planted amplitude
STRIPE_LAMBDA, STRIPE_ITERATIONS = 0.5, 1000
PLAIN_LAMBDAS = (0.25, 0.5, 1.0, 2.0, 4.0)


@functools.lru_cache(maxsize=None)
def stripe_sinograms(noise=0.3, seed=31):
    """(the sinogram with the four offsets, the same without them), float64 [1, 24, 48]"""
    clean = K.dense(K.N, STRIPE_NU).fp(K.phantom(1)) + noise * np.random.default_rng(seed).standard_normal((1, K.NA, STRIPE_NU))
    s = np.zeros((1, STRIPE_NU))
    s[0, list(STRIPE_COLUMNS)] = STRIPE_OFFSETS
    striped = clean + s[:, None, :]
    for a in (clean, striped):
        a.setflags(write=False)
    return striped, clean


@functools.lru_cache(maxsize=None)
def stripe_errors():
    """{"striped" / "clean": (relative error with the variable, s, {lambda: relative error without it})} against the phantom"""
    op, L_A, truth = K.dense(K.N, STRIPE_NU), K.lipschitz(K.N, STRIPE_NU), K.phantom(1)
    out = {}
    for name, b in zip(("striped", "clean"), stripe_sinograms()):
        state = {}
        x = S.pdhg_stripe(op, b, L_A, STRIPE_ITERATIONS, mu=MU, fidelity="LS", regulariser="TV", lam=STRIPE_LAMBDA,
                          dtype=np.float64, state=state)
        plain = {lam: K.rel_error(P.pdhg(op, b, L_A, STRIPE_ITERATIONS, fidelity="LS", lam=lam, dtype=np.float64), truth)
                 for lam in PLAIN_LAMBDAS}
        out[name] = (K.rel_error(x, truth), state["s"], plain)
    return out


# ------------------------------------------------------------------------------------------------ the kernel tests
# tests/test_gpu_pdhg_stripe.py: both launches on seeded arrays; the segment length is 64 rows, a lane owns 4 columns, a
# workgroup 256
KERNEL_NA = (1, 63, 64, 65, 130)
KERNEL_NU = (1, 3, 4, 5, 64, 257)
KERNEL_NZ = (1, 3)
KERNEL_SIGMA, KERNEL_TAU_S, KERNEL_THETA = np.float32(0.3125), np.float32(0.0625), np.float32(0.5)


def kernel_inputs(nz, na, nu, seed=5):
    """(y, r, b, sigma_i, s-bar): seeded float32 arrays; b has negative samples (the KL clamp), the L1 clip is reached on a
    share of the samples"""
    rng = np.random.default_rng([seed, nz, na, nu])
    f = lambda *shape, scale=1.0: (scale * rng.standard_normal(shape)).astype(np.float32)  # noqa: E731
    y, r, b = f(nz, na, nu, scale=0.6), f(nz, na, nu, scale=2.0) + np.float32(1.0), f(nz, na, nu, scale=2.0) + np.float32(1.0)
    sig = rng.uniform(0.05, 1.5, (nz, na, nu)).astype(np.float32)
    return y, r, b, sig, f(nz, nu, scale=0.5)


def update_inputs(nz, na, nu, seed=6):
    """(s, part) for step 6 with KERNEL_TAU_S and KERNEL_THETA = 0.5: `part` holds small integers and `s` multiples of 1/16,
    so w = s - c / 16 is exact; the first elements are set so that w is exactly +theta, -theta, inside the dead zone, +0,
    just outside on either side (the comparisons are strict: w = +-theta gives +0)"""
    rng = np.random.default_rng([seed, nz, na, nu])
    k = S.n_seg(na)
    part = rng.integers(-3, 4, (k, nz, nu)).astype(np.float32)
    s = (rng.integers(-24, 25, (nz, nu)) / 16.0).astype(np.float32)
    want_w = [0.5, -0.5, 0.25, 0.0, 0.5 + 2.0 ** -20, -0.5 - 2.0 ** -20, -0.25]
    flat_s, c = s.reshape(-1), part.sum(axis=0).reshape(-1)
    for i, w in enumerate(want_w[:flat_s.size]):
        flat_s[i] = np.float32(w + float(KERNEL_TAU_S) * float(c[i]))
    return s, part
