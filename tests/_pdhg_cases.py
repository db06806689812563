"""TEST INFRASTRUCTURE shared by tests/test_pdhg_oracle.py (CPU) and tests/test_gpu_pdhg.py (MI355X): the inputs of the PDHG
tests -- seeded phantom, noise, lambda -- and the oracle's runs on them, computed once per session and never modified.
Nothing here is a tolerance: the cases are inputs, chosen before the code under test existed and recorded with what the
float64 oracle gives on them (docs/kernels/pdhg.md carries the figures)."""
import functools

import numpy as np

import _matched_bp_oracle as M
import _pdhg_oracle as P

N, NU, NA, NZ = 32, 32, 24, 3
ANGLES = np.linspace(0.0, np.pi, NA, endpoint=False)
COUNTS = (10, 100, 300)            # float32 against float64
CHECKPOINTS = (10, 30, 100, 300)   # the objective


def phantom(nz=NZ, n=N, seed=21, floor=0.0):
    """background 0.1 inside the inscribed disc, plus five seeded rectangles of height 0.2 .. 1 that stay inside it and
    shift by one voxel per plane, plus `floor` everywhere (the KL input: every ray then meets a positive voxel):
    piecewise constant, non-negative, float64"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:n, :n]
    disc = (xx - n / 2 + 0.5) ** 2 + (yy - n / 2 + 0.5) ** 2 <= (0.45 * n) ** 2
    vol = np.zeros((nz, n, n))
    boxes = [(rng.integers(n // 4, n // 2), rng.integers(n // 4, n // 2), rng.integers(3, n // 4), rng.integers(3, n // 4),
              rng.uniform(0.2, 1.0)) for _ in range(5)]
    for z in range(nz):
        plane = 0.1 * disc
        for y0, x0, h, w, v in boxes:
            plane[y0 + z:y0 + z + h, x0:x0 + w] += v
        vol[z] = plane * disc + floor
    return vol


@functools.lru_cache(maxsize=None)
def dense(n=N, nu=NU):
    return P.Dense64(n, nu, ANGLES, 0.0)


@functools.lru_cache(maxsize=None)
def matched(nz=NZ, n=N, nu=NU):
    return M.MatchedProjector(nz, n, nu, ANGLES, 0.0)


@functools.lru_cache(maxsize=None)
def lipschitz(n=N, nu=NU):
    """L_A: the largest eigenvalue of A^T A of the dense float64 matrix"""
    return dense(n, nu).norm2()


@functools.lru_cache(maxsize=None)
def sinogram(nz=NZ, noise=0.3, seed=22, positive=False):
    """A x* + Gaussian noise of standard deviation `noise`, float32; `positive` (the KL input): x* has the floor 0.1 and
    the data are clamped at 0.05"""
    b = dense().fp(phantom(nz, floor=0.1 if positive else 0.0)) + noise * np.random.default_rng(seed).standard_normal((nz, NA, NU))
    if positive:
        b = np.maximum(b, 0.05)
    b = np.ascontiguousarray(b.astype(np.float32))
    b.setflags(write=False)
    return b


# name -> the keyword arguments of pdhg_iterates and whether the data are clamped positive
CASES = {
    "LS+TV": (dict(fidelity="LS", lam=0.5), False),
    "L1+TV": (dict(fidelity="L1", lam=0.5), False),
    "KL+TV": (dict(fidelity="KL", lam=0.05, nonneg=True), True),
    "LS": (dict(fidelity="LS", lam=None), False),
}


@functools.lru_cache(maxsize=None)
def run(name, dtype_name, counts):
    """{n: x after n iterations} of a case in float32 (on the C oracle's fp and the float32 A^T) or float64 (dense)"""
    kw, positive = CASES[name]
    op = matched() if dtype_name == "float32" else dense()
    res = P.pdhg_many(op, sinogram(positive=positive), lipschitz(), counts, dtype=np.dtype(dtype_name).type, **kw)
    for v in res.values():
        v.setflags(write=False)
    return res


# ------------------------------------------------------------------------------------------------ zingers
ZINGER_LAMBDAS = (0.5, 1.0, 2.0, 4.0, 8.0)
ZINGER_L1_LAMBDA = 0.5
ZINGER_ITERATIONS = 1000


@functools.lru_cache(maxsize=None)
def zinger_sinogram(seed=23):
    """the noisy 2D sinogram with +40 on 2 % of its samples"""
    b = np.array(sinogram(1), np.float64)
    hit = np.random.default_rng(seed).random(b.shape) < 0.02
    return b + 40.0 * hit


def rel_error(x, ref):
    return float(np.linalg.norm(np.ravel(x) - np.ravel(ref)) / np.linalg.norm(np.ravel(ref)))


@functools.lru_cache(maxsize=None)
def zinger_errors():
    """(relative error of L1 + TV, {lambda: relative error of LS + TV}) against the phantom after 1000 float64 iterations"""
    truth, b = phantom(1), zinger_sinogram()
    go = lambda fid, lam: rel_error(P.pdhg(dense(), b, lipschitz(), ZINGER_ITERATIONS, fidelity=fid, lam=lam,  # noqa: E731
                                           dtype=np.float64), truth)
    return go("L1", ZINGER_L1_LAMBDA), {lam: go("LS", lam) for lam in ZINGER_LAMBDAS}


# ------------------------------------------------------------------------------------------------ the kernel tests
# steps 4 and 5 on a fixed g (tests/test_gpu_pdhg.py): the two marches run TGV's tile -- 63 columns per wave, 4 rows per
# lane, 2 x 2 waves = 126 x 8 voxels per workgroup, z-chunks of at least 16 planes (tests/_edge_shapes.LAUNCHES["tgv"])
MARCH_SHAPES = tuple(dict.fromkeys(
    [(1, 9, 70), (7, 1, 70), (7, 9, 1)]                                   # a dimension of 1 (the first runs nd = 2)
    + [(3, 5, w) for w in (62, 63, 64, 125, 126, 127)]                    # the wave's / the workgroup's last column +- 1
    + [(3, h, 64) for h in (3, 4, 5, 7, 8, 9)]                            # the lane's / the workgroup's last row +- 1
    + [(d, 9, 11) for d in (15, 16, 17, 33, 49)]                          # 1, 1, 2, 3 and 4 z-chunks
    + [(33, 1, 8 * 126 + 1)]))                                            # nine workgroup tiles, three z-chunks
MARCH_COUNTS = (1, 2, 5)
MARCH_SIGMA, MARCH_TAU = np.float32(0.25), np.float32(0.2)
MARCH_LAMBDA = {"noise": np.float32(0.035), "terraces": np.float32(1.0)}   # noise: the projection is on for 10-90 % of the voxels


def march_input(kind, shape):
    import _edge_shapes as E
    return E.step_noise(shape) if kind == "noise" else E.terraces(shape, block=4)


def march_g(shape):
    return (0.5 * np.random.default_rng(9).standard_normal(shape)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def march_oracle(kind, shape, methodTV, nonneg):
    """({n: (x, x-bar, q)}, the share of voxels the projection of step 4 changed in the first step)"""
    stats = {}
    res = P.march_steps(march_input(kind, shape), march_g(shape), MARCH_SIGMA, MARCH_TAU, MARCH_LAMBDA[kind], methodTV, nonneg,
                        MARCH_COUNTS, stats=stats)
    for x, xbar, q in res.values():
        for arr in (x, xbar, *q):
            arr.setflags(write=False)
    return res, stats["active"]
