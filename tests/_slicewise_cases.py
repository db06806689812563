"""TEST INFRASTRUCTURE shared by tests/test_slicewise.py (CPU) and tests/test_gpu_slicewise.py (MI355X): the inputs, the
shapes, the per-slice oracle and the tolerance cases of the slice-wise PD_TV / ROF_TV (docs/kernels/slicewise.md).

Shapes are (nz, ny, nx) and come from the tiles of tomobar_amd/csrc/tv_slices.hip, the way tests/_edge_shapes.py derives its
own: a PD_TV wave owns 8 rows x 58 / 60 / 62 columns (3 / 2 / 1 iterations per launch), a ROF_TV wave 8 rows x 60 columns,
four waves make a workgroup, and the tile index runs over (slice, tile row, tile column).  So: widths one below, at and one
above a tile (57, 58, 59; 59, 60, 61; 61, 62, 63) and two tiles plus one (117, 121); heights 7, 8, 9 and 17; the smallest
array there is (2 in every extent); 2, 3 and 5 slices, so that a workgroup spans two slices and the last one is partly
empty (e.g. (3, 9, 59): 2 x 2 tiles per slice, 12 tiles, the second workgroup holds the last tile of slice 0 and three of
slice 1).  Iteration counts 1, 2, 3, 4 (= 2 + 2) and 7 (= 3 + 2 + 2) take every launch form, first / middle / last."""
import functools

import numpy as np

from oracle import tomo_oracle as O

LAM, ROF_TAU, LIPSCHITZ = 0.05, 0.005, 8.0

# (shape, iterations)
PD_CASES = [((2, 2, 2), 7), ((3, 9, 59), 7), ((5, 17, 117), 7), ((2, 7, 57), 3), ((3, 8, 58), 4), ((5, 2, 117), 1),
            ((2, 17, 2), 2), ((3, 9, 61), 2), ((2, 8, 63), 1), ((5, 7, 59), 3), ((3, 17, 58), 7)]
ROF_CASES = [((2, 2, 2), 7), ((3, 9, 59), 7), ((5, 17, 117), 7), ((2, 7, 60), 3), ((3, 8, 61), 4), ((5, 2, 121), 1),
             ((2, 17, 2), 2), ((5, 9, 57), 3)]
# the shapes on which the issue states how far the 3D result lies from the slice-wise one (7 iterations)
DISTINCT_SHAPES = [(3, 9, 59), (5, 17, 117), (2, 2, 2)]
FLAG_SHAPES = [((3, 9, 59), 7), ((5, 17, 117), 4)]


def case_id(case):
    shape, iters = case
    return "x".join(map(str, shape)) + f"-it{iters}"


def volume(shape, seed=0, changed=None):
    """a z-ramp from 0 to 1 plus noise of amplitude 0.1 that is seeded PER SLICE (slice k of any stack with the same seed and
    the same (ny, nx) carries the same noise); `changed`: that slice gets other noise"""
    nz, ny, nx = shape
    out = np.empty(shape, np.float32)
    for k in range(nz):
        rng = np.random.default_rng([seed, k, 1 if k == changed else 0])
        out[k] = np.float32(k / max(nz - 1, 1)) + np.float32(0.1) * rng.standard_normal((ny, nx)).astype(np.float32)
    return out


def pd_kwargs(iters, methodTV=0, nonneg=0, half=False):
    return dict(regularisation_parameter=LAM, iterations=iters, methodTV=methodTV, nonneg=nonneg, lipschitz_const=LIPSCHITZ,
                half_precision=half)


def rof_kwargs(iters, half=False):
    return dict(regularisation_parameter=LAM, iterations=iters, time_marching_parameter=ROF_TAU, half_precision=half)


def oracle_slices(method, vol, **kw):
    """the oracle's 2D operator on every slice, stacked"""
    fn = O.pd_tv if method == "PD_TV" else O.rof_tv
    return np.stack([fn(np.ascontiguousarray(vol[k]), **kw).reshape(vol.shape[1:]) for k in range(vol.shape[0])])


def oracle_3d(method, vol, **kw):
    return (O.pd_tv if method == "PD_TV" else O.rof_tv)(vol, **kw)


# ------------------------------------------------------------------------------------------------ tolerance
# The threshold comes from the oracle's own sequence, by the rule of tests/_tolerance_cases.py: d_n compares the WHOLE stack
# after n iterations with the whole stack after n - 6; "stop at the j-th check".
TOL_SHAPE, TOL_ITERATIONS = (3, 40, 40), 66
# name -> (method, keyword arguments, target check j)
TOL_CASES = {
    "pd": ("PD_TV", dict(regularisation_parameter=0.05), 4),
    "pd_half_nonneg_aniso": ("PD_TV", dict(regularisation_parameter=0.05, methodTV=1, nonneg=1, half_precision=True), 4),
    "rof": ("ROF_TV", dict(regularisation_parameter=0.05, time_marching_parameter=0.005), 4),
    "rof_half": ("ROF_TV", dict(regularisation_parameter=0.05, time_marching_parameter=0.005, half_precision=True), 3),
}


def tol_input():
    import _tolerance_cases as T
    return T.phantom(TOL_SHAPE)


def tol_oracle(name, iterations):
    method, kw, _ = TOL_CASES[name]
    return tol_input() if iterations == 0 else oracle_slices(method, tol_input(), iterations=iterations, **kw)


@functools.lru_cache(maxsize=None)
def tol_sequence(name):
    import _tolerance_cases as T
    prev, seq = tol_oracle(name, 0), []
    for n in T.check_points(TOL_ITERATIONS):
        cur = tol_oracle(name, n)
        seq.append(T.rel_d(cur, prev))
        prev = cur
    return tuple(seq)


def tol_plan(name):
    """(tol, iterations the oracle's sequence stops after, the d it stops on, a tol that is never met)"""
    import _tolerance_cases as T
    seq, j = tol_sequence(name), TOL_CASES[name][2]
    return T.threshold(seq, j), T.check_points(TOL_ITERATIONS)[j - 1], seq[j - 1], T.never(seq)
