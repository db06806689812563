"""TEST INFRASTRUCTURE: the operator-independent half of the numpy restatements of the explicit time-marching regularisers
(NDF, Diff4th, LLT_ROF), written once.  tests/_ndf_oracle.py, tests/_diff4th_oracle.py and tests/_llt_rof_oracle.py each hold
one formula -- `step(U, f, *scalars, ...)` -- with its parameter sets, and build a `Marcher` from them: the record the
shared suites (tests/_march_oracle_suite.py, tests/_march_gloo_suite.py, tests/_march_gpu_suite.py) and the edge-shape tests
run every operator through.  numpy only."""
import functools

import numpy as np

from _tgv_oracle import phantom, rel_d

TOL_INTERVAL, TOL_MIN_SAVED = 6, 3


def _sh(U, ax, s):
    """U[i + s e_ax], the index clamped into the array"""
    n = U.shape[ax]
    return np.take(U, np.clip(np.arange(n) + s, 0, n - 1), axis=ax)


def _as_numpy(t):
    return t.numpy() if hasattr(t, "numpy") else np.asarray(t)


def slab_bounds(nz, world):
    base, extra = divmod(nz, world)
    bounds, z = [], 0
    for r in range(world):
        bounds.append((z, z + base + (1 if r < extra else 0)))
        z = bounds[-1][1]
    return bounds


def rel_change_sums(x, ref, keep=None):
    """CPU stand-in for tomo_rel_change at the slab driver's seam (tomobar_amd.slab._hip_rel_change): (sum (x - ref)^2,
    sum x^2) in float64 from the float32 values; with `keep`, keep[...] = x afterwards"""
    x64, r64 = _as_numpy(x).astype(np.float64).ravel(), _as_numpy(ref).astype(np.float64).ravel()
    num, den = float(np.sum((x64 - r64) ** 2)), float(np.sum(x64 ** 2))
    if keep is not None:
        keep.copy_(x.view(keep.shape))
    return num, den


def slab_step(step, inp, u_in, u_out, dx, dy, nzl, lo, hi, scalars, zr, ghost, **extra):
    """One iteration of `step` on ghosted slab arrays [lo + nzl + hi][dy][dx] (host torch tensors or numpy arrays): `ghost`
    planes exist exactly where a z-neighbour exists, so the plain whole-array step on the ghosted array treats z as a
    boundary only at the global faces and is right on every LOCAL plane; only the local planes [z0, z1) of `u_out` are
    written."""
    z0, z1 = zr if zr is not None else (0, nzl)
    f, U, out = _as_numpy(inp), _as_numpy(u_in), _as_numpy(u_out)
    assert U.shape == (lo + nzl + hi, dy, dx) and U.dtype == np.float32
    a, b = max(lo + z0 - ghost, 0), min(lo + z1 + ghost, U.shape[0])    # the output planes and the ghost depth either side
    new = step(U[a:b], f[a:b], *(np.float32(v) for v in scalars), **extra)
    out[lo + z0:lo + z1] = new[lo + z0 - a:lo + z1 - a]


class Marcher:
    """One operator's record.  `step(U, f, *scalars, <the other keys of a parameter set>, stats=None)` is one iteration;
    `keys` names the scalars of a parameter set in step's order, and what else a set holds (NDF's penalty) follows them in
    `extra`.  Every operator-independent entry point of a restatement is a method.

    narrow: the scalars are rounded to float32 before they are converted to `dtype` (so a float64 run uses the float32
        values) -- LLT_ROF; otherwise they are converted to `dtype` as given.
    stats_each: `stats` receives step's figures of every iteration n (1-based) under (key, n); otherwise step writes the
        figures of the LAST iteration straight into it -- NDF.
    step_slab: an operator's own single-iteration slab function where the one below does not fit."""

    def __init__(self, name, step, PARAMS, keys, GHOST, TOL_CASE, TOL_CASE_SLAB, narrow=False, stats_each=True,
                 step_slab=None):
        self.name, self.step, self.PARAMS, self.keys, self.GHOST = name, step, PARAMS, tuple(keys), GHOST
        self.TOL_CASE, self.TOL_CASE_SLAB = TOL_CASE, TOL_CASE_SLAB
        self.extra = tuple(k for k in next(iter(PARAMS.values())) if k not in self.keys)
        self.narrow, self.stats_each = narrow, stats_each
        if step_slab is not None:
            self.step_slab = step_slab

    def positional(self, params):
        """a parameter set in the order step, step_slab and the ops function take it: the scalars, then the rest"""
        return tuple(params[k] for k in self.keys + self.extra)

    def call_args(self, params, iterations):
        """... and in the order the *_cupy function and the slab driver take it: the two parameters, the iteration count,
        the time step, then the rest"""
        a, b, tau = (params[k] for k in self.keys)
        return (a, b, iterations, tau) + tuple(params[k] for k in self.extra)

    # -------------------------------------------------------------------------------------------- the whole array
    def iterates(self, f, iterations=1, dtype=np.float32, stats=None, **params):
        """yields U after every iteration (a fresh array each time); `stats` (a dict): see the class"""
        t = dtype
        f = np.asarray(f).astype(t)
        assert f.ndim in (2, 3)
        scalars = [t(np.float32(params[k])) if self.narrow else t(params[k]) for k in self.keys]
        extra = {k: params[k] for k in self.extra}
        U = f
        for n in range(1, iterations + 1):
            if stats is None or not self.stats_each:
                s = stats if n == iterations else None
            else:
                s = {}
            U = self.step(U, f, *scalars, stats=s, **extra)
            if s is not None and self.stats_each:
                stats.update({(k, n): v for k, v in s.items()})
            yield U

    def run(self, f, iterations=1, dtype=np.float32, stats=None, **params):
        """U after `iterations` iterations (a copy of the input, as `dtype`, for 0)"""
        out = np.asarray(f).astype(dtype)
        for out in self.iterates(f, iterations, dtype, stats, **params):
            pass
        return out

    def many(self, f, params, counts, dtype=np.float32):
        """{n: U after n iterations} for every n of `counts`, from ONE run"""
        counts = sorted(set(counts))
        out = {}
        for n, U in enumerate(self.iterates(f, iterations=counts[-1], dtype=dtype, **params), 1):
            if n in counts:
                out[n] = U
        return out

    @functools.lru_cache(maxsize=None)
    def cached(self, shape, pname, counts, dtype_name="float32"):
        """`many` of the phantom of `shape` under the parameter set `pname`: computed once per session, never modified"""
        res = self.many(phantom(shape), self.PARAMS[pname], counts, np.dtype(dtype_name).type)
        for v in res.values():
            v.setflags(write=False)
        return res

    # -------------------------------------------------------------------------------------------- z-slabs
    def step_slab(self, inp, u_in, u_out, dx, dy, nzl, lo, hi, *args, zr=None, ghost=None):
        """the step_fn of the operator's tomobar_amd.slab driver (see slab_step): `args` are the parameters in `positional`
        order, then optionally the plane range `zr`.  (`ghost` below GHOST exists for the test that shows GHOST planes are
        needed.)"""
        ghost = self.GHOST if ghost is None else ghost
        n = len(self.keys)
        if len(args) > n + len(self.extra):
            zr = args[-1]
        assert lo in (0, ghost) and hi in (0, ghost)
        slab_step(self.step, inp, u_in, u_out, dx, dy, nzl, lo, hi, args[:n], zr, ghost,
                  **dict(zip(self.extra, args[n:])))

    def by_slabs(self, f, params, iterations, world, bounds=None, ghost=None):
        """the whole volume run as `world` ghosted slabs (`bounds`: their plane ranges, an even split by default) exchanged by
        hand after every iteration, stitched"""
        ghost = self.GHOST if ghost is None else ghost
        f = np.asarray(f, np.float32)
        bounds = bounds or slab_bounds(f.shape[0], world)
        U = f.copy()
        for _ in range(iterations):
            new = np.empty_like(U)
            for r, (z0, z1) in enumerate(bounds):
                lo, hi = ghost * int(r > 0), ghost * int(r < len(bounds) - 1)
                g_in = np.ascontiguousarray(U[z0 - lo:z1 + hi])
                g_f = np.ascontiguousarray(f[z0 - lo:z1 + hi])
                g_out = np.full_like(g_in, np.nan)
                self.step_slab(g_f, g_in, g_out, f.shape[2], f.shape[1], z1 - z0, lo, hi, *self.positional(params), ghost=ghost)
                new[z0:z1] = g_out[lo:lo + z1 - z0]
            U = new
        return U

    # -------------------------------------------------------------------------------------------- the tolerance rule
    @functools.lru_cache(maxsize=None)
    def tolerance_plan(self, slab=False):
        """(tol, n the oracle's sequence stops after, the d it stops on, the whole sequence) of TOL_CASE (TOL_CASE_SLAB with
        `slab`): d_n compares iterate n with iterate n - 6 (iterate 0 = the input) after every 6th iteration that leaves at
        least 3; tol is the geometric mean of the (j-1)-th and j-th values, as tests/_tgv_oracle.py chooses its threshold"""
        c = self.TOL_CASE_SLAB if slab else self.TOL_CASE
        points = [n for n in range(TOL_INTERVAL, c["iterations"] + 1, TOL_INTERVAL) if c["iterations"] - n >= TOL_MIN_SAVED]
        its = self.cached(c["shape"], c["pname"], tuple(points))
        prev, seq = phantom(c["shape"]), []
        for n in points:
            seq.append(rel_d(its[n], prev))
            prev = its[n]
        j = c["j"]
        tol = float(np.sqrt(seq[j - 2] * seq[j - 1]))
        assert all(abs(v - tol) >= 0.01 * tol for v in seq), ("a value of the sequence is too close to the threshold", tol, seq)
        assert next(i for i, v in enumerate(seq, 1) if v < tol) == j, ("the target is not the first value below the threshold", seq)
        return tol, points[j - 1], seq[j - 1], tuple(seq)
