"""TEST INFRASTRUCTURE beside tests/_cpu_backend.py: the CPU stand-ins for what the tolerance keys add to the
``tomobar_amd.ops`` seam -- ``rel_change``, ``pdtv_tol`` / ``roftv_tol`` -- plus whole-volume ``pdtv`` / ``roftv`` on the
oracle, so that the drivers' early-stopping control flow (tests/test_tolerance.py) runs in a GPU-less process.  The
stand-ins state the stopping rule independently of the library: every iterate a check needs is recomputed by the oracle
from the input, and the sums are float64 numpy."""
import numpy as np
import torch

from oracle import tomo_oracle as O

import _cpu_backend as B
from _tolerance_cases import INNER_INTERVAL, INNER_MIN_SAVED


def rel_change(x, ref, keep=None):
    x64, r64 = B._np(x).astype(np.float64).ravel(), B._np(ref).astype(np.float64).ravel()
    num, den = float(np.sum((x64 - r64) ** 2)), float(np.sum(x64 ** 2))
    if keep is not None:
        keep.copy_(x.view(keep.shape))
    return num, den


def _dims(a):
    return (a.shape[1], a.shape[0], 1, 2) if a.ndim == 2 else (a.shape[2], a.shape[1], a.shape[0], 3)


def _orc_pdtv(data, sigma, tau, lt, theta, iterations, methodTV, nonneg, half):
    a = np.ascontiguousarray(B._np(data))
    if iterations == 0:
        return a.copy()
    out = np.empty_like(a)
    dx, dy, dz, nd = _dims(a)
    rc = O.lib().orc_pdtv(O._fptr(a), O._fptr(out), dx, dy, dz, nd, np.float32(sigma), np.float32(tau), np.float32(lt),
                          np.float32(theta), int(iterations), int(bool(methodTV)), int(bool(nonneg)), int(bool(half)))
    assert rc == 0
    return out


def _orc_roftv(data, lam, tau, iterations, half):
    a = np.ascontiguousarray(B._np(data))
    if iterations == 0:
        return a.copy()
    out = np.empty_like(a)
    dx, dy, dz, nd = _dims(a)
    rc = O.lib().orc_roftv(O._fptr(a), O._fptr(out), dx, dy, dz, nd, np.float32(lam), np.float32(tau), int(iterations),
                           int(bool(half)))
    assert rc == 0
    return out


def _with_rule(iterate, data, out, iterations, tolerance):
    """iterate(n) = the oracle's result after n iterations; the rule: compare iterate n with iterate n - 6 at every multiple
    of 6 that leaves at least 3 of the requested iterations"""
    prev, d = B._np(data), float("nan")
    for n in range(INNER_INTERVAL, iterations + 1, INNER_INTERVAL):
        if iterations - n < INNER_MIN_SAVED:
            break
        cur = iterate(n)
        num, den = rel_change(torch.from_numpy(cur), torch.from_numpy(np.ascontiguousarray(prev)))
        d = 0.0 if num == 0.0 else (float("inf") if den == 0.0 else float(np.sqrt(num / den)))
        if tolerance > 0.0 and d < tolerance:
            return B._put(out, cur), n, d
        prev = cur
    return B._put(out, iterate(iterations)), iterations, d


def pdtv(data, out, sigma, tau, lt, theta, iterations, methodTV, nonneg, half):
    return B._put(out, _orc_pdtv(data, sigma, tau, lt, theta, iterations, methodTV, nonneg, half))


def roftv(data, out, lam, tau, iterations, half):
    return B._put(out, _orc_roftv(data, lam, tau, iterations, half))


def pdtv_tol(data, out, sigma, tau, lt, theta, iterations, methodTV, nonneg, half, tolerance):
    return _with_rule(lambda n: _orc_pdtv(data, sigma, tau, lt, theta, n, methodTV, nonneg, half), data, out, iterations,
                      float(tolerance))


def roftv_tol(data, out, lam, tau, iterations, half, tolerance):
    return _with_rule(lambda n: _orc_roftv(data, lam, tau, n, half), data, out, iterations, float(tolerance))


def install(monkeypatch=None, whole_volume_tv=True):
    """tests/_cpu_backend.install plus the new names.  `whole_volume_tv` False keeps that file's guard that a slab rank
    never calls the whole-volume TV operators."""
    import tomobar_amd.methodsIR_CuPy as IR
    import tomobar_amd.slab as SL
    B.install(monkeypatch)
    ops = IR.ops   # the stand-in module B.install created (shared by every patched module)
    ops.rel_change = rel_change
    if whole_volume_tv:
        ops.pdtv, ops.roftv, ops.pdtv_tol, ops.roftv_tol = pdtv, roftv, pdtv_tol, roftv_tol
    # element-wise glue of the SIRT / CGLS drivers (one float32 rounding per operation, like the kernels)
    ops.axpby = lambda a, x, b, y: B._put(y, np.float32(a) * B._np(x) + np.float32(b) * B._np(y))
    ops.mul = lambda x, y: B._put(y, B._np(x) * B._np(y))

    def recip_safe(x, y):
        with np.errstate(divide="ignore", invalid="ignore"):
            return B._put(y, np.nan_to_num(np.float32(1) / B._np(x), nan=1.0, posinf=1.0, neginf=1.0))
    ops.recip_safe = recip_safe
    ops.get_variant = lambda kernel: 0
    ops.variant = _no_variant
    if monkeypatch is not None:
        monkeypatch.setattr(SL, "_hip_rel_change", rel_change)
    else:
        SL._hip_rel_change = rel_change
    return ops


class _no_variant:
    """`with ops.variant("pdtv", 22)`: the oracle's PD_TV has the reference's roundings already"""

    def __init__(self, kernel, value):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False
