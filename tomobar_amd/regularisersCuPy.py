"""TV proximal operators on MI355X: same functions and argument meaning as the reference's
``tomobar/regularisersCuPy.py`` (``prox_regul`` :6-38, ``ROF_TV_cupy`` :41-167, ``PD_TV_cupy`` :170-296),
arrays are float32 ``torch.Tensor`` on the GPU instead of ``cupy.ndarray``.  ``TGV_cupy`` (second-order total generalised
variation), ``NDF_cupy`` (nonlinear diffusion with the Huber, Perona-Malik and Tukey penalties), ``Diff4th_cupy``
(anisotropic fourth-order diffusion) and ``LLT_ROF_cupy`` (ROF plus the fourth-order Lysaker-Lundervold-Tai term) have no
counterpart in this reference version: formula-level parity, unpinned (docs/kernels/tgv.md, docs/kernels/ndf.md,
docs/kernels/diff4th.md, docs/kernels/llt_rof.md).  ``WAVELETS_cupy`` (db5 wavelet shrinkage, docs/kernels/wavelets.md) is the
step behind the ``_WAVELETS`` suffix of a method: the reference's tutorials use it, its tree no longer implements it.
``PatchSelect_cupy`` and ``NLTV_cupy`` (non-local TV over neighbour tables, docs/kernels/nltv.md) are the two halves behind
the method "NLTV" of the reference's legacy demo, likewise implemented nowhere in its tree.

The iteration loops run inside ``libtomo_mi355x.so`` (``tomo_pdtv`` / ``tomo_roftv``): one fused HIP kernel per
iteration, launched back to back on the caller's stream, scratch taken from the library's arena
(the reference allocates nine arrays and looks the CUDA module up on every call, :84,220-232).
"""

from __future__ import annotations

import threading
from typing import Optional, Tuple

import numpy as np
import torch

from . import ops
from .convergence import check_tolerance
from .supp.regularisers import (NLTV_CUPY, SLICEWISE_KINDS, WAVELETS_REFUSED, has_wavelets, is_nltv, kind_of, nltv_check,
                                nltv_iterations, nltv_tables, slicewise_of, wavelet_threshold)

_last = threading.local()


def last_prox() -> Optional[Tuple[int, float]]:
    """(iterations_done, rel_change) of the calling thread's most recent ``prox_regul`` or ``*_cupy`` call (the functions
    supp/regularisers.py names): how many inner iterations ran and the last relative change the stopping rule evaluated
    (NaN if it evaluated none, e.g. with the tolerance off); None before the first call."""
    return getattr(_last, "value", None)


def _record(done: int, rel_change: float) -> None:
    _last.value = (int(done), float(rel_change))


def prox_regul(self, X: torch.Tensor, _regularisation_: dict, out=None) -> torch.Tensor:
    """Dispatch on the ``method`` substring exactly like regularisersCuPy.py:16-38.

    One key beyond the reference's: ``_regularisation_["exact_roundings"] = True`` runs PD_TV with the rounding sequence of
    the reference's kernels for float32 duals too (``tomo_set_variant("pdtv", 22)``: bit-identical to the reference
    arithmetic, 5-16 % slower per launch) for this call; absent / False = the default (within 1e-5).

    ``_regularisation_["tolerance"]`` > 0 stops the inner iterations early (tomobar_amd/convergence.py; the reference
    accepts the key and ignores it); ``last_prox()`` tells how far the call got.

    A method that names a kind and contains ``WAVELETS`` (the reference's tutorials: "PD_TV_WAVELETS") returns
    ``(prox_kind(X) + W_t(X)) * 0.5`` with ``W_t`` the wavelet shrinkage of ``WAVELETS_cupy`` and t = ``regul_param2``: the
    kind runs exactly as without the suffix (all keys keep their meaning for it, ``last_prox()`` reports its iterations),
    then the shrinkage of the same X is averaged into its result.  In z-slab mode that step needs no communication (it is
    per slice).

    ``_regularisation_["slicewise"] = True`` (ROF_TV and PD_TV; absent / False = the default, 3D TV coupled along z) returns
    ``stack([prox2d(X[k]) for k in range(nz)])`` for a 3D volume whose extents all exceed 1: the 2D total variation of every
    (y, x) slice on its own, all slices in one set of launches (docs/kernels/slicewise.md), every other key keeping its
    meaning.  The result does not depend on how z is cut into chunks or slabs: a slab rank runs its own slices through the
    same whole-volume function and never touches the communicator (no ghost planes, no reduction), which is why a
    tolerance > 0 is refused there -- the ranks would stop at different iterations.  A 2D input or a singleton axis already
    runs the 2D kernels: the key changes nothing there.  The other kinds refuse the key.

    A method that contains ``NLTV`` and names no kind (the reference's legacy demo: "NLTV") runs ``NLTV_cupy`` over the tables
    under ``NLTV_H_i``, ``NLTV_H_j`` and ``NLTV_Weights`` (built beforehand with ``PatchSelect_cupy``) with lambda =
    ``regul_param`` and ``IterNumb`` (else ``iterations``) iterations (docs/kernels/nltv.md).  It is per slice by definition:
    a slab rank runs its own slices over its own tables without communication, and refuses a tolerance > 0 as above."""
    if _regularisation_.get("exact_roundings") and "PD_TV" in _regularisation_["method"] and ops.get_variant("pdtv") == 0:
        with ops.variant("pdtv", 22):
            return _prox_regul(self, X, _regularisation_, out)
    return _prox_regul(self, X, _regularisation_, out)


def _prox_regul(self, X: torch.Tensor, _regularisation_: dict, out=None) -> torch.Tensor:
    method = _regularisation_["method"]
    kind = kind_of(method)
    slab = getattr(self, "slab", None)
    check_prox_available(self, X.shape, _regularisation_)
    tol = check_tolerance(_regularisation_.get("tolerance"), "_regularisation_['tolerance']")
    if is_nltv(method):
        # per slice by definition: a slab rank runs its own slices over its own tables, no communication
        return globals()[NLTV_CUPY](X, *nltv_tables(_regularisation_), _regularisation_["regul_param"], nltv_iterations(_regularisation_),
                                    self.Atools.device_index, out=out, tolerance=tol)
    if kind is None:
        raise ValueError(f"unknown regularisation method {method!r}: ROF_TV, PD_TV and TGV are supported, as are NDF, Diff4th "
                         "and LLT_ROF")
    args = kind.args(_regularisation_, self)
    half = (_regularisation_.get("half_precision", False),) if kind.half else ()
    true3d = X.dim() == 3 and min(X.shape) > 1
    if slicewise_of(_regularisation_) and true3d:
        # every slice on its own: the whole-volume function on this rank's slices, with or without a slab
        res = globals()[kind.cupy](X, *args, self.Atools.device_index, *half, out=out, tolerance=tol, slicewise=True)
    elif slab is not None and true3d:
        # the volume is one z-slab of a larger one: 3D TV with ghost planes exchanged between z-neighbours
        from . import slab as slab_drivers
        info = {"iterations_done": _regularisation_["iterations"], "rel_change": float("nan")}
        res = getattr(slab_drivers, kind.slab)(ops.contiguous(X), slab, *args, *half, out=out, tolerance=tol, info=info)
        _record(info["iterations_done"], info["rel_change"])
    else:
        res = globals()[kind.cupy](X, *args, self.Atools.device_index, *half, out=out, tolerance=tol)
    if has_wavelets(method):
        # the average of the two proximal maps of X: the last wavelet launch reads the kind's result where it writes
        dst = ops.to_device(res, self.Atools.device_index) if ops.is_cupy(res) else res
        WAVELETS_cupy(X, wavelet_threshold(_regularisation_), self.Atools.device_index, out=dst, mix=dst)
    return res


def check_prox_available(self, vol_shape, _regularisation_: dict) -> None:
    """What TGV cannot do yet, as a ValueError before any work is done: z-slab mode on a real 3D volume (the halo protocol
    for its 13 further fields does not exist) and binary16 storage of its fields.  NDF, Diff4th and LLT_ROF have no binary16
    storage either (they do run in z-slab mode).  The ``WAVELETS`` suffix does not combine with LLT_ROF (``regul_param2`` is
    already that kind's LLT weight).  ``slicewise=True`` exists for ROF_TV and PD_TV only, and on a slab rank with a real 3D
    volume it does not combine with a tolerance > 0 (no communication: the ranks would stop at different iterations and the
    result would depend on the split).  NLTV (docs/kernels/nltv.md) combines with no kind, not with ``WAVELETS`` and not with
    ``half_precision=True``; a slab rank runs it on its own slices, so there it refuses a tolerance > 0 for the same reason
    as ``slicewise`` (the key itself is not consulted: NLTV is per slice by definition).  The other methods pass."""
    nltv_check(_regularisation_)
    if is_nltv(_regularisation_.get("method")):
        if getattr(self, "slab", None) is not None and _true_3d(vol_shape) \
                and check_tolerance(_regularisation_.get("tolerance"), "_regularisation_['tolerance']") > 0.0:
            raise ValueError("NLTV does not take a tolerance in z-slab mode: every rank would stop on its own slices and "
                             "the result would depend on the split")
        return
    kind = kind_of(_regularisation_.get("method"))
    if kind is None:
        return
    slicewise = slicewise_of(_regularisation_)
    if slicewise and kind.name not in SLICEWISE_KINDS:
        raise ValueError(f"{kind.name} does not support slicewise=True")
    if slicewise and getattr(self, "slab", None) is not None and _true_3d(vol_shape) \
            and check_tolerance(_regularisation_.get("tolerance"), "_regularisation_['tolerance']") > 0.0:
        raise ValueError(f"{kind.name} with slicewise=True does not take a tolerance in z-slab mode: every rank would stop "
                         "on its own slices and the result would depend on the split")
    if kind.name in WAVELETS_REFUSED and has_wavelets(_regularisation_.get("method")):
        raise ValueError(f"{kind.name} does not combine with WAVELETS: regul_param2 is already its second weight")
    if not kind.half and _regularisation_.get("half_precision", False):
        raise ValueError(f"{kind.name} does not support half_precision=True")
    if kind.slab is None and getattr(self, "slab", None) is not None:
        if _true_3d(vol_shape):
            raise ValueError(f"{kind.name} is not available in z-slab mode")


def _true_3d(vol_shape) -> bool:
    shape = tuple(int(v) for v in vol_shape)
    return len(shape) == 3 and min(shape) > 1


def reserve_prox_scratch(self, vol_shape, _regularisation_: dict) -> None:
    """Set-up step of the iterative drivers: allocate -- and place, tomo_reserve_scratch -- the library's TV scratch arena
    for volumes of ``vol_shape`` before the loop starts, so that the placement search (0.1-4 s, transient footprint of up
    to `tries` x arena) is not part of the first proximal step.  No reference counterpart (CuPy's pool allocates the nine
    arrays inside every call, regularisersCuPy.py:220-232).  Nothing to do without a TV method, and in z-slab mode the
    slab drivers take their own placed block (slab.py)."""
    check_prox_available(self, vol_shape, _regularisation_)
    if is_nltv(_regularisation_.get("method")):   # one work array, on a slab rank as well (its prox is the whole-volume call)
        ops.reserve_nltv_scratch(tuple(int(v) for v in vol_shape), f"cuda:{self.Atools.device_index}")
        return
    kind = kind_of(_regularisation_.get("method"))
    if kind is None or getattr(self, "slab", None) is not None:
        return
    shape = tuple(int(v) for v in vol_shape)
    if slicewise_of(_regularisation_) and _true_3d(shape):   # the work arrays of the slice-wise form
        ops.reserve_tv_slices_scratch(shape, f"cuda:{self.Atools.device_index}", kind.name, bool(_regularisation_.get("half_precision", False)))
        if has_wavelets(_regularisation_.get("method")):
            ops.reserve_wavelet_scratch(shape, f"cuda:{self.Atools.device_index}")
        return
    if len(shape) == 3 and 1 in shape:       # a singleton axis runs the 2D kernels (_check_if_input_2d_or_3d)
        i = shape.index(1)
        shape = shape[:i] + shape[i + 1:]
    ops.reserve_tv_scratch(shape, f"cuda:{self.Atools.device_index}", kind.name, bool(_regularisation_.get("half_precision", False)))
    if has_wavelets(_regularisation_.get("method")):   # the coefficient pyramid shares that arena: it grows to the larger need
        ops.reserve_wavelet_scratch(shape, f"cuda:{self.Atools.device_index}")


def _prepare(data, gpu_id: int):
    if gpu_id < 0:
        raise ValueError("The gpu_device must be a positive integer or zero")
    data = ops.to_device(data, gpu_id)
    if data.dtype != torch.float32:
        raise ValueError("The input data should be float32 data type")
    data, is2d, axis = _check_if_input_2d_or_3d(data)
    return ops.contiguous(data), is2d, axis


def _finish(result, is2d, axis, orig_shape, out, given=None):
    result = result.unsqueeze(axis) if is2d else result
    return ops.like(result, given) if out is None else out.view(orig_shape)


def _marched(run, data, gpu_id: int, out, tolerance):
    """The shared body of TGV_cupy / NDF_cupy / Diff4th_cupy / LLT_ROF_cupy: ``run(d, res, tolerance)`` is the ops call, which
    returns (res, iterations_done, rel_change)."""
    tolerance = check_tolerance(tolerance, "tolerance")
    orig_shape = tuple(data.shape)
    d, is2d, axis = _prepare(data, gpu_id)
    res = torch.empty_like(d) if out is None else out.view(d.shape)
    _, done, change = run(d, res, tolerance)
    _record(done, change)
    return _finish(res, is2d, axis, orig_shape, out, data)


def ROF_TV_cupy(data, regularisation_parameter: float = 1e-05, iterations: int = 3000,
                time_marching_parameter: float = 0.001, gpu_id: int = 0, half_precision: bool = False,
                out=None, tolerance: float = 0.0, slicewise: bool = False) -> torch.Tensor:
    """Rudin-Osher-Fatemi TV by explicit time marching (reference: regularisersCuPy.py:41-167).

    ``half_precision`` reproduces the reference's binary16 storage of the D fields (they are rounded through
    half in registers; the fused kernel never writes them to memory).  ``tolerance`` > 0 (no reference counterpart) stops
    the iterations early by the rule of tomobar_amd/convergence.py; ``last_prox()`` tells after which iteration.
    ``slicewise=True`` (no reference counterpart) treats a 3D array as a stack of independent 2D images along axis 0: slice k
    of the result is what this function returns for ``data[k]``, all slices in one launch per iteration and with one
    stopping decision over the whole array; a 2D array or a singleton axis runs as without it."""
    tolerance = check_tolerance(tolerance, "tolerance")
    orig_shape = tuple(data.shape)
    d, is2d, axis = _prepare(data, gpu_id)
    res = torch.empty_like(d) if out is None else out.view(d.shape)
    if slicewise and not is2d:
        _, done, change = ops.roftv_slices(d, res, np.float32(regularisation_parameter), np.float32(time_marching_parameter),
                                           iterations, half_precision, tolerance)
        _record(done, change)
    elif tolerance > 0.0:
        _, done, change = ops.roftv_tol(d, res, np.float32(regularisation_parameter), np.float32(time_marching_parameter),
                                        iterations, half_precision, tolerance)
        _record(done, change)
    else:
        ops.roftv(d, res, np.float32(regularisation_parameter), np.float32(time_marching_parameter), iterations,
                  half_precision)
        _record(iterations, float("nan"))
    return _finish(res, is2d, axis, orig_shape, out, data)


def PD_TV_cupy(data, regularisation_parameter: float = 1e-05, iterations: int = 1000, methodTV: int = 0,
               nonneg: int = 0, lipschitz_const: float = 8.0, gpu_id: int = 0, half_precision: bool = False,
               out=None, tolerance: float = 0.0, slicewise: bool = False) -> torch.Tensor:
    """Chambolle-Pock primal-dual TV (reference: regularisersCuPy.py:170-296).  ``tolerance`` > 0 (no reference
    counterpart) stops the iterations early by the rule of tomobar_amd/convergence.py; ``last_prox()`` tells after which.
    ``slicewise=True`` (no reference counterpart) treats a 3D array as a stack of independent 2D images along axis 0: slice k
    of the result is what this function returns for ``data[k]``, all slices in one set of launches and with one stopping
    decision over the whole array; a 2D array or a singleton axis runs as without it."""
    tolerance = check_tolerance(tolerance, "tolerance")
    orig_shape = tuple(data.shape)
    d, is2d, axis = _prepare(data, gpu_id)
    # float32 scalar set-up of regularisersCuPy.py:215-218 (NumPy-2 weak-scalar promotion => float32 arithmetic)
    tau = np.float32(regularisation_parameter * 0.1)
    sigma = np.float32(1.0 / (lipschitz_const * tau))
    theta = np.float32(1.0)
    lt = np.float32(tau / regularisation_parameter)
    res = torch.empty_like(d) if out is None else out.view(d.shape)
    if slicewise and not is2d:
        _, done, change = ops.pdtv_slices(d, res, sigma, tau, lt, theta, iterations, methodTV, nonneg, half_precision, tolerance)
        _record(done, change)
    elif tolerance > 0.0:
        _, done, change = ops.pdtv_tol(d, res, sigma, tau, lt, theta, iterations, methodTV, nonneg, half_precision, tolerance)
        _record(done, change)
    else:
        ops.pdtv(d, res, sigma, tau, lt, theta, iterations, methodTV, nonneg, half_precision)
        _record(iterations, float("nan"))
    return _finish(res, is2d, axis, orig_shape, out, data)


def TGV_cupy(data, regularisation_parameter: float = 1e-05, iterations: int = 1000, alpha1: float = 1.0,
             alpha0: float = 2.0, lipschitz_const: float = 12.0, gpu_id: int = 0, out=None,
             tolerance: float = 0.0) -> torch.Tensor:
    """Second-order total generalised variation (Bredies-Kunisch-Pock) by Chambolle-Pock iterations:
    ``argmin_u 1/2 |u - f|^2 + lambda min_v (alpha1 |grad u - v|_1 + alpha0 |E v|_1)``.

    There is no reference implementation of it in this reference version (it took TGV from the regularisation toolkit it no
    longer depends on): the algorithm is the one stated in docs/kernels/tgv.md -- formula-level parity, unpinned; the
    float32 result equals the numpy restatement tests/_tgv_oracle.py bit for bit.  ``tolerance`` > 0 stops the iterations
    early by the rule of tomobar_amd/convergence.py; ``last_prox()`` tells after which iteration.  There is no
    non-negativity switch (the drivers clamp before the prox) and no binary16 storage."""
    def run(d, res, tolerance):
        # float32 scalars, formed the way PD_TV_cupy forms its own
        lam = np.float32(regularisation_parameter)
        tau = np.float32(np.float32(1.0) / np.sqrt(np.float32(lipschitz_const)))
        return ops.tgv(d, res, lam, np.float32(alpha1), np.float32(alpha0), tau, tau, iterations, tolerance)
    return _marched(run, data, gpu_id, out, tolerance)


def NDF_cupy(data, regularisation_parameter: float = 1e-05, edge_parameter: float = 0.01, iterations: int = 1000,
             time_marching_parameter: float = 0.001, penalty_type: str = "Huber", gpu_id: int = 0, out=None,
             tolerance: float = 0.0) -> torch.Tensor:
    """Nonlinear diffusion by explicit time marching: ``U' = U + tau (lambda S - (U - f))`` with ``S`` the sum over the axes
    of the fluxes ``g`` of the forward and backward differences, zero flux through the faces of the volume.
    ``penalty_type`` chooses ``g`` against the noise threshold ``edge_parameter``: "Huber" (behaves like TV), "PM"
    (Perona-Malik: sharpens edges) or "Tukey" (biweight: differences above the threshold are left untouched).

    There is no reference implementation of it in this reference version (its dicts_check names NDF beside
    ``time_marching_step``, nothing implements it): the algorithm is the one stated in docs/kernels/ndf.md -- formula-level
    parity, unpinned; the float32 result equals the numpy restatement tests/_ndf_oracle.py bit for bit.  ``tolerance`` > 0
    stops the iterations early by the rule of tomobar_amd/convergence.py; ``last_prox()`` tells after which iteration.
    There is no non-negativity switch (the drivers clamp before the prox) and no binary16 storage."""
    from ._lib import ndf_penalty_id
    ndf_penalty_id(penalty_type)   # an unknown penalty: ValueError before anything is moved to the device
    return _marched(lambda d, res, tol: ops.ndf(d, res, np.float32(regularisation_parameter), np.float32(edge_parameter),
                                                np.float32(time_marching_parameter), penalty_type, iterations, tol),
                    data, gpu_id, out, tolerance)


def Diff4th_cupy(data, regularisation_parameter: float = 1e-05, edge_parameter: float = 0.01, iterations: int = 1000,
                 time_marching_parameter: float = 0.001, gpu_id: int = 0, out=None, tolerance: float = 0.0) -> torch.Tensor:
    """Anisotropic fourth-order diffusion (Hajiaboli) by explicit time marching: ``U' = U - tau (lambda Lap(W) + (U - f))``
    with ``W`` the second derivatives of ``U`` along and across its gradient, weighted by ``cw^2`` and ``cw``,
    ``cw = 1 / (1 + |grad U|^2 / sigma^2)``: smooth regions are driven towards planes instead of TV's staircase, edges
    above the threshold ``edge_parameter`` (sigma) are kept.  The scheme is explicit: keep
    ``time_marching_parameter * (1 + 16 * nd**2 * regularisation_parameter)`` at or below 1 (not checked).

    There is no reference implementation of it in this reference version (its dicts_check names Diff4th beside
    ``time_marching_step``, nothing implements it): the algorithm is the one stated in docs/kernels/diff4th.md --
    formula-level parity, unpinned; the float32 result equals the numpy restatement tests/_diff4th_oracle.py bit for bit.
    ``tolerance`` > 0 stops the iterations early by the rule of tomobar_amd/convergence.py; ``last_prox()`` tells after
    which iteration.  There is no non-negativity switch (the drivers clamp before the prox) and no binary16 storage."""
    return _marched(lambda d, res, tol: ops.diff4th(d, res, np.float32(regularisation_parameter), np.float32(edge_parameter),
                                                    np.float32(time_marching_parameter), iterations, tol),
                    data, gpu_id, out, tolerance)


def LLT_ROF_cupy(data, regularisation_parameterROF: float = 1e-05, regularisation_parameterLLT: float = 1e-05,
                 iterations: int = 1000, time_marching_parameter: float = 0.001, gpu_device: int = 0, out=None,
                 tolerance: float = 0.0) -> torch.Tensor:
    """ROF total variation plus the fourth-order Lysaker-Lundervold-Tai (LLT) term by explicit time marching:
    ``U' = U - tau ((lambda_LLT B - lambda_ROF V) + (U - f))`` with ``V`` the divergence of the ROF flux
    ``grad U / sqrt(|grad U|^2 + eps)`` and ``B`` the second differences of the per-axis LLT flux ``h / (|h| + eps)`` of the
    second differences ``h`` of ``U``.  The ROF term keeps edges, the LLT term removes the staircase on ramps;
    ``regularisation_parameterROF`` and ``regularisation_parameterLLT`` weigh the one against the other.  Both fluxes are
    bounded by 1, so no bound on ``time_marching_parameter`` is checked.

    There is no reference implementation of it in this reference version (its dicts_check names LLT_ROF beside
    ``time_marching_step``, nothing implements it): the algorithm is the one stated in docs/kernels/llt_rof.md --
    formula-level parity, unpinned; the float32 result equals the numpy restatement tests/_llt_rof_oracle.py bit for bit.
    ``tolerance`` > 0 stops the iterations early by the rule of tomobar_amd/convergence.py; ``last_prox()`` tells after
    which iteration.  There is no non-negativity switch (the drivers clamp before the prox) and no binary16 storage."""
    return _marched(lambda d, res, tol: ops.llt_rof(d, res, np.float32(regularisation_parameterROF),
                                                    np.float32(regularisation_parameterLLT),
                                                    np.float32(time_marching_parameter), iterations, tol),
                    data, gpu_device, out, tolerance)


def WAVELETS_cupy(data, regularisation_parameter: float = 0.001, gpu_device: int = 0, out=None, mix=None) -> torch.Tensor:
    """Wavelet shrinkage ``W_t``: three levels of the 2D orthonormal Daubechies-5 transform (periodization mode) of every
    (y, x) slice -- a 3D array is a stack of independent slices over z --, soft threshold ``regularisation_parameter`` on
    every detail coefficient, inverse transform.  A threshold of 0 gives the input back up to rounding; a negative one is a
    ValueError.  With ``mix`` (an array like ``out``; it may be ``out``) the result is ``(mix + W_t(data)) * 0.5``, formed as
    the last launch writes: how ``prox_regul`` averages the shrinkage with the prox of a ``<kind>_WAVELETS`` method.

    The reference's tutorials name the step ("PD_TV_WAVELETS", ``regul_param2``); its implementation lived in the removed
    RecToolsIR class on the CUDA-only pypwt package: the algorithm is the one stated in docs/kernels/wavelets.md --
    formula-level parity, unpinned; the float32 result equals the numpy restatement tests/_wavelet_oracle.py bit for bit.
    Not iterative: ``last_prox()`` is left as it was."""
    if not float(regularisation_parameter) >= 0.0:
        raise ValueError("the wavelet threshold must not be negative")
    orig_shape = tuple(data.shape)
    d, is2d, axis = _prepare(data, gpu_device)
    res = torch.empty_like(d) if out is None else out.view(d.shape)
    ops.wavelet_shrink(d, np.float32(regularisation_parameter), out=res, mix=None if mix is None else mix.view(d.shape))
    return _finish(res, is2d, axis, orig_shape, out, data)


def PatchSelect_cupy(data, searchwindow: int = 7, patchwindow: int = 2, neighbours: int = 15, edge_parameter: float = 0.9,
                     gpu_id: int = 0):
    """The neighbour tables of ``NLTV_cupy``: for every pixel the ``neighbours`` (1..32) pixels of its search window
    ``[-searchwindow, searchwindow]^2`` (1..15) whose ``(2 patchwindow + 1)^2`` patch (1..4) is most similar to its own, with
    the weights ``exp(-d / edge_parameter^2)`` of their Gaussian-weighted patch distances ``d``.  A 3D array is a stack of
    independent (y, x) slices along axis 0 (singleton axes included): search and patches never leave a slice.  Returns
    ``(H_i, H_j, Weights)`` of shape ``(neighbours, *data.shape)`` on the device: the x and the y index of each neighbour
    (uint16) and its weight (float32), most similar first; a pixel with fewer candidates than ``neighbours`` fills the rest
    with its own index and the weight 0.  The tables take ``8 * neighbours`` bytes per voxel.

    The defaults are those of the reference's legacy demo (Demos/methods_IR_legacy/DemoFISTA_NLTV_2D.py), whose
    ``PatchSelect`` lived in the regularisation toolkit the reference no longer depends on: the algorithm is the one stated
    in docs/kernels/nltv.md -- formula-level parity, unpinned; indices and weights equal the numpy restatement
    tests/_nltv_oracle.py bit for bit."""
    d = _prepare_stack(data, gpu_id)
    return tuple(ops.like(t, data) for t in ops.patch_select(d, searchwindow, patchwindow, neighbours, np.float32(edge_parameter)))


def NLTV_cupy(data, H_i, H_j, Weights, regularisation_parameter: float = 1e-05, iterations: int = 3, gpu_id: int = 0,
              out=None, tolerance: float = 0.0) -> torch.Tensor:
    """Non-local total variation over the tables of ``PatchSelect_cupy``: ``iterations`` Jacobi iterations, from ``u = data``,
    of ``u' = (data / lambda + c sum_k W_k u_k) / (1 / lambda + c sum_k W_k)`` with ``u_k`` the k-th neighbour of the pixel
    and ``c = 2 / sqrt(sum_k W_k (u_k - u)^2 + 1e-12)``.  A 3D array is a stack of independent (y, x) slices along axis 0
    (singleton axes included).  The tables hold ``Weights.shape[0]`` neighbours per voxel; any shape with that many
    elements per neighbour is accepted (of the squeezed or the unsqueezed array).  Tables that are not on the device are
    copied there on every call: keep them there.  An index beyond the slice is clamped into it.  Like every ``*_cupy``
    function here (and the reference's), a 2D input comes back with a leading singleton axis unless ``out`` is given.

    There is no reference implementation of it in this reference version (its legacy demo still passes the tables; the
    function lived in the regularisation toolkit it no longer depends on): the algorithm is the one stated in
    docs/kernels/nltv.md -- formula-level parity, unpinned; the float32 result equals the numpy restatement
    tests/_nltv_oracle.py bit for bit.  ``tolerance`` > 0 stops the iterations early by the rule of
    tomobar_amd/convergence.py; ``last_prox()`` tells after which iteration.  There is no non-negativity switch (the drivers
    clamp before the prox) and no binary16 storage."""
    if gpu_id < 0:
        raise ValueError("The gpu_device must be a positive integer or zero")
    shape = tuple(int(v) for v in data.shape)
    if len(shape) not in (2, 3):
        raise ValueError("2D or 3D arrays must be provided only")
    tables = []
    for name, t, dtype in (("H_i", H_i, torch.uint16), ("H_j", H_j, torch.uint16), ("Weights", Weights, torch.float32)):
        t = ops.to_device(t, gpu_id)
        if t.dtype != dtype:
            raise ValueError(f"{name} must be a {str(dtype).replace('torch.', '')} array")
        if t.dim() < 2 or not t.is_contiguous():
            raise ValueError(f"{name} must be a C-contiguous array of shape (neighbours, *data.shape)")
        tables.append(t)
    neighbours = int(tables[2].shape[0])
    for name, t in zip(("H_i", "H_j", "Weights"), tables):
        if t.shape[0] != neighbours or t.numel() != neighbours * int(np.prod(shape)):
            raise ValueError(f"{name} has the shape {tuple(t.shape)}: ({neighbours}, {', '.join(map(str, shape))}) is expected")
    tables = [t.view((neighbours,) + shape) for t in tables]
    # _marched squeezes a singleton axis; the kernels take the stack as it is
    return _marched(lambda d, res, tol: ops.nltv(d.view(shape), res.view(shape), *tables, np.float32(regularisation_parameter),
                                                 iterations, tol),
                    data, gpu_id, out, tolerance)


def _prepare_stack(data, gpu_id: int) -> torch.Tensor:
    """the array of PatchSelect_cupy on the device: 2D, or 3D = a stack of slices along axis 0, nothing squeezed"""
    if gpu_id < 0:
        raise ValueError("The gpu_device must be a positive integer or zero")
    data = ops.to_device(data, gpu_id)
    if data.dtype != torch.float32:
        raise ValueError("The input data should be float32 data type")
    if data.ndim not in (2, 3):
        raise ValueError("2D or 3D arrays must be provided only")
    return ops.contiguous(data)


def _check_if_input_2d_or_3d(data) -> Tuple[torch.Tensor, bool, int]:
    """(array, treated_as_2d, squeezed_axis): a 3D input with a singleton axis runs the 2D kernels
    (reference: regularisersCuPy.py:299-315)."""
    if data.ndim == 2:
        return (data, True, 0)
    if data.ndim == 3:
        for i, extent in enumerate(data.shape):
            if extent == 1:
                return (data.squeeze(i), True, i)
        return (data, False, 0)
    raise ValueError("2D or 3D arrays must be provided only")
