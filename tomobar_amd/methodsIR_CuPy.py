"""Iterative reconstruction on MI355X behind the reference's ``RecToolsIRCuPy`` surface
(``tomobar/methodsIR_CuPy.py:36-667``): same constructor, methods, dictionaries and return shapes; arrays are
float32 ``torch.Tensor`` on ``cuda:<device_projector>`` where the reference uses ``cupy.ndarray``.

What differs is how a sub-iteration is executed.  The reference issues ~10 CuPy launches with temporaries plus two
ASTRA calls that rebuild a projector object each time (``methodsIR_CuPy.py:447-475``, ``astra_base.py:538-604``).
Here a FISTA-OS sub-iteration is

    residual  = forward-projection kernel with the (w *)(Ax - b) / KL epilogue, subset gathered by angle index
    gradient  = back-projection kernel whose epilogue applies  X = P+(X_t - g/L)  (and, when no proximal
                operator sits in between, the momentum update as well)
    prox      = ``tomo_pdtv`` / ``tomo_roftv``: one fused kernel per inner iteration (``tomo_tgv``: two)
    momentum  = one streaming kernel

on persistent buffers, all asynchronous on the current stream.  Scalar bookkeeping (t-sequence, step sizes) is done
in float32 exactly where the reference's NumPy-2 semantics make it float32 (``methodsIR_CuPy.py:438-475,523-554``).
"""

from __future__ import annotations

import collections
import contextlib
from typing import Optional, Union

import numpy as np
import torch
from numpy import float32

from . import ops
from .convergence import check_tolerance, relative_change
from .primal_dual_steps import pdhg_steps, spdhg_steps
from .projector import HipTools3D, geom_size
from .regularisersCuPy import check_prox_available, last_prox, prox_regul, reserve_prox_scratch
from .supp.dicts import dicts_check
from .supp.regularisers import has_wavelets
from .supp.suppTools import _apply_horiz_detector_padding, check_kwargs, perform_recon_crop


class _RunMonitor:
    """Early stopping and the run record of one driver call (``RecToolsIRCuPy.last_run``).

    ``_algorithm_["tolerance"]`` > 0: after every outer iteration the returned variable is compared with its value one outer
    iteration earlier (tomobar_amd/convergence.py) in one pass that also refreshes the snapshot (ops.rel_change with
    keep = the snapshot); over z-slabs the (num, den) pair is summed over the ranks first, so all ranks stop together.
    The snapshot volume exists only while that tolerance is on; with both tolerances off nothing is launched."""

    def __init__(self, rt, method: str, a: dict, start, r: Optional[dict] = None):
        self.slab = rt.slab
        self.tol = check_tolerance(a.get("tolerance"), "_algorithm_['tolerance']")
        self.inner = (r is not None and r.get("method") is not None
                      and check_tolerance(r.get("tolerance"), "_regularisation_['tolerance']") > 0.0)
        self.verbose = bool(a.get("verbose"))
        self.snap = start.clone() if self.tol > 0.0 else None   # v_0: the starting volume
        self.run = rt.last_run = {"method": method, "iterations_done": int(a["iterations"]), "converged": False,
                                  "rel_change": [], "prox_iterations": []}

    def prox_done(self) -> None:
        """after a proximal call: how many inner iterations it ran (recorded while the inner tolerance is on)"""
        if self.inner:
            self.run["prox_iterations"].append(last_prox()[0])

    def stop(self, k: int, v) -> bool:
        """after outer iteration k (1-based) with the returned variable in `v`: True if the loop ends here"""
        if self.snap is None:
            return False
        pair = ops.rel_change(v, self.snap, self.snap)
        if self.slab is not None:
            pair = self.slab.allreduce_sums(pair)
        d = relative_change(*pair)
        self.run["rel_change"].append(d)
        if not d < self.tol:
            return False
        self.run["iterations_done"], self.run["converged"] = k, True
        if self.verbose:
            print(f"{self.run['method']} stopped after iteration {k}: relative change {d:.3e} < tolerance {self.tol:.3e}")
        return True


@contextlib.contextmanager
def _planar_layouts(A):
    """PDHG's and SPDHG's protected region: no cached projector state, planar residuals and volumes on entry, and the same
    again on the way out, whatever was raised inside."""
    planar_volume = getattr(A, "set_volume_layout", None)
    A.invalidate()
    A.set_residual_layout("planar")
    if planar_volume is not None:
        planar_volume("planar")
    try:
        yield
    finally:
        A.set_residual_layout("planar")
        if planar_volume is not None:
            planar_volume("planar")
        A.invalidate()


# PDHG's work arrays: x-bar, g = A^T y, the TV duals q or the TGV fields (lists, empty where absent) and, with the preconditioner,
# the steps per voxel (else None)
_PdhgWork = collections.namedtuple("_PdhgWork", "xbar g q tgv_p tgv_q v vbar tau")


def _pdhg_work(shape, device, block, diag: bool) -> _PdhgWork:
    """One placed block of their own (the projector calls see ordinary tensors); `block` as in ``pdhg_steps``."""
    if block == "PD_TGV":
        xbar, g, tgv_p, tgv_q, v, vbar, *rest = ops.pdhg_tgv_work_arrays(shape, device, tau=diag)
        return _PdhgWork(xbar, g, [], tgv_p, tgv_q, v, vbar, rest[0] if diag else None)
    if diag:
        xbar, g, q, tau, _ = ops.pdhg_work_arrays(shape, device, block is not None, tau=True)
        return _PdhgWork(xbar, g, q, [], [], [], [], tau)
    xbar, g, q, _ = ops.pdhg_work_arrays(shape, device, block is not None)
    return _PdhgWork(xbar, g, q, [], [], [], [], None)


class RecToolsIRCuPy:
    """Iterative reconstruction algorithms (FISTA, ADMM, PDHG, SPDHG, OSEM, SIRT, CGLS, Landweber, power method).

    Args:
        DetectorsDimH (int): Horizontal detector dimension size.
        DetectorsDimH_pad (int): The amount of padding for the horizontal detector.
        DetectorsDimV (int, None): Vertical detector dimension size, 'None' for 2D or an integer for 3D.
        CenterRotOffset (float, np.ndarray): The Centre of Rotation (CoR) scalar or a vector for each angle.
        AnglesVec (np.ndarray): Vector of projection angles in radians.
        ObjSize (int): The size of the reconstructed object (a slice) defined as [recon_size, recon_size].
        device_projector (int, optional): GPU index. Defaults to 0.
        OS_number (int, optional): The number of ordered subsets, None for non-OS reconstruction.
    """

    def __init__(self, DetectorsDimH: int, DetectorsDimH_pad: int, DetectorsDimV: Union[int, None],
                 CenterRotOffset: Union[float, np.ndarray], AnglesVec: np.ndarray, ObjSize: int,
                 device_projector: int = 0, OS_number: Optional[int] = None, adjoint: str = "unmatched"):
        self.OS_number = OS_number
        # padding the detector enlarges the reconstruction grid; the result is cropped back (methodsIR_CuPy.py:72-79)
        self.objsize_user_given = ObjSize if DetectorsDimH_pad != 0 else None
        if DetectorsDimH_pad > 0:
            ObjSize = DetectorsDimH + 2 * DetectorsDimH_pad
        if DetectorsDimV == 0 or DetectorsDimV is None:
            DetectorsDimV = 1  # 2D is one slice of the 3D geometry (:81-82)
        self.geom = "3D"
        # (the keyword travels only when it is not the default: projector classes with the reference's constructor still fit)
        self.Atools = HipTools3D(DetectorsDimH, DetectorsDimH_pad, DetectorsDimV, AnglesVec, CenterRotOffset,
                                 ObjSize, "gpu", device_projector, OS_number,
                                 **({} if adjoint == "unmatched" else {"adjoint": adjoint}))
        self.power_seed = None  # set to an int for a reproducible power-method start vector
        self.last_run = None    # record of the most recent driver call (see _RunMonitor): iterations run, relative changes
        self.slab = None        # tomobar_amd.slab.SlabComm when this object reconstructs one z-slab of a larger volume

    @property
    def slab(self):
        return self._slab

    @slab.setter
    def slab(self, comm):
        self._slab = comm
        self.Atools.slab = comm   # the projector exchanges ghost detector rows itself when a vertical CoR component is set

    @property
    def adjoint(self) -> str:
        """Which back projector the drivers use (no reference counterpart): "unmatched" (default), ASTRA's voxel-driven
        one, or "matched", the exact transpose of the forward projector -- what CGLS, SIRT, Landweber and the power
        method assume (docs/kernels/bp_matched.md).  Forwards to ``Atools.adjoint``."""
        return self.Atools.adjoint

    @adjoint.setter
    def adjoint(self, value):
        self.Atools.adjoint = value

    @property
    def OS_number(self) -> int:
        return self._OS_number

    @OS_number.setter
    def OS_number(self, value):
        self._OS_number = 1 if value is None else value

    @property
    def objsize_user_given(self):
        return self._objsize_user_given

    @objsize_user_given.setter
    def objsize_user_given(self, value):
        self._objsize_user_given = value

    def reserve_scratch(self, _regularisation_: Union[dict, None]) -> None:
        """Optional set-up call (no reference counterpart): allocate and PLACE the TV operators' scratch arena for this
        geometry now.  ``FISTA`` / ``ADMM`` / ``OSEM`` do it themselves at the start of their first call; calling it right
        after the constructor -- before the projection data are moved to the GPU -- lets the placement search see an
        empty device, where it ends on a block of the fast class in 5 of 5 processes instead of 2 of 5
        (docs/kernels/placement.md, profiles/r5f_bench_reserve_order_ab.txt).  A later call is a no-op."""
        if _regularisation_ is not None and _regularisation_.get("method") is not None:
            reserve_prox_scratch(self, self.Atools.vol_shape(), _regularisation_)

    # ------------------------------------------------------------------ operators
    def _Ax(self, x, sub_ind: int = 1, os: bool = False):
        return self.Atools._forwprojOSCuPy(x, os_index=sub_ind) if os else self.Atools._forwprojCuPy(x)

    def _Atb(self, b, sub_ind: int = 1, os: bool = False):
        return self.Atools._backprojOSCuPy(b, os_index=sub_ind) if os else self.Atools._backprojCuPy(b)

    # ------------------------------------------------------------------ shared set-up / tear-down
    def _gdot(self, x, y) -> float:
        """Inner product over the whole volume / sinogram (sum-all-reduced over the z-slabs when sharded)."""
        v = ops.dot(x, y)
        return v if self.slab is None else self.slab.allreduce_sum(v)

    def _new_vol(self, fill=None):
        v = torch.empty(self.Atools.vol_shape(), dtype=torch.float32, device=self.Atools._device)
        if fill is not None:
            ops.fill(v, fill)
        return v

    def _prepare_data(self, _data_, _algorithm_, _regularisation_, method_run):
        self._given = _data_.get("projection_data") if isinstance(_data_, dict) else None  # decides the array library of the result
        d, a, r = dicts_check(self, _data_, _algorithm_, _regularisation_, method_run=method_run)
        check_prox_available(self, self.Atools.vol_shape(), r)   # before any projector call
        d["projection_data"] = _apply_horiz_detector_padding(d["projection_data"], self.Atools.detectors_x_pad, True)
        expect = self.Atools.sino_shape(None)
        if tuple(d["projection_data"].shape) != expect:
            raise ValueError(f"projection data has shape {tuple(d['projection_data'].shape)} after axis swap and "
                             f"padding, the geometry expects {expect}")
        if d["projection_data"].dtype != torch.float32:
            raise ValueError("projection data must be float32")
        return d, a, r

    def _finalise(self, x, _algorithm_):
        given = getattr(self, "_given", None)
        self._given = None
        if self.objsize_user_given is not None:
            return ops.like(perform_recon_crop(x, self.objsize_user_given), given)  # cropped result is not masked (:477-478)
        return ops.like(check_kwargs(x, cupyrun=True, recon_mask_radius=_algorithm_["recon_mask_radius"]), given)

    def __common_initialisation(self, _data_, _algorithm_, _regularisation_, method_run):
        d, a, r = self._prepare_data(_data_, _algorithm_, _regularisation_, method_run)
        # (PDHG with the diagonal preconditioner takes its steps from A 1 and A^T 1: no operator norm, no power method)
        if a.get("lipschitz_const") is None and not (method_run == "PDHG" and a["PDHG_preconditioner"] == "diagonal"):
            # SPDHG steps with one bound for every subset's operator; the other drivers with subset 0's (the reference's)
            a["lipschitz_const"] = self._largest_subset_norm() if method_run == "SPDHG" else self.powermethod(d)
        rec_dim = geom_size(self.Atools.vol_geom)
        x0 = None
        if a["initialise"] is not None:
            if tuple(a["initialise"].shape) == rec_dim:
                x0 = ops.contiguous(ops.to_device(a["initialise"], self.Atools.device_index)).clone()
            else:
                print(f"Provided initialisation (array) has incorrect dimensions, the correct dims are {rec_dim}. "
                      "Zero initialisation is used.")
        if x0 is None:
            x0 = self._new_vol(1.0 if method_run == "OSEM" else 0.0)
        use_os = self.OS_number > 1
        w = ops.pwls_weights(d["projection_data"], self.slab) if _data_["data_fidelity"] in ["PWLS", "SWLS"] else None
        # the TV operators' scratch arena is allocated and placed here, at set-up, not inside the first proximal step
        # (PDHG and SPDHG run no prox: their work arrays are a placed block of their own)
        if method_run not in ("PDHG", "SPDHG"):
            reserve_prox_scratch(self, rec_dim, r)
        return (d, a, r, x0, w, use_os)

    # ------------------------------------------------------------------ power method
    def powermethod(self, _data_: dict) -> float:
        """Largest eigenvalue of A^T A (of subset 0's operator when OS_number > 1) by 15 power iterations
        (reference: methodsIR_CuPy.py:311-354)."""
        if _data_.get("data_fidelity") is None:
            _data_["data_fidelity"] = "LS"
        return self._power_iterations(0 if self.OS_number > 1 else None)

    def _largest_subset_norm(self) -> float:
        """The largest of the power-method values of the OS_number subsets' operators (each from the same start vector)."""
        return max(self._power_iterations(j if self.OS_number > 1 else None) for j in range(self.OS_number))

    def _power_iterations(self, sub) -> float:
        """Largest eigenvalue of A_sub^T A_sub (`sub` None: all angles) by 15 power iterations."""
        A = self.Atools
        gen = None
        if self.power_seed is not None:
            gen = torch.Generator(device=A._device)
            gen.manual_seed(int(self.power_seed))
        x1 = torch.randn(A.vol_shape(), dtype=torch.float32, device=A._device, generator=gen)
        y = A.forward(x1, sub)  # PWLS weights are all-ones here (:331-333,:344-346): no effect
        s = 1.0
        for _ in range(15):
            A.backward(y, sub, out=x1)
            s = ops.norm2(x1)
            if self.slab is not None:  # the eigenvector spans all slabs: global 2-norm
                s = float(np.sqrt(self.slab.allreduce_sum(s * s)))
            s = float32(s)
            ops.scale(float32(1.0) / s, x1, x1)
            A.forward(x1, sub, out=y)
        return float(s)

    # ------------------------------------------------------------------ FISTA
    def FISTA(self, _data_: dict, _algorithm_: Union[dict, None] = None,
              _regularisation_: Union[dict, None] = None) -> torch.Tensor:
        """Fast Iterative Shrinkage-Thresholding Algorithm with optional ordered subsets and ROF_TV / PD_TV / TGV proximal
        regularisation (reference: methodsIR_CuPy.py:401-484).  Returns the float32 volume ``[detY, N, N]``."""
        (d, a, r, x0, w, use_os) = self.__common_initialisation(_data_, _algorithm_, _regularisation_, "FISTA")
        A = self.Atools
        L_inv = float32(1.0 / a["lipschitz_const"])
        b = d["projection_data"]
        fid = self.data_fidelity
        nonneg = bool(a["nonnegativity"])
        has_prox = r["method"] is not None

        # ring-artefact data terms (BASELINE configs[4]; not in this reference version, see supp/dicts.py here):
        # Group-Huber offsets r [detY, detX] (one per detector pixel, constant over the angles) and / or SWLS weighting
        ring_lambda = d.get("ringGH_lambda")
        use_ring = ring_lambda is not None
        use_swls = fid == "SWLS"
        # Huber / Student's-t data terms: the (weighted) residual is re-weighted before the back projection
        robust = None
        if d.get("huber_threshold") is not None:
            robust = ("huber", float32(d["huber_threshold"]))
        elif d.get("studentst_threshold") is not None:
            robust = ("studentst", float32(d["studentst_threshold"]))
        if use_ring:
            ring_acc = float32(d["ringGH_accelerate"])
            r_shape = (A.nz, A.nu)
            r_cur = torch.zeros(r_shape, dtype=torch.float32, device=A._device)
            r_old = torch.zeros(r_shape, dtype=torch.float32, device=A._device)
            r_x = torch.zeros(r_shape, dtype=torch.float32, device=A._device)

        t = float32(1.0)
        X = x0                      # doubles as X_old at the start of every sub-iteration
        res = {}
        X_grad = self._new_vol() if has_prox else None
        X_prox = self._new_vol() if has_prox else None

        # the transposed X_t that A.momentum leaves in the projector context is a one-shot token for the NEXT residual of
        # this loop; nothing of it may survive this call (a later call's X_t can land at the same address)
        A.invalidate()
        # on the plain LS / PWLS / KL path nobody but the back projector reads the residual: producer and consumer use the
        # quad-interleaved layout (HipTools3D.set_residual_layout); the ring terms and the vertical CoR resampling read it
        # as [detY, angles, detX] and keep the planar one
        zquad = not (use_ring or use_swls) and not getattr(A, "has_vertical_shift", False)
        A.set_residual_layout("zquad" if zquad else "planar")
        # with a prox between gradient step and momentum X_t has one producer (A.momentum) and two consumers (A.residual,
        # A.grad_step): where the residual runs quad-interleaved and every subset's kernels read it, X_t is held
        # quad-interleaved as well (HipTools3D.set_volume_layout) and x0 is converted once.  Without a prox
        # (grad_step_momentum), on a z-slab and with a projector object that does not know the layout it stays planar.
        vquad = (has_prox and zquad and self.slab is None and hasattr(A, "volume_zquad_ok")
                 and A.residual_layout() == "zquad"   # (the matched back projector keeps the planar residual)
                 and all(A.volume_zquad_ok(s if use_os else None) for s in range(self.OS_number)))
        n_sub_total = a["iterations"] * self.OS_number
        mon = _RunMonitor(self, "FISTA", a, x0, r)
        try:
            if vquad:
                A.set_volume_layout("zquad")
                X_t = A.volume_to_zquad(x0)
            else:
                X_t = x0.clone()
            for it_no in range(a["iterations"]):
                for sub_ind in range(self.OS_number):
                    sub = sub_ind if use_os else None
                    t_old = t
                    if sub not in res:
                        res[sub] = A.residual_buffer(sub)
                    if use_ring:
                        # res = (A_s X_t - b_s) + accelerate * r_x ;  r = r_x - (1/L) sum_angles res ;  then the PWLS weights
                        A.residual_ring(X_t, b, r_x, ring_acc, sub, res[sub])
                        A.ring_reduce(res[sub], w if fid == "PWLS" else None, r_x, L_inv, sub, r_cur)
                        if robust is not None:
                            A.robust_apply(res[sub], *robust)
                    elif use_swls:
                        A.residual(X_t, b, None, "LS", sub, res[sub])
                        A.swls_apply(res[sub], w, float32(d["beta_SWLS"]), sub)
                        if robust is not None:
                            A.robust_apply(res[sub], *robust)
                    else:
                        A.residual(X_t, b, w, fid, sub, res[sub], robust=robust)
                    t = float32((float32(1.0) + np.sqrt(float32(1.0) + float32(4.0) * t * t)) * float32(0.5))
                    beta = float32((t_old - float32(1.0)) / t)
                    if not has_prox:
                        # X <- P+(X_t - grad/L) and X_t <- X + beta (X - X_old) inside the back-projection epilogue
                        A.grad_step_momentum(res[sub], X_t, X, L_inv, beta, nonneg, sub)
                    else:
                        A.grad_step(res[sub], X_t, X_grad, L_inv, nonneg, sub)
                        prox_regul(self, X_grad, r, out=X_prox)
                        mon.prox_done()
                        if it_no * self.OS_number + sub_ind + 1 < n_sub_total:
                            # also leaves X_t transposed for the next forward projection; after the LAST sub-iteration X_t
                            # is never read again (the reference still computes it, methodsIR_CuPy.py:475): skipped
                            A.momentum(X_prox, X, X_t, beta)
                        X, X_prox = X_prox, X
                    if use_ring:
                        # r <- soft(r, lambda) ;  r_x = r + beta (r - r_old)
                        A.ring_update(r_cur, r_old, r_x, float32(ring_lambda), beta)
                # (the momentum of the last sub-iteration is already launched when the loop ends here: X is returned, not X_t)
                if mon.stop(it_no + 1, X):
                    break
        finally:
            A.set_residual_layout("planar")
            if vquad:
                A.set_volume_layout("planar")
            A.invalidate()
        return self._finalise(X, a)

    # ------------------------------------------------------------------ ADMM
    def ADMM(self, _data_: dict, _algorithm_: Union[dict, None] = None,
             _regularisation_: Union[dict, None] = None) -> torch.Tensor:
        """Linearised, relaxed ADMM with optional ordered subsets (reference: methodsIR_CuPy.py:486-585).

        Divergence from the reference, on purpose: ``regul_param / ADMM_rho_const`` is applied to a private copy of
        the regularisation dictionary (the reference rewrites the caller's dictionary on every call, :526-528); LLT_ROF's
        second weight ``regul_param2`` is divided likewise, and so is the wavelet threshold of a ``_WAVELETS`` method."""
        (d, a, r, x0, w, use_os) = self.__common_initialisation(_data_, _algorithm_, _regularisation_, "ADMM")
        A = self.Atools
        b = d["projection_data"]
        fid = self.data_fidelity
        nonneg = bool(a["nonnegativity"])
        has_prox = r["method"] is not None
        rho, alpha = a["ADMM_rho_const"], a["ADMM_relax_par"]
        tau = float32(0.9 / (a["lipschitz_const"] + rho))
        r_local = dict(r)
        if has_prox:
            r_local["regul_param"] = r["regul_param"] / rho
            # both weights multiply the regulariser: LLT_ROF's second weight and the threshold of the WAVELETS suffix
            if ("LLT_ROF" in r["method"] or has_wavelets(r["method"])) and "regul_param2" in r:
                r_local["regul_param2"] = r["regul_param2"] / rho

        x = x0
        z = x0.clone()
        u = self._new_vol(0.0)
        zu = self._new_vol()
        res = {}
        # the residual goes from the forward projector straight into the fused z-update: quad-interleaved (see FISTA)
        A.set_residual_layout("planar" if getattr(A, "has_vertical_shift", False) else "zquad")
        mon = _RunMonitor(self, "ADMM", a, x0, r)
        try:
            for iter_no in range(a["iterations"]):
                for sub_ind in range(self.OS_number):
                    sub = sub_ind if use_os else None
                    if sub not in res:
                        res[sub] = A.residual_buffer(sub)
                    A.residual(z, b, w, fid, sub, res[sub])
                    # z-update, projection, over-relaxation (from the third outer iteration on) and zu = z + u
                    A.admm_z_update(res[sub], z, x, u, zu, tau, float32(rho), iter_no > 1, float32(1.0 - alpha),
                                    float32(alpha), nonneg, sub)
                    if has_prox:
                        prox_regul(self, zu, r_local, out=x)
                        mon.prox_done()
                    else:
                        x, zu = zu, x
                ops.admm_dual(u, z, x)  # once per outer iteration (:566)
                if a["verbose"] and np.mod(iter_no, (round)(a["iterations"] / 5) + 1) == 0:
                    print("ADMM iteration (", iter_no + 1, ") using", r["method"], "regularisation")
                if mon.stop(iter_no + 1, x):
                    break
        finally:
            A.set_residual_layout("planar")
        return self._finalise(x, a)

    # ------------------------------------------------------------------ PDHG
    def PDHG(self, _data_: dict, _algorithm_: Union[dict, None] = None,
             _regularisation_: Union[dict, None] = None) -> torch.Tensor:
        """Primal-dual hybrid gradient (Chambolle-Pock) on  min_x F(Ax) + lambda TV(x)  itself (no reference counterpart in
        this reference version; the algorithm is stated in docs/kernels/pdhg.md, formula-level parity, unpinned).
        ``_data_["data_fidelity"]`` is "LS", "KL" or "L1" -- the non-smooth terms exactly, no re-weighting and no clamp of
        Ax --, ``_regularisation_["method"]`` None or "PD_TV": the TV term sits in the dual of the outer problem, so an
        iteration is one forward projection, one matched back projection and one stencil pass, with no inner loop.
        ``"PD_TGV"`` puts the second-order TGV term lambda min_v (alpha1 |grad x - v| + alpha0 |E v|) there instead
        (``regul_param``, ``TGV_alpha1``, ``TGV_alpha2``): one TGV dual and one TGV primal launch per iteration.
        ``_algorithm_["PDHG_ratio"]`` is sigma / tau (default 1).  ``_data_["stripe_lambda"]`` = mu (default None: off) adds a
        stripe variable against ring artefacts: min_{x, s} F(Ax + Ss) + lambda R(x) + mu |s|_1 with one offset s[z, u] per
        detector pixel, added to every angle; ``last_run["stripes"]`` returns it as ``[detY, detX]``.  Needs
        ``adjoint="matched"``; no ordered subsets, no z-slabs.  Returns the float32 volume ``[detY, N, N]``."""
        (d, a, r, x, _, _) = self.__common_initialisation(_data_, _algorithm_, _regularisation_, "PDHG")
        A = self.Atools
        b = d["projection_data"]
        fid = self.data_fidelity
        nonneg = bool(a["nonnegativity"])
        block = r.get("method")   # dicts_check lets nothing but None, "PD_TV" and "PD_TGV" through
        diag = a["PDHG_preconditioner"] == "diagonal"
        # the stripe variable s (one offset per detector pixel, added to every angle; mu |s|_1): off unless the key is given
        stripes = d.get("stripe_lambda") is not None
        n_angles = int(b.shape[1])
        lam = float32(r["regul_param"]) if block is not None else None
        if block == "PD_TGV":   # the radii of the two balls: r1 = lambda alpha1, r0 = lambda alpha0
            r1, r0 = lam * float32(r["TGV_alpha1"]), lam * float32(r["TGV_alpha2"])

        # the steps: float32 host scalars (with the preconditioner the numerators; the arrays are built below)
        nd = 3 if A.vol_shape()[0] > 1 else 2
        st = pdhg_steps(a.get("lipschitz_const"), n_angles, nd, block, a["PDHG_ratio"], diag, stripes, d.get("stripe_lambda"))

        # the work arrays and their fills
        w = _pdhg_work(A.vol_shape(), A._device, block, diag)
        w.xbar.copy_(x)
        for field in (*w.q, *w.tgv_p, *w.tgv_q, *w.v, *w.vbar):
            ops.fill(field, 0.0)
        y = torch.empty_like(b)
        ops.fill(y, 0.0)
        proj = torch.empty_like(b)
        if stripes:   # s, s-bar [nz, nu] and the segments' partial sums of y along the angles
            s, sbar = (torch.empty((b.shape[0], b.shape[2]), dtype=torch.float32, device=b.device) for _ in range(2))
            part = torch.empty((ops.pdhg_stripe_segments(n_angles), b.shape[0], b.shape[2]), dtype=torch.float32, device=b.device)
            for field in (s, sbar, part):
                ops.fill(field, 0.0)

        with _planar_layouts(A):
            mon = _RunMonitor(self, "PDHG", a, x)
            self.last_run["preconditioner"] = "diagonal" if diag else None
            if block == "PD_TGV":
                self.last_run["regulariser"] = "PD_TGV"
            sigma_y, tau_x = st.sigma, st.tau   # the steps of y and x: one each, or with the preconditioner one per element
            if diag:   # from the row and column sums of A; g and proj hold the ones, the loop overwrites both before it reads them
                sigma_y, tau_x = torch.empty_like(b), w.tau
                row_add = (float32(1),) if stripes else ()   # with the stripe variable a row of [A S] gains one entry 1
                ops.fill(w.g, 1.0)
                A.forward(w.g, None, out=sigma_y)
                ops.pdhg_diag_steps(sigma_y, sigma_y, st.numer_sigma, *row_add)
                ops.fill(proj, 1.0)
                A.backward(proj, None, out=tau_x)
                ops.pdhg_diag_steps(tau_x, tau_x, st.numer_tau, st.col_add)

            # which launches an iteration makes is settled here, once (each still looked up on `ops` when it is made)
            if stripes:   # step 2 on A x-bar + S s-bar, the sums of y along the angles in the same pass; then step 6
                def sino_dual():
                    ops.pdhg_sino_dual_stripe(y, proj, b, sbar, part, fid, sigma_y)
                    ops.pdhg_stripe_update(s, sbar, part, n_angles, st.tau_s, st.theta)
            elif diag:
                def sino_dual():
                    ops.pdhg_sino_dual_diag(y, proj, b, sigma_y, fid)
            else:
                def sino_dual():
                    ops.pdhg_sino_dual(y, proj, b, fid, sigma_y)
            if block == "PD_TGV":
                def primal():
                    ops.pdhg_tgv_dual(w.xbar, w.vbar, w.tgv_p, w.tgv_q, st.sigma_p, st.sigma_q, r1, r0)
                    ops.pdhg_tgv_primal(x, w.xbar, w.g, w.v, w.vbar, w.tgv_p, w.tgv_q, tau_x, st.tau_v, nonneg)
            elif diag:
                def primal():
                    ops.pdhg_primal_diag(x, w.xbar, w.g, w.q, tau_x, nonneg)
            else:
                def primal():
                    ops.pdhg_primal(x, w.xbar, w.g, w.q, tau_x, nonneg)
            has_tv = block == "PD_TV"

            for k in range(a["iterations"]):
                A.forward(w.xbar, None, out=proj)
                sino_dual()
                A.backward(y, None, out=w.g)
                if has_tv:
                    ops.pdhg_tv_dual(w.xbar, w.q, st.sigma, lam, r["methodTV"])
                primal()
                if a["verbose"] and np.mod(k, (round)(a["iterations"] / 5) + 1) == 0:
                    print("PDHG iteration (", k + 1, ") using", block, "regularisation")
                if mon.stop(k + 1, x):
                    break
        if stripes:   # without the detector-padding columns, in the caller's array library
            pad = A.detectors_x_pad
            self.last_run["stripes"] = ops.like(ops.contiguous(s[:, pad:s.shape[1] - pad]), getattr(self, "_given", None))
        return self._finalise(x, a)

    # ------------------------------------------------------------------ SPDHG
    def SPDHG(self, _data_: dict, _algorithm_: Union[dict, None] = None,
              _regularisation_: Union[dict, None] = None) -> torch.Tensor:
        """Stochastic PDHG over the ordered subsets (Chambolle, Ehrhardt, Richtarik, Schoenlieb 2018; no reference
        counterpart in this reference version; the algorithm is stated in docs/kernels/spdhg.md, formula-level parity,
        unpinned): PDHG's problem, data terms and TV block, but one update touches one subset of angles or the TV block,
        drawn with ``numpy.random.default_rng(_algorithm_["SPDHG_seed"])``.  ``iterations`` counts epochs: OS_number block
        updates, twice as many with TV, i.e. the projector work of one PDHG iteration.  ``lipschitz_const`` bounds every
        subset's operator (absent: the largest power-method value of the subsets).  Needs ``adjoint="matched"``; any
        OS_number >= 1; no z-slabs.  Returns the float32 volume ``[detY, N, N]``."""
        (d, a, r, x, _, use_os) = self.__common_initialisation(_data_, _algorithm_, _regularisation_, "SPDHG")
        A = self.Atools
        fid = self.data_fidelity
        nonneg = bool(a["nonnegativity"])
        has_tv = r.get("method") is not None     # dicts_check lets nothing but None and "PD_TV" through for SPDHG
        m = self.OS_number
        blocks = 2 * m if has_tv else m          # E: the block updates of one epoch
        draws = np.random.default_rng(a["SPDHG_seed"]).integers(0, blocks, size=a["iterations"] * blocks)
        nd = 3 if A.vol_shape()[0] > 1 else 2
        sigma_A, sigma_G, tau, w_A, w_G = spdhg_steps(a["lipschitz_const"], nd, m, has_tv, a["PDHG_ratio"])
        lam = float32(r["regul_param"]) if has_tv else None

        # z = sum K_j^T y_j, delta and the TV fields live in a placed block of their own; b and y are held subset-major,
        # every subset one contiguous [nz, Na_j, Nu] array (the caller's data are gathered once, never written)
        z, delta, q, e, _ = ops.spdhg_work_arrays(A.vol_shape(), A._device, has_tv)
        for field in [z] + q:
            ops.fill(field, 0.0)
        subs = [j if use_os else None for j in range(m)]
        sizes = [int(np.prod(A.sino_shape(sub))) for sub in subs]
        offsets = np.concatenate(([0], np.cumsum(sizes)))
        full = d["projection_data"]
        b_all = torch.empty(int(offsets[-1]), dtype=torch.float32, device=full.device)
        y_all = torch.empty_like(b_all)
        ops.fill(y_all, 0.0)
        proj_all = torch.empty(max(sizes), dtype=torch.float32, device=full.device)
        b, y, proj = [], [], []
        for j, sub in enumerate(subs):
            shape = A.sino_shape(sub)
            b.append(b_all[offsets[j]:offsets[j + 1]].view(shape))
            y.append(y_all[offsets[j]:offsets[j + 1]].view(shape))
            proj.append(proj_all[:sizes[j]].view(shape))
            if use_os:
                index = torch.from_numpy(np.ascontiguousarray(A.subset_indices(j), dtype=np.int64)).to(full.device)
                torch.index_select(full, 1, index, out=b[j])
            else:
                b[j].copy_(full)
        if nonneg:
            ops.clamp_min(x, 0.0)     # SPDHG's first primal step with z-bar = 0

        with _planar_layouts(A):
            mon = _RunMonitor(self, "SPDHG", a, x)
            done = [0, 0]
            mon.run["block_updates"] = (0, 0)
            for epoch in range(a["iterations"]):
                for j in draws[epoch * blocks:(epoch + 1) * blocks]:
                    if j < m:
                        A.forward(x, subs[j], out=proj[j])
                        ops.spdhg_sino_dual(y[j], proj[j], b[j], fid, sigma_A)
                        A.backward(proj[j], subs[j], out=delta)
                        ops.spdhg_primal(x, z, delta, tau, w_A, nonneg)
                    else:
                        ops.spdhg_tv_dual(x, q, e, sigma_G, lam, r["methodTV"])
                        ops.spdhg_tv_primal(x, z, e, tau, w_G, nonneg)
                    done[int(j >= m)] += 1
                mon.run["block_updates"] = tuple(done)
                if a["verbose"] and np.mod(epoch, (round)(a["iterations"] / 5) + 1) == 0:
                    print("SPDHG epoch (", epoch + 1, ") using", r.get("method"), "regularisation")
                if mon.stop(epoch + 1, x):
                    break
        return self._finalise(x, a)

    # ------------------------------------------------------------------ simple iterative methods
    def Landweber(self, _data_: dict, _algorithm_: Union[dict, None] = None) -> torch.Tensor:
        """x <- x - tau A^T(Ax - b)   (reference: methodsIR_CuPy.py:128-172)."""
        d, a, _ = self._prepare_data(_data_, _algorithm_, None, "Landweber")
        A = self.Atools
        b = d["projection_data"]
        x = self._new_vol(0.0)
        step = float32(a["tau_step_lanweber"])
        # the residual goes straight from the forward projector into the fused gradient step: quad-interleaved (see FISTA)
        A.set_residual_layout("planar" if getattr(A, "has_vertical_shift", False) else "zquad")
        try:
            res = A.residual_buffer(None)
            mon = _RunMonitor(self, "Landweber", a, x)
            for k in range(a["iterations"]):
                A.residual(x, b, None, "LS", None, res)
                # x - tau*g with the clamp as a separate rounding step, like the reference's in-place ops
                A.grad_step(res, x, x, step, a["nonnegativity"], None)
                if mon.stop(k + 1, x):
                    break
        finally:
            A.set_residual_layout("planar")
        return self._finalise(x, a)

    def SIRT(self, _data_: dict, _algorithm_: Union[dict, None] = None) -> torch.Tensor:
        """x <- x + C A^T (R (b - Ax))   (reference: methodsIR_CuPy.py:174-231)."""
        d, a, _ = self._prepare_data(_data_, _algorithm_, None, "SIRT")
        A = self.Atools
        b = d["projection_data"]
        ones_v = self._new_vol(1.0)
        R = A.forward(ones_v)
        ops.recip_safe(R, R)
        ones_s = torch.empty_like(b)
        ops.fill(ones_s, 1.0)
        Cm = A.backward(ones_s)
        ops.recip_safe(Cm, Cm)
        del ones_s
        x = ones_v
        res = torch.empty_like(b)
        upd = self._new_vol()
        mon = _RunMonitor(self, "SIRT", a, x)
        for k in range(a["iterations"]):
            A.forward(x, None, out=res)
            ops.axpby(1.0, b, -1.0, res)   # b - Ax
            ops.mul(R, res)
            A.backward(res, None, out=upd)
            ops.mul(Cm, upd)
            ops.axpby(1.0, upd, 1.0, x)
            if a["nonnegativity"]:
                ops.clamp_min(x, 0.0)
            if mon.stop(k + 1, x):
                break
        return self._finalise(x, a)

    def CGLS(self, _data_: dict, _algorithm_: Union[dict, None] = None) -> torch.Tensor:
        """Conjugate-gradient least squares (reference: methodsIR_CuPy.py:233-309)."""
        d, a, _ = self._prepare_data(_data_, _algorithm_, None, "CGLS")
        A = self.Atools
        x = self._new_vol(0.0)
        r_vec = d["projection_data"].clone()
        dvec = A.backward(r_vec)
        normr2 = float32(self._gdot(dvec, dvec))
        Ad = torch.empty_like(r_vec)
        s = self._new_vol()
        mon = _RunMonitor(self, "CGLS", a, x)
        for k in range(a["iterations"]):
            A.forward(dvec, None, out=Ad)
            alpha = float32(normr2 / float32(self._gdot(Ad, Ad)))
            ops.axpby(alpha, dvec, 1.0, x)
            ops.axpby(-alpha, Ad, 1.0, r_vec)
            A.backward(r_vec, None, out=s)
            normr2_new = float32(self._gdot(s, s))
            beta = float32(normr2_new / normr2)
            normr2 = normr2_new
            ops.axpby(1.0, s, beta, dvec)  # d = s + beta d
            if a["nonnegativity"]:
                ops.clamp_min(x, 0.0)
            if mon.stop(k + 1, x):
                break
        return self._finalise(x, a)

    def OSEM(self, _data_: dict, _algorithm_: Union[dict, None] = None,
             _regularisation_: Union[dict, None] = None) -> torch.Tensor:
        """OSEM / MLEM for emission data as the reference writes it (methodsIR_CuPy.py:587-667): the multiplicative
        update uses ``backproj * normalisation`` with ``normalisation = clip(A_0^T 1, 1e-8)`` (:654; the textbook
        form divides -- kept as is so results match the reference)."""
        (d, a, r, x, w, use_os) = self.__common_initialisation(_data_, _algorithm_, _regularisation_, "OSEM")
        A = self.Atools
        b = d["projection_data"]
        eps = 1e-8
        sub0 = 0 if use_os else None
        ones_s = torch.empty(A.sino_shape(sub0), dtype=torch.float32, device=A._device)
        ops.fill(ones_s, 1.0)
        normalisation = A.backward(ones_s, sub0)
        ops.clamp_min(normalisation, eps)
        del ones_s
        ratio, back = {}, self._new_vol()
        mon = _RunMonitor(self, "OSEM", a, x, r)
        for k in range(a["iterations"]):
            for sub_ind in range(self.OS_number):
                sub = sub_ind if use_os else None
                if sub not in ratio:
                    ratio[sub] = torch.empty(A.sino_shape(sub), dtype=torch.float32, device=A._device)
                # ratio = b_s / clip(A_s x, eps) as the forward projector's epilogue
                A.residual(x, b, None, "RATIO", sub, ratio[sub])
                A.backward(ratio[sub], sub, out=back)
                ops.mul(normalisation, back)
                ops.mul(back, x)
                if r["method"] is not None:
                    x = prox_regul(self, x, r)
                    mon.prox_done()
            if mon.stop(k + 1, x):
                break
        return self._finalise(x, a)
