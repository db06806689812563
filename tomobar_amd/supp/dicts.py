"""Validation and default population of the ``_data_`` / ``_algorithm_`` / ``_regularisation_`` dictionaries.

Behavioural mirror of the reference's ``tomobar/supp/dicts.py:6-184`` (same keys, defaults, error types and the
same in-place effects on the caller's dictionaries), written table-driven.  Divergence, on purpose: the axis
swap materialises a C-contiguous device array (the reference keeps a strided view and later hands its raw
pointer to ASTRA, astra_base.py:533-535).
"""

from __future__ import annotations

import numbers
from typing import Optional

from .. import ops
from ..convergence import check_tolerance
from .funcs import _data_dims_swapper
from .regularisers import (NLTV_ITERATIONS, NLTV_NEIGHBOURS, NLTV_TABLES, WAVELETS_DEFAULTS, has_wavelets, is_nltv, kind_of,
                           nltv_check, nltv_iterations, nltv_tables, slicewise_of)

LABELS_3D = ["detY", "angles", "detX"]
LABELS_2D = ["angles", "detX"]

# default outer-iteration counts: method -> (classical, ordered-subsets)   (dicts.py:101-133)
_DEFAULT_ITERATIONS = {
    "SIRT": (200, 200), "CGLS": (30, 30), "power": (15, 15), "Landweber": (1500, 1500),
    "OSEM": (300, 15), "FISTA": (400, 20), "ADMM": (400, 10), "PDHG": (500, 500),
    "SPDHG": (100, 100),   # epochs (docs/kernels/spdhg.md)
}
_NO_OS_METHODS = {"SIRT", "CGLS", "Landweber"}
_NO_LIPSCHITZ = {"SIRT", "CGLS", "power", "Landweber", "OSEM"}

_ALGORITHM_DEFAULTS = (("initialise", None), ("nonnegativity", False), ("recon_mask_radius", 1.0),
                       ("tolerance", 0.0), ("verbose", False))
_REGULARISATION_DEFAULTS = (("regul_param", 0.001), ("iterations", 150), ("tolerance", 0.0),
                            ("time_marching_step", 0.005), ("PD_LipschitzConstant", 12.0), ("methodTV", 0),
                            ("device_regulariser", 0))


def _nltv_keys(self, reg: dict) -> None:
    """The keys of the NLTV method (supp/regularisers.py; those of the reference's legacy demo): the three tables are
    required and checked -- dtype, one shape (K, ...) for all three, K times the voxels of the volume --, ``NumNeighb`` is
    filled with K and must equal it, and the iteration count ``IterNumb`` (the demo's key) becomes ``iterations``."""
    nltv_tables(reg)
    for key, want in zip(NLTV_TABLES, ("uint16", "uint16", "float32")):
        got = str(getattr(reg[key], "dtype", None)).split(".")[-1]
        if got != want:
            raise ValueError(f"_regularisation_['{key}'] must be a {want} array, got {got}")
    shapes = [tuple(int(v) for v in reg[key].shape) for key in NLTV_TABLES]
    if len(shapes[2]) not in (3, 4) or shapes[0] != shapes[2] or shapes[1] != shapes[2]:
        raise ValueError(f"the NLTV tables must share one shape (neighbours, *volume), got {shapes[0]}, {shapes[1]} and {shapes[2]}")
    neighbours = shapes[2][0]
    vol_shape = getattr(self.Atools, "vol_shape", None)
    if callable(vol_shape):
        vol = tuple(int(v) for v in vol_shape())
        nvox = 1
        for v in vol:
            nvox *= v
        per_neighbour = 1
        for v in shapes[2][1:]:
            per_neighbour *= v
        if per_neighbour != nvox:
            raise ValueError(f"the NLTV tables have the shape {shapes[2]}: (neighbours, *volume) with the volume {vol} is expected")
    if reg.get(NLTV_NEIGHBOURS) is None:
        reg[NLTV_NEIGHBOURS] = neighbours
    if int(reg[NLTV_NEIGHBOURS]) != neighbours:
        raise ValueError(f"_regularisation_['{NLTV_NEIGHBOURS}'] = {reg[NLTV_NEIGHBOURS]}, the tables hold {neighbours} neighbours")
    if reg.get(NLTV_ITERATIONS) is not None:
        reg["iterations"] = nltv_iterations(reg)
        if reg["iterations"] < 0:
            raise ValueError(f"_regularisation_['{NLTV_ITERATIONS}'] must not be negative")


_PDHG_METHODS = {"PDHG", "SPDHG"}   # the primal-dual drivers: the same data terms, keys and refusals but for the subsets


def _pdhg_refusals(self, _data_: dict, name: str = "PDHG") -> None:
    """What PDHG and SPDHG (RecToolsIRCuPy.PDHG, .SPDHG; docs/kernels/pdhg.md, spdhg.md) cannot run on, as a ValueError before
    any projector call: an unmatched operator pair (the iteration assumes the exact adjoint), ordered subsets (PDHG only), a
    z-slab, the weighted data terms, the ring and robust keys."""
    if getattr(self, "adjoint", None) != "matched":
        raise ValueError(f"{name} needs the exact adjoint of the forward projector: construct with adjoint=\"matched\"")
    if self.OS_number > 1 and name == "PDHG":
        raise ValueError("There is no ordered-subsets implementation of PDHG, please set OS_number=None")
    if getattr(self, "slab", None) is not None:
        raise ValueError(f"{name} is not available in z-slab mode")
    if _data_["data_fidelity"] not in {"LS", "KL", "L1"}:
        raise ValueError(f"{name} supports the 'LS', 'KL' and 'L1' data fidelities, not {_data_['data_fidelity']!r}")
    for key in ("ringGH_lambda", "huber_threshold", "studentst_threshold"):
        if _data_.get(key) is not None:
            raise ValueError(f"_data_['{key}'] is available in FISTA only ({name}: the 'L1' data fidelity is the robust term)")


def _pdhg_keys(_algorithm_: dict, _regularisation_: dict, name: str = "PDHG") -> None:
    """The keys of PDHG and SPDHG: ``PDHG_ratio`` (sigma / tau, default 1.0, positive), ``PDHG_preconditioner`` (None, the
    default, or "diagonal"; SPDHG takes None only), for SPDHG ``SPDHG_seed`` (the seed
    of the block draws, default 0, a non-negative int), and a regulariser that is None or exactly "PD_TV" -- the same TV
    semi-norm, solved jointly in the dual, so only ``regul_param`` and ``methodTV`` are read (and filled); no prox runs,
    hence no slice-wise or half-precision form.  PDHG alone also takes exactly "PD_TGV", the second-order TGV term in its
    dual: ``regul_param``, ``TGV_alpha1`` (1.0) and ``TGV_alpha2`` (2.0), all positive, and nothing else."""
    _algorithm_.setdefault("PDHG_ratio", 1.0)
    if not float(_algorithm_["PDHG_ratio"]) > 0.0:
        raise ValueError("_algorithm_['PDHG_ratio'] (sigma / tau) must be positive")
    # the diagonal preconditioner (docs/kernels/pdhg.md): PDHG's alone, so SPDHG refuses it instead of ignoring it
    pre = _algorithm_.setdefault("PDHG_preconditioner", None)
    if name == "SPDHG" and pre is not None:
        raise ValueError("_algorithm_['PDHG_preconditioner'] is available in PDHG only: there is no preconditioned SPDHG")
    if pre not in (None, "diagonal"):
        raise ValueError(f"_algorithm_['PDHG_preconditioner'] must be None or 'diagonal', not {pre!r}")
    if name == "SPDHG":
        seed = _algorithm_.setdefault("SPDHG_seed", 0)
        if isinstance(seed, bool) or not isinstance(seed, numbers.Integral) or seed < 0:
            raise ValueError("_algorithm_['SPDHG_seed'] must be a non-negative int")
    method = _regularisation_.get("method")
    if method is None:
        return
    tgv = name == "PDHG" and method == "PD_TGV"
    if method != "PD_TV" and not tgv:
        also = " or 'PD_TGV' (the TGV term in its dual)" if name == "PDHG" else ""
        raise ValueError(f"{name} takes _regularisation_['method'] = None or 'PD_TV' (the TV term in its dual){also}, not {method!r}")
    if _regularisation_.get("slicewise", False) is not False:
        raise ValueError(f"{name} does not support slicewise=True")
    if _regularisation_.get("half_precision", False):
        raise ValueError(f"{name} does not support half_precision=True")
    _regularisation_.setdefault("regul_param", 0.001)
    if tgv:   # lambda min_v (alpha1 |grad x - v| + alpha0 |E v|): the weights of the TGV prox by their names there, nothing else
        _regularisation_.setdefault("TGV_alpha1", 1.0)
        _regularisation_.setdefault("TGV_alpha2", 2.0)
        for key in ("regul_param", "TGV_alpha1", "TGV_alpha2"):
            if not float(_regularisation_[key]) > 0.0:
                raise ValueError(f"_regularisation_['{key}'] must be positive")
        return
    _regularisation_.setdefault("methodTV", 0)
    if not float(_regularisation_["regul_param"]) > 0.0:
        raise ValueError("_regularisation_['regul_param'] must be positive")
    if _regularisation_["methodTV"] not in (0, 1):
        raise ValueError("_regularisation_['methodTV'] must be 0 (isotropic) or 1 (anisotropic)")


def dicts_check(self, _data_: dict, _algorithm_: Optional[dict] = None, _regularisation_: Optional[dict] = None,
                method_run: str = "FISTA") -> tuple:
    """Populate the three dictionaries in place and return them (see module docstring)."""
    # ------------------------------------------------------------------ _data_
    if _data_ is None:
        raise NameError("The data dictionary must be always provided")
    if _data_.get("projection_data") is None:
        raise NameError("'projection_data' needs to be provided")
    device_index = self.Atools.device_index
    data = ops.to_device(_data_["projection_data"], device_index)
    is_2d = data.ndim == 2
    labels = _data_.setdefault("data_axes_labels_order", None)
    if labels is not None:
        data = _data_dims_swapper(data, labels, LABELS_2D if is_2d else LABELS_3D)
        _data_["data_axes_labels_order"] = None  # swapped once; never again
    if is_2d:
        data = data.unsqueeze(0)
    _data_["projection_data"] = ops.contiguous(data)

    if _data_.get("data_fidelity") is None:
        _data_["data_fidelity"] = "LS"
    # "SWLS" (stripe-weighted least squares) and the Group-Huber keys below are the ring-artefact data terms of the
    # reference's removed RecToolsIR class (docs/source/tutorials/real_data_recon.rst:100-151); the reference's current
    # dicts_check knows LS / PWLS / KL only
    # "L1" is PDHG's and SPDHG's alone (docs/kernels/pdhg.md): the other drivers need a differentiable data term
    if _data_["data_fidelity"] not in {"LS", "PWLS", "KL", "SWLS"} and not (
            method_run in _PDHG_METHODS and _data_["data_fidelity"] == "L1"):
        raise ValueError("_data_['data_fidelity'] should be provided as 'LS', 'PWLS', 'KL' (or 'SWLS').")
    if method_run in _PDHG_METHODS:
        _pdhg_refusals(self, _data_, method_run)
    self.data_fidelity = _data_["data_fidelity"]
    _data_.setdefault("ringGH_lambda", None)        # Group-Huber offsets: off unless a threshold is given
    _data_.setdefault("ringGH_accelerate", 50)
    _data_.setdefault("beta_SWLS", 0.1)
    if _data_["ringGH_lambda"] is not None and _data_["data_fidelity"] not in {"LS", "PWLS"}:
        raise ValueError("the Group-Huber ring term (ringGH_lambda) combines with the 'LS' and 'PWLS' data fidelities only")
    if _data_["data_fidelity"] == "SWLS" and method_run != "FISTA":
        raise ValueError("the 'SWLS' data fidelity is available in FISTA only")
    if _data_["ringGH_lambda"] is not None and method_run != "FISTA":
        raise ValueError("the Group-Huber ring term (ringGH_lambda) is available in FISTA only")

    # Huber / Student's-t data terms (outlier-robust re-weighting of the residual): keys of the removed RecToolsIR class as
    # well (Demos/methods_IR_legacy/DemoFISTA_artifacts2D.py:197,263,307,348; docs/source/introduction/about.rst:38)
    _data_.setdefault("huber_threshold", None)
    _data_.setdefault("studentst_threshold", None)
    for key in ("huber_threshold", "studentst_threshold"):
        if _data_[key] is not None:
            if method_run != "FISTA":
                raise ValueError(f"the robust data term ({key}) is available in FISTA only")
            if _data_["data_fidelity"] == "KL":
                raise ValueError(f"the robust data term ({key}) combines with the 'LS', 'PWLS' and 'SWLS' data fidelities only")
            if not float(_data_[key]) > 0.0:
                raise ValueError(f"_data_['{key}'] must be a positive threshold")
    if _data_["huber_threshold"] is not None and _data_["studentst_threshold"] is not None:
        raise ValueError("give either 'huber_threshold' or 'studentst_threshold', not both")
    # the stripe variable of PDHG (docs/kernels/pdhg.md): mu of mu |s|_1, one offset s per detector pixel added to every
    # angle.  Read, never filled: absent means off, and the dictionaries of every other call stay what they were
    stripe = _data_.get("stripe_lambda")
    if stripe is not None:
        if method_run != "PDHG":
            raise ValueError("_data_['stripe_lambda'] is available in PDHG only")
        if not float(stripe) > 0.0:
            raise ValueError("_data_['stripe_lambda'] (the weight mu of the stripe variable's L1 norm) must be positive")

    if self.OS_number > 1 and method_run in _NO_OS_METHODS:
        raise NameError(
            "There is no ordered-subsets implementation for this reconstruction method, please set OS_number=None")

    # ------------------------------------------------------------------ _algorithm_
    if _algorithm_ is None:
        _algorithm_ = {}
    if method_run in _NO_LIPSCHITZ:
        _algorithm_["lipschitz_const"] = 0  # these methods never need it
        if _algorithm_.get("tau_step_lanweber") is None:
            _algorithm_["tau_step_lanweber"] = 1e-05
    if _algorithm_.get("iterations") is None and method_run in _DEFAULT_ITERATIONS:
        classical, os_count = _DEFAULT_ITERATIONS[method_run]
        _algorithm_["iterations"] = os_count if self.OS_number > 1 else classical
    if method_run == "ADMM":
        _algorithm_.setdefault("ADMM_rho_const", 1.0)
        _algorithm_.setdefault("ADMM_relax_par", 1.6)
    for key, value in _ALGORITHM_DEFAULTS:
        _algorithm_.setdefault(key, value)
    if _algorithm_["nonnegativity"] not in [True, False]:
        raise ValueError("_algorithm_['nonnegativity'] should be set to True or False.")
    self.nonneg_regul = 1 if _algorithm_["nonnegativity"] else 0
    # the tolerance keys are honoured here (tomobar_amd/convergence.py; the reference accepts and ignores them)
    check_tolerance(_algorithm_["tolerance"], "_algorithm_['tolerance']")

    # ------------------------------------------------------------------ _regularisation_
    if _regularisation_ is None:
        _regularisation_ = {}
    if not _regularisation_:
        _regularisation_["method"] = None
    if method_run in _PDHG_METHODS:   # before the prox methods' own checks: nothing but None / "PD_TV" gets that far
        _pdhg_keys(_algorithm_, _regularisation_, method_run)
    nltv_check(_regularisation_)
    if is_nltv(_regularisation_.get("method")):   # before the defaults: "iterations" must still be the caller's own
        _nltv_keys(self, _regularisation_)
    if method_run in {"FISTA", "ADMM", "OSEM"}:
        for key, value in _REGULARISATION_DEFAULTS:
            _regularisation_.setdefault(key, value)
    check_tolerance(_regularisation_.get("tolerance"), "_regularisation_['tolerance']")
    slicewise_of(_regularisation_)   # checked where present (a bool), never filled: absent means False
    # the keys of the method prox_regul will run (supp/regularisers.py: TGV, NDF, Diff4th and LLT_ROF add some, none of them
    # implemented in this reference version).  Dictionaries of the other methods are not touched.
    kind = kind_of(_regularisation_.get("method"))
    extra_keys = kind.defaults if kind is not None else ()
    if has_wavelets(_regularisation_.get("method")):   # the suffix: the threshold of the wavelet shrinkage
        extra_keys += tuple(k for k in WAVELETS_DEFAULTS if k not in extra_keys)
    for key, value, _ in extra_keys:
        _regularisation_.setdefault(key, value)
    for key, _, choices in extra_keys:
        if choices is not None:
            if _regularisation_[key] not in choices:
                named = ", ".join(repr(c) for c in choices[:-1]) + " or " + repr(choices[-1])
                raise ValueError(f"_regularisation_['{key}'] must be {named}")
        elif not float(_regularisation_[key]) > 0.0:
            raise ValueError(f"_regularisation_['{key}'] must be positive")
    return (_data_, _algorithm_, _regularisation_)
