"""The regularisers ``_regularisation_["method"]`` can name, in the order ``prox_regul`` dispatches in, and what follows
from the choice: which function runs it, which scratch arena and placed slot it takes, which dictionary keys it adds.
This is the one place the precedence is written: ``regularisersCuPy.prox_regul`` / ``check_prox_available`` /
``reserve_prox_scratch``, ``dicts.dicts_check``, ``ops.reserve_tv_scratch``, the march drivers of ``slab`` and the package's
lazy names all read it.  No reference counterpart (its ``prox_regul`` is a two-branch if, regularisersCuPy.py:16-38).

Next to the table stands the one suffix a method string can carry, ``WAVELETS`` (``has_wavelets``): not a kind but a modifier
of every kind except LLT_ROF -- the prox is averaged with a db5 wavelet shrinkage whose threshold is ``regul_param2``
(docs/kernels/wavelets.md).  The same call sites read it.

Imports neither torch nor ``ops``.  Functions are held by NAME and looked up on their module when they are called:
the CPU tests stand the oracle in for them by setting module attributes.
"""

from __future__ import annotations

from typing import NamedTuple, Optional

# the keys beyond the reference's, with the value an absent key stands for
_DEFAULT = {"TGV_alpha1": 1.0, "TGV_alpha2": 2.0, "NDF_penalty": "Huber", "edge_threshold": 0.01, "regul_param2": 0.001}


def _opt(reg, key):
    return reg.get(key, _DEFAULT[key])


def _keys(*checked):
    """``defaults`` of a record: (key, default, choices) in the order dicts_check fills and then checks them; ``choices`` None
    = the value must be positive, else the values it may take."""
    return tuple((key, _DEFAULT[key], choices) for key, choices in checked)


class Kind(NamedTuple):
    name: str              # the substring of _regularisation_["method"]
    cupy: str              # the whole-volume function in regularisersCuPy
    slab: Optional[str]    # the z-slab driver in slab (None: not available in z-slab mode)
    scratch: str           # the C symbol that sizes the scratch arena ...
    scratch_half: bool     # ... and whether it takes `half` after (dx, dy, dz, nd)
    half: bool             # half_precision=True is accepted, and passed on as the last positional argument
    slot: Optional[int]    # the placed block of the slab driver (ops.placed_empty): one per operator, so that solvers of
    #                        different operators on one stream never alias
    ghost: Optional[int]   # ghost planes of U per interior boundary of a MarchSlab (PdSlab / RofSlab: asymmetric, their own)
    entry: Optional[str]   # the C entry point of one MarchSlab iteration
    defaults: tuple        # see _keys
    args: object           # args(reg, self): the positional arguments after the array (slab driver: after the communicator);
    #                        the *_cupy call appends the device index, both append half_precision where `half`


KINDS = (
    Kind("ROF_TV", "ROF_TV_cupy", "rof_tv_slab", "tomo_roftv_scratch_bytes", False, True, 1, None, None, (),
         lambda reg, self: (reg["regul_param"], reg["iterations"], reg["time_marching_step"])),
    Kind("PD_TV", "PD_TV_cupy", "pd_tv_slab", "tomo_pdtv_scratch_bytes", True, True, 0, None, None, (),
         lambda reg, self: (reg["regul_param"], reg["iterations"], reg["methodTV"], self.nonneg_regul,
                            reg["PD_LipschitzConstant"])),
    # TGV_alpha2 is the weight of the second-order term, alpha0 in docs/kernels/tgv.md (the key names are those of the
    # reference's removed RecToolsIR class); the halo protocol for its 13 further fields does not exist
    Kind("TGV", "TGV_cupy", None, "tomo_tgv_scratch_bytes", False, False, None, None, None,
         _keys(("TGV_alpha1", None), ("TGV_alpha2", None)),
         lambda reg, self: (reg["regul_param"], reg["iterations"], _opt(reg, "TGV_alpha1"), _opt(reg, "TGV_alpha2"),
                            reg["PD_LipschitzConstant"])),
    # NDF, Diff4th, LLT_ROF: named by the reference's comment on time_marching_step (tomobar/supp/dicts.py:173), implemented
    # nowhere in its tree (docs/kernels/ndf.md, diff4th.md, llt_rof.md)
    Kind("NDF", "NDF_cupy", "ndf_slab", "tomo_ndf_scratch_bytes", False, False, 2, 1, "tomo_ndf_iter_slab_range",
         _keys(("NDF_penalty", ("Huber", "PM", "Tukey")), ("edge_threshold", None)),
         lambda reg, self: (reg["regul_param"], _opt(reg, "edge_threshold"), reg["iterations"], reg["time_marching_step"],
                            _opt(reg, "NDF_penalty"))),
    # ghost 2 = the stencil's radius: W at distance 1 needs U at distance 2
    Kind("Diff4th", "Diff4th_cupy", "diff4th_slab", "tomo_diff4th_scratch_bytes", False, False, 3, 2,
         "tomo_diff4th_iter_slab_range", _keys(("edge_threshold", None)),
         lambda reg, self: (reg["regul_param"], _opt(reg, "edge_threshold"), reg["iterations"], reg["time_marching_step"])),
    # regul_param is the ROF weight, regul_param2 the LLT weight (keys of the removed RecToolsIR class); ghost 2 = the
    # stencil's radius: E_d at distance 1 needs U at distance 2
    Kind("LLT_ROF", "LLT_ROF_cupy", "llt_rof_slab", "tomo_llt_rof_scratch_bytes", False, False, 4, 2,
         "tomo_llt_rof_iter_slab_range", _keys(("regul_param2", None)),
         lambda reg, self: (reg["regul_param"], _opt(reg, "regul_param2"), reg["iterations"], reg["time_marching_step"])),
)
BY_NAME = {k.name: k for k in KINDS}


def kind_of(method) -> Optional[Kind]:
    """The record ``method`` means: the first of KINDS whose name is a substring of it; None for None, for anything that is
    not a string and for a string that names none."""
    if not isinstance(method, str):
        return None
    return next((k for k in KINDS if k.name in method), None)


# ---- the suffix: "<kind>_WAVELETS" averages the kind's prox with the wavelet shrinkage W_t, t = regul_param2 (the key and
# its default 0.001 are those of the removed RecToolsIR class; the reference's tutorials still write "PD_TV_WAVELETS")
WAVELETS = "WAVELETS"
WAVELETS_CUPY = "WAVELETS_cupy"                    # the stand-alone function in regularisersCuPy
WAVELETS_SCRATCH = "tomo_wavelet_scratch_bytes"    # the C symbol that sizes the coefficient pyramid
WAVELETS_DEFAULTS = _keys(("regul_param2", None))  # what dicts_check fills and checks for it, as `defaults` of a record
WAVELETS_REFUSED = ("LLT_ROF",)                    # regul_param2 is already that kind's LLT weight


def has_wavelets(method) -> bool:
    """``method`` names a kind and carries the suffix (a string with ``WAVELETS`` that names no kind is an unknown method)."""
    return isinstance(method, str) and WAVELETS in method and kind_of(method) is not None


def wavelet_threshold(reg):
    return _opt(reg, "regul_param2")


# ---- NLTV stands beside the table as well: non-local TV over neighbour tables the caller builds beforehand with
# ``PatchSelect_cupy`` (docs/kernels/nltv.md).  The keys are those of the reference's legacy demo
# (Demos/methods_IR_legacy/DemoFISTA_NLTV_2D.py), which notes that "NLTV method is quite different to the generic structure
# of other regularisers": no record of KINDS fits it (three arrays among its arguments, per slice by definition, no z-slab
# driver and no placed slot).  The call sites branch on ``is_nltv`` before ``kind_of``.
NLTV = "NLTV"
NLTV_CUPY = "NLTV_cupy"                            # the whole-volume function in regularisersCuPy (a slab rank runs it too)
NLTV_SELECT_CUPY = "PatchSelect_cupy"              # what builds the tables
NLTV_TABLES = ("NLTV_H_i", "NLTV_H_j", "NLTV_Weights")   # required keys: (K, *volume) arrays, uint16 / uint16 / float32
NLTV_NEIGHBOURS = "NumNeighb"                      # optional: must equal the tables' first extent
NLTV_ITERATIONS = "IterNumb"                       # the demo's key for the iteration count; absent: "iterations"


def is_nltv(method) -> bool:
    """``method`` is a string that contains ``NLTV`` and names no kind (one that names both is refused: ``nltv_check``)."""
    return isinstance(method, str) and NLTV in method and kind_of(method) is None


def nltv_check(reg) -> None:
    """The method strings and keys NLTV refuses, as a ValueError: a string that names a kind as well, the ``WAVELETS``
    suffix, ``half_precision=True``.  Nothing to do for any other method."""
    method = reg.get("method")
    if not isinstance(method, str) or NLTV not in method:
        return
    kind = kind_of(method)
    if kind is not None:
        raise ValueError(f"the regularisation method {method!r} names both {kind.name} and NLTV")
    if WAVELETS in method:
        raise ValueError("NLTV does not combine with WAVELETS")
    if reg.get("half_precision", False):
        raise ValueError("NLTV does not support half_precision=True")


def nltv_tables(reg) -> tuple:
    """The three tables of ``reg`` in the order ``NLTV_cupy`` takes them.  A missing one is a ValueError that names the key --
    and the methods that run without tables, which is what a caller who wrote "NLTV" without building any needs to know."""
    for key in NLTV_TABLES:
        if reg.get(key) is None:
            raise ValueError(f"_regularisation_['{key}'] is required by the NLTV method: it takes the tables {NLTV_SELECT_CUPY} "
                             f"returns as {', '.join(NLTV_TABLES)}; without tables ROF_TV, PD_TV and TGV are supported, as are "
                             "NDF, Diff4th and LLT_ROF")
    return tuple(reg[key] for key in NLTV_TABLES)


def nltv_iterations(reg) -> int:
    """``IterNumb`` where present, else ``iterations``; both present and different is a ValueError."""
    if reg.get(NLTV_ITERATIONS) is None:
        return reg["iterations"]
    if reg.get("iterations") is not None and int(reg["iterations"]) != int(reg[NLTV_ITERATIONS]):
        raise ValueError(f"_regularisation_['{NLTV_ITERATIONS}'] = {reg[NLTV_ITERATIONS]} and _regularisation_['iterations'] = "
                         f"{reg['iterations']} differ: give one of them")
    return int(reg[NLTV_ITERATIONS])


# ---- the key "slicewise": True runs the 2D form of the kind on every (y, x) slice of a 3D volume instead of coupling the
# slices along z (docs/kernels/slicewise.md).  Absent = False; dicts_check does not fill it.
SLICEWISE = "slicewise"
SLICEWISE_KINDS = ("ROF_TV", "PD_TV")              # the kinds that have a slice-wise form; the others refuse the key


def slicewise_of(reg) -> bool:
    """The value of ``reg["slicewise"]`` (absent: False); anything but a bool is a ValueError."""
    value = reg.get(SLICEWISE, False)
    if not isinstance(value, bool):
        raise ValueError(f"_regularisation_['{SLICEWISE}'] must be True or False, got {value!r}")
    return value
