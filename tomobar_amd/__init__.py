"""tomobar_amd -- MI355X (gfx950) engine for ToMoBAR's ordered-subsets FISTA / ADMM hot path.

Drop-in surface (same names and argument meaning as the reference package ``tomobar``):

    from tomobar_amd.methodsIR_CuPy import RecToolsIRCuPy      # FISTA / ADMM / OSEM / SIRT / CGLS / Landweber
    from tomobar_amd.methodsDIR_CuPy import RecToolsDIRCuPy    # FORWPROJ / BACKPROJ / FBP
    from tomobar_amd.regularisersCuPy import PD_TV_cupy, ROF_TV_cupy, TGV_cupy, NDF_cupy, Diff4th_cupy, LLT_ROF_cupy, WAVELETS_cupy
    from tomobar_amd.regularisersCuPy import PatchSelect_cupy, NLTV_cupy                           # non-local TV and its tables

Arrays are float32 ``torch.Tensor`` on the GPU.  All arithmetic runs in hand-written HIP kernels of
``libtomo_mi355x.so`` (C-ABI: ``include/tomo_mi355x.h``); importing this package never builds or falls back to
anything: without the library or without a GPU the operators raise.
"""

__version__ = "0.1.0"

from . import _lib  # noqa: F401
from .supp.regularisers import KINDS as _KINDS, NLTV_CUPY as _NLTV_CUPY, NLTV_SELECT_CUPY as _NLTV_SELECT_CUPY, WAVELETS_CUPY as _WAVELETS_CUPY


def library_path() -> str:
    return _lib.LIB_PATH


def __getattr__(name):
    # `from tomobar_amd import NDF_cupy` (any *_cupy of supp/regularisers.py: WAVELETS_cupy, NLTV_cupy and
    # PatchSelect_cupy included) without importing torch at package import
    if name in (_WAVELETS_CUPY, _NLTV_CUPY, _NLTV_SELECT_CUPY) or any(name == k.cupy for k in _KINDS):
        from . import regularisersCuPy
        return getattr(regularisersCuPy, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
