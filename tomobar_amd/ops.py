"""Tensor-level wrappers over the C-ABI: device memory and streams come from torch (plumbing only),
every arithmetic operation is a HIP kernel in ``libtomo_mi355x.so``.

Arrays are ``torch.Tensor`` (float32, device ``cuda:<index>``) where the reference uses ``cupy.ndarray``.
"""

from __future__ import annotations

import contextlib
import ctypes as C
import threading

import numpy as np
import torch

from . import _lib as L
from .supp.regularisers import BY_NAME, SLICEWISE_KINDS


def _require_gpu(device_index: int) -> torch.device:
    if not torch.cuda.is_available():
        raise L.TomoRuntimeError(
            "no ROCm device is visible to torch: tomobar_amd runs on MI355X (gfx950) only and has no CPU fallback")
    return torch.device("cuda", int(device_index))


def to_device(x, device_index: int = 0) -> torch.Tensor:
    """numpy / torch / cupy (DLPack or __cuda_array_interface__) object -> float32-preserving device tensor (no dtype
    change, no copy for arrays that already live on the device)."""
    dev = _require_gpu(device_index)
    if isinstance(x, torch.Tensor):
        return x.to(dev)
    if isinstance(x, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    if is_cupy(x) and hasattr(x, "__dlpack__"):
        return torch.from_dlpack(x).to(dev)
    return torch.as_tensor(x, device=dev)


def is_cupy(x) -> bool:
    return type(x).__module__.split(".")[0] == "cupy"


def base_ptr(x):
    """Device address of a torch / cupy array (None for anything else): used to detect zero-copy views of caller memory."""
    if isinstance(x, torch.Tensor):
        return x.data_ptr()
    if is_cupy(x):
        return int(x.data.ptr)
    return None


def like(result, given):
    """`result` (a device tensor) in the array library the caller used for `given`: the reference's classes return
    ``cupy.ndarray`` (methodsIR_CuPy.py:484), so a caller that hands CuPy arrays in gets CuPy arrays back (zero-copy through
    DLPack) wherever CuPy-on-ROCm is installed; every other caller gets the ``torch.Tensor``.  CuPy is never required."""
    if isinstance(result, torch.Tensor) and is_cupy(given):
        import cupy
        return cupy.from_dlpack(result)
    return result


def stream_ptr(t: torch.Tensor):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _on(t: torch.Tensor):
    """Context making the tensor's device current for a launch (the launch stream belongs to that device)."""
    return torch.cuda.device(t.device)


def ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _chk_f32(t: torch.Tensor, name="array"):
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be C-contiguous")
    if not t.is_cuda:
        raise ValueError(f"{name} must live on the GPU")


def contiguous(t: torch.Tensor) -> torch.Tensor:
    """Materialise a (possibly permuted) <=3-D float32 view as a C-contiguous tensor with tomo_permute3."""
    if t.is_contiguous():
        return t
    if t.dtype != torch.float32 or t.dim() > 3:
        raise ValueError("only float32 arrays of at most 3 dimensions are supported")
    shape = list(t.shape)
    strides = list(t.stride())
    while len(shape) < 3:
        shape.insert(0, 1)
        strides.insert(0, 0)
    out = torch.empty(t.shape, dtype=torch.float32, device=t.device)
    with torch.cuda.device(t.device):
        L.check(L.lib().tomo_permute3(ptr(t), ptr(out), shape[0], shape[1], shape[2],
                                      strides[0], strides[1], strides[2], stream_ptr(t)))
    return out


# ----------------------------------------------------------------------------- element-wise / reductions
def momentum(x, x_old, x_t, beta):
    with _on(x):
        L.check(L.lib().tomo_momentum(ptr(x), ptr(x_old), ptr(x_t), float(beta), x.numel(), stream_ptr(x)))


def admm_dual(u, z, x):
    with _on(u):
        L.check(L.lib().tomo_admm_dual(ptr(u), ptr(z), ptr(x), u.numel(), stream_ptr(u)))


def axpby(a, x, b, y):
    with _on(y):
        L.check(L.lib().tomo_axpby(float(a), ptr(x), float(b), ptr(y), y.numel(), stream_ptr(y)))


def scale(a, x, y):
    with _on(y):
        L.check(L.lib().tomo_scale(float(a), ptr(x), ptr(y), y.numel(), stream_ptr(y)))


def clamp_min(x, lo=0.0):
    with _on(x):
        L.check(L.lib().tomo_clamp_min(ptr(x), float(lo), x.numel(), stream_ptr(x)))


def mul(x, y):
    with _on(y):
        L.check(L.lib().tomo_mul(ptr(x), ptr(y), y.numel(), stream_ptr(y)))


def recip_safe(x, y):
    with _on(y):
        L.check(L.lib().tomo_recip_safe(ptr(x), ptr(y), y.numel(), stream_ptr(y)))


def fill(x, value):
    with _on(x):
        L.check(L.lib().tomo_fill(ptr(x), float(value), x.numel(), stream_ptr(x)))


def norm2(x) -> float:
    out = C.c_double(0.0)
    with torch.cuda.device(x.device):
        L.check(L.lib().tomo_norm2(ptr(x), x.numel(), C.byref(out), stream_ptr(x)))
    return out.value


def dot(x, y) -> float:
    out = C.c_double(0.0)
    with torch.cuda.device(x.device):
        L.check(L.lib().tomo_dot(ptr(x), ptr(y), x.numel(), C.byref(out), stream_ptr(x)))
    return out.value


def rel_change(x, ref, keep=None):
    """(num, den) = (sum (x - ref)^2, sum x^2) in float64 from the float32 values, one streaming pass (tomo_rel_change);
    with `keep` (a float32 array of the same size; may be `ref` itself) the pass also writes ``keep[...] = x``.  The
    relative change the tolerance keys are compared with is ``convergence.relative_change(num, den)``.  Synchronises the
    stream."""
    for name, t in (("x", x), ("ref", ref), ("keep", keep)):
        if t is not None:
            _chk_f32(t, name)
            if t.numel() != x.numel():
                raise ValueError(f"{name} must have as many elements as x")
    out = (C.c_double * 2)()
    with torch.cuda.device(x.device):
        L.check(L.lib().tomo_rel_change(ptr(x), ptr(ref), ptr(keep), x.numel(), out, stream_ptr(x)))
    return float(out[0]), float(out[1])


def pwls_weights(b, slab=None):
    """w = max(b, 1e-6) / max(max(b, 1e-6)); with a SlabComm the maximum is taken over all z-slabs."""
    w = torch.empty_like(b)
    with torch.cuda.device(b.device):
        if slab is None:
            L.check(L.lib().tomo_pwls_weights(ptr(b), ptr(w), b.numel(), stream_ptr(b)))
        else:
            m = C.c_float(0.0)
            L.check(L.lib().tomo_pwls_max(ptr(b), b.numel(), C.byref(m), stream_ptr(b)))
            wmax = np.float32(slab.allreduce_max(float(m.value)))
            L.check(L.lib().tomo_pwls_weights_scaled(ptr(b), ptr(w), b.numel(), float(wmax), stream_ptr(b)))
    return w


# ----------------------------------------------------------------------------- pre / post
def pad_edge(b, pad):
    nz, na, nu0 = b.shape
    out = torch.empty((nz, na, nu0 + 2 * pad), dtype=torch.float32, device=b.device)
    with _on(b):
        L.check(L.lib().tomo_pad_edge(ptr(b), ptr(out), nz * na, nu0, pad, stream_ptr(b)))
    return out


def crop_center(vol, m):
    nz, n, _ = vol.shape
    out = torch.empty((nz, m, m), dtype=torch.float32, device=vol.device)
    with _on(vol):
        L.check(L.lib().tomo_crop_center(ptr(vol), ptr(out), nz, n, m, stream_ptr(vol)))
    return out


def circ_mask_(vol, radius):
    nz, n, _ = vol.shape
    with _on(vol):
        L.check(L.lib().tomo_circ_mask(ptr(vol), nz, n, float(radius), stream_ptr(vol)))
    return vol


# ----------------------------------------------------------------------------- TV
def _tv_dims(t):
    if t.dim() == 2:
        return t.shape[1], t.shape[0], 1, 2
    return t.shape[2], t.shape[1], t.shape[0], 3


def pdtv(data, out, sigma, tau, lt, theta, iterations, methodTV, nonneg, half):
    dx, dy, dz, nd = _tv_dims(data)
    with torch.cuda.device(data.device):
        L.check(L.lib().tomo_pdtv(data.device.index, ptr(data), ptr(out), dx, dy, dz, nd, float(sigma), float(tau),
                                  float(lt), float(theta), int(iterations), int(bool(methodTV)), int(bool(nonneg)),
                                  int(bool(half)), stream_ptr(data)))
    return out


def roftv(data, out, lam, tau, iterations, half):
    dx, dy, dz, nd = _tv_dims(data)
    with torch.cuda.device(data.device):
        L.check(L.lib().tomo_roftv(data.device.index, ptr(data), ptr(out), dx, dy, dz, nd, float(lam), float(tau),
                                   int(iterations), int(bool(half)), stream_ptr(data)))
    return out


def pdtv_tol(data, out, sigma, tau, lt, theta, iterations, methodTV, nonneg, half, tolerance):
    """`pdtv` with the stopping rule of tomo_pdtv_tol: returns (out, iterations_done, rel_change) -- the last relative
    change evaluated, NaN if no check took place."""
    dx, dy, dz, nd = _tv_dims(data)
    done, last = C.c_int(0), C.c_double(float("nan"))
    with torch.cuda.device(data.device):
        L.check(L.lib().tomo_pdtv_tol(data.device.index, ptr(data), ptr(out), dx, dy, dz, nd, float(sigma), float(tau),
                                      float(lt), float(theta), int(iterations), int(bool(methodTV)), int(bool(nonneg)),
                                      int(bool(half)), float(tolerance), C.byref(done), C.byref(last), stream_ptr(data)))
    return out, int(done.value), float(last.value)


def roftv_tol(data, out, lam, tau, iterations, half, tolerance):
    """`roftv` with the stopping rule of tomo_roftv_tol: returns (out, iterations_done, rel_change)."""
    dx, dy, dz, nd = _tv_dims(data)
    done, last = C.c_int(0), C.c_double(float("nan"))
    with torch.cuda.device(data.device):
        L.check(L.lib().tomo_roftv_tol(data.device.index, ptr(data), ptr(out), dx, dy, dz, nd, float(lam), float(tau),
                                       int(iterations), int(bool(half)), float(tolerance), C.byref(done), C.byref(last),
                                       stream_ptr(data)))
    return out, int(done.value), float(last.value)


def _slices_dims(data, out):
    for name, t in (("data", data), ("out", out)):
        _chk_f32(t, name)
    if data.dim() != 3:
        raise ValueError("a stack of slices [nslices, dy, dx] must be provided")
    if tuple(out.shape) != tuple(data.shape) or out.device != data.device:
        raise ValueError("out must have the shape and the device of the data")
    return data.shape[2], data.shape[1], data.shape[0]


def pdtv_slices(data, out, sigma, tau, lt, theta, iterations, methodTV, nonneg, half, tolerance=0.0):
    """Slice-wise PD_TV (tomo_pdtv_slices; docs/kernels/slicewise.md): every slice ``data[k]`` of a 3D array receives what
    `pdtv` returns for it as a 2D image, all slices in one set of launches.  Returns (out, iterations_done, rel_change): one
    stopping decision over the whole array (tolerance 0 = off: all iterations, NaN)."""
    dx, dy, ns = _slices_dims(data, out)
    done, last = C.c_int(0), C.c_double(float("nan"))
    with torch.cuda.device(data.device):
        L.check(L.lib().tomo_pdtv_slices(data.device.index, ptr(data), ptr(out), dx, dy, ns, float(sigma), float(tau),
                                         float(lt), float(theta), int(iterations), int(bool(methodTV)), int(bool(nonneg)),
                                         int(bool(half)), float(tolerance), C.byref(done), C.byref(last), stream_ptr(data)))
    return out, int(done.value), float(last.value)


def roftv_slices(data, out, lam, tau, iterations, half, tolerance=0.0):
    """Slice-wise ROF_TV (tomo_roftv_slices): as `pdtv_slices`; `out` must be another array than `data` (the iterations
    ping-pong through it)."""
    dx, dy, ns = _slices_dims(data, out)
    done, last = C.c_int(0), C.c_double(float("nan"))
    with torch.cuda.device(data.device):
        L.check(L.lib().tomo_roftv_slices(data.device.index, ptr(data), ptr(out), dx, dy, ns, float(lam), float(tau),
                                          int(iterations), int(bool(half)), float(tolerance), C.byref(done), C.byref(last),
                                          stream_ptr(data)))
    return out, int(done.value), float(last.value)


def _marched(entry, data, out, scalars, iterations, tolerance, ints=()):
    """The call behind tgv / ndf / diff4th / llt_rof: `entry` is the C entry point, `scalars` its float parameters and `ints`
    the integer ones that follow them.  Returns (out, iterations_done, rel_change)."""
    dx, dy, dz, nd = _tv_dims(data)
    done, last = C.c_int(0), C.c_double(float("nan"))
    with torch.cuda.device(data.device):
        L.check(getattr(L.lib(), entry)(data.device.index, ptr(data), ptr(out), dx, dy, dz, nd, *map(float, scalars),
                                        *map(int, ints), int(iterations), float(tolerance), C.byref(done), C.byref(last),
                                        stream_ptr(data)))
    return out, int(done.value), float(last.value)


def tgv(data, out, lam, alpha1, alpha0, tau, sigma, iterations, tolerance=0.0):
    """Second-order TGV prox (tomo_tgv; the algorithm: docs/kernels/tgv.md): `iterations` Chambolle-Pock iterations of
    `data` into `out` (a different array: U is iterated there).  Returns (out, iterations_done, rel_change) -- the last
    relative change the stopping rule evaluated, NaN if none (tolerance 0 = off)."""
    return _marched("tomo_tgv", data, out, (lam, alpha1, alpha0, tau, sigma), iterations, tolerance)


def ndf(data, out, lam, sigma, tau, penalty, iterations, tolerance=0.0):
    """Nonlinear diffusion (tomo_ndf; the algorithm: docs/kernels/ndf.md): `iterations` explicit time-marching steps of
    `data` into `out` (a different array: the iterations ping-pong through it; `data` is never written).  `penalty` is
    "Huber", "PM" or "Tukey"; `lam`, `sigma` (the edge threshold) and `tau` are float32 scalars.  Returns (out,
    iterations_done, rel_change) -- the last relative change the stopping rule evaluated, NaN if none (tolerance 0 = off)."""
    return _marched("tomo_ndf", data, out, (lam, sigma, tau), iterations, tolerance, ints=(L.ndf_penalty_id(penalty),))


def diff4th(data, out, lam, sigma, tau, iterations, tolerance=0.0):
    """Anisotropic fourth-order diffusion (tomo_diff4th; the algorithm: docs/kernels/diff4th.md): `iterations` explicit
    time-marching steps of `data` into `out` (a different array: the iterations ping-pong through it; `data` is never
    written).  `lam`, `sigma` (the edge threshold) and `tau` are float32 scalars.  Returns (out, iterations_done,
    rel_change) -- the last relative change the stopping rule evaluated, NaN if none (tolerance 0 = off)."""
    return _marched("tomo_diff4th", data, out, (lam, sigma, tau), iterations, tolerance)


def llt_rof(data, out, lam_rof, lam_llt, tau, iterations, tolerance=0.0):
    """ROF plus fourth-order LLT diffusion (tomo_llt_rof; the algorithm: docs/kernels/llt_rof.md): `iterations` explicit
    time-marching steps of `data` into `out` (a different array: the iterations ping-pong through it; `data` is never
    written).  `lam_rof`, `lam_llt` (the weights of the two terms) and `tau` are float32 scalars.  Returns (out,
    iterations_done, rel_change) -- the last relative change the stopping rule evaluated, NaN if none (tolerance 0 = off)."""
    return _marched("tomo_llt_rof", data, out, (lam_rof, lam_llt, tau), iterations, tolerance)


# ----------------------------------------------------------------------------- PDHG (docs/kernels/pdhg.md)
PDHG_SLOT = 5   # the placed block of the PDHG driver's work arrays (slots 0-4: the slab drivers, supp/regularisers.py)


def pdhg_work_arrays(shape, device, tv: bool = True, tau: bool = False):
    """The work arrays of one PDHG call on a volume of `shape` ([nz, ny, nx]), uninitialised, from the placed block of
    ``PDHG_SLOT``: (x-bar, g, [q_1 .. q_nd]) and the lease token of ``placed_empty``; nd = 3 if nz > 1 else 2, no q without
    the TV block.  With it the block has the size ``tomo_pdhg_scratch_bytes`` states.  `tau` (the diagonal preconditioner):
    one more array behind the others, the steps per voxel, returned in front of the lease -- (x-bar, g, [q], tau, lease);
    with TV the block then has the size ``tomo_pdhg_diag_scratch_bytes`` states."""
    nd = 3 if shape[0] > 1 else 2
    count = 2 + (nd if tv else 0)
    arrays, lease = placed_empty([(tuple(shape), torch.float32)] * (count + bool(tau)), device, slot=PDHG_SLOT)
    if tau:
        return arrays[0], arrays[1], arrays[2:count], arrays[count], lease
    return arrays[0], arrays[1], arrays[2:], lease


# What the PDHG and SPDHG wrappers check before a launch.  Aliasing and the ranges of the scalars are the library's to refuse.
def _pdhg_flat(named):
    """the element-wise launches: the (name, array) pairs are float32, contiguous, of the size and the device of the first"""
    first = named[0][1]
    for name, t in named:
        _chk_f32(t, name)
        if t.numel() != first.numel() or t.device != first.device:
            raise ValueError(f"{name} must have the size and the device of {named[0][0]}")


def _pdhg_like(x, named):
    for name, t in named:
        _chk_f32(t, name)
        if tuple(t.shape) != tuple(x.shape) or t.device != x.device:
            raise ValueError(f"{name} must have the shape and the device of the volume")


def _pdhg_fields(x, groups, or_none=False):
    """(dx, dy, dz, nd) of a volume `x` [nz, ny, nx]: nd = 3 if nz > 1 else 2 (a dimension of 1 elsewhere stays 3D); every
    (name, arrays) of `groups` holds nd fields like `x` (`or_none`: or is empty)"""
    _chk_f32(x, "volume")
    if x.dim() != 3:
        raise ValueError("PDHG volumes are [nz, ny, nx] arrays")
    dx, dy, dz, nd = x.shape[2], x.shape[1], x.shape[0], 3 if x.shape[0] > 1 else 2
    for name, group in groups:
        if len(group) != nd and not (or_none and len(group) == 0):
            raise ValueError(f"a volume of {dz} plane{'s' if dz > 1 else ''} takes {nd} dual fields"
                             f"{' or none' if or_none else ''}, got {len(group)} for {name}")
        _pdhg_like(x, [(f"{name}{d + 1}", t) for d, t in enumerate(group)])
    return dx, dy, dz, nd


def _pdhg_ptrs(group):
    return [ptr(t) for t in group] + [ptr(None)] * (3 - len(group))


def pdhg_sino_dual(y, r, b, fidelity: str, sigma):
    """Step 2 of a PDHG iteration (tomo_pdhg_sino_dual): the sinogram dual `y` <- the prox of the conjugate of the data term
    `fidelity` ("LS", "L1" or "KL") at y + sigma r, in place; `r` = A x-bar, `b` = the data, `sigma` a float32 scalar."""
    if fidelity not in L.PDHG_FID:
        raise ValueError(f"unknown PDHG data term {fidelity!r}: LS, L1 and KL are supported")
    _pdhg_flat([("y", y), ("r", r), ("b", b)])
    with _on(y):
        L.check(L.lib().tomo_pdhg_sino_dual(ptr(y), ptr(r), ptr(b), y.numel(), L.PDHG_FID[fidelity], float(sigma), stream_ptr(y)))
    return y


def pdhg_tv_dual(xbar, q, sigma, lam, methodTV=0):
    """Step 4 of a PDHG iteration (tomo_pdhg_tv_dual): q_d <- q_d + sigma F_d(x-bar), projected (methodTV 0: onto the ball of
    radius `lam`, 1: onto the box), in place; `q` holds nd fields like `xbar`."""
    dx, dy, dz, nd = _pdhg_fields(xbar, [("q", q)])
    with _on(xbar):
        L.check(L.lib().tomo_pdhg_tv_dual(xbar.device.index, ptr(xbar), *_pdhg_ptrs(q), dx, dy, dz, nd, float(sigma), float(lam),
                                          int(methodTV), stream_ptr(xbar)))


def pdhg_primal(x, xbar, g, q, tau, nonneg=False):
    """Step 5 of a PDHG iteration (tomo_pdhg_primal): x' = x - tau (g - div q), clamped at 0 with `nonneg`; x-bar <- 2 x' - x,
    x <- x', in place.  `q`: the nd dual fields, or an empty sequence for no TV block (div q = 0)."""
    dx, dy, dz, nd = _pdhg_fields(x, [("q", q)], or_none=True)
    _pdhg_like(x, [("xbar", xbar), ("g", g)])
    with _on(x):
        L.check(L.lib().tomo_pdhg_primal(x.device.index, ptr(x), ptr(xbar), ptr(g), *_pdhg_ptrs(q), dx, dy, dz, nd, float(tau),
                                         int(bool(nonneg)), stream_ptr(x)))


def pdhg_diag_steps(out, sums, numer, add=0.0):
    """The steps of PDHG's diagonal preconditioner (tomo_pdhg_diag_steps): `out` <- numer / max(sums + add, 2^-10),
    element-wise; `sums` = A 1 (the steps sigma_i, add = 0) or A^T 1 (the steps tau_j, add = 2 nd with TV); `numer`, `add`
    float32 scalars.  `out` may be `sums` itself.  Returns `out`."""
    _pdhg_flat([("out", out), ("sums", sums)])
    with _on(out):
        L.check(L.lib().tomo_pdhg_diag_steps(ptr(out), ptr(sums), out.numel(), float(numer), float(add), stream_ptr(out)))
    return out


def pdhg_sino_dual_diag(y, r, b, sigma, fidelity: str):
    """`pdhg_sino_dual` with a step per sample (tomo_pdhg_sino_dual_diag): `sigma` is an array like `y`."""
    if fidelity not in L.PDHG_FID:
        raise ValueError(f"unknown PDHG data term {fidelity!r}: LS, L1 and KL are supported")
    _pdhg_flat([("y", y), ("r", r), ("b", b), ("sigma", sigma)])
    with _on(y):
        L.check(L.lib().tomo_pdhg_sino_dual_diag(ptr(y), ptr(r), ptr(b), ptr(sigma), y.numel(), L.PDHG_FID[fidelity], stream_ptr(y)))
    return y


def pdhg_primal_diag(x, xbar, g, q, tau, nonneg=False):
    """`pdhg_primal` with a step per voxel (tomo_pdhg_primal_diag): `tau` is an array like `x`."""
    dx, dy, dz, nd = _pdhg_fields(x, [("q", q)], or_none=True)
    _pdhg_like(x, [("xbar", xbar), ("g", g), ("tau", tau)])
    with _on(x):
        L.check(L.lib().tomo_pdhg_primal_diag(x.device.index, ptr(x), ptr(xbar), ptr(g), ptr(tau), *_pdhg_ptrs(q), dx, dy, dz, nd,
                                              int(bool(nonneg)), stream_ptr(x)))


# ---- PDHG with the stripe variable (_data_["stripe_lambda"], docs/kernels/pdhg.md; include/tomo_mi355x.h)
def pdhg_stripe_segments(na: int) -> int:
    """n_seg = ceil(na / 64): the segments the angles are cut into for the sum of y along them"""
    return (int(na) + L.PDHG_STRIPE_SEG - 1) // L.PDHG_STRIPE_SEG


def _pdhg_stripe_like(first, named):
    """every (name, array, shape) is float32, contiguous, of that shape and on the device of `first`"""
    for name, t, shape in named:
        _chk_f32(t, name)
        if tuple(t.shape) != tuple(shape) or t.device != first.device:
            raise ValueError(f"{name} must have the shape {tuple(shape)} and the device of the first array")


def pdhg_sino_dual_stripe(y, r, b, sbar, part, fidelity: str, sigma):
    """Step 2 of a PDHG iteration with the stripe variable (tomo_pdhg_sino_dual_stripe): `pdhg_sino_dual` on e = r + s-bar,
    s-bar[z, u] added to every angle, `y` [nz, angles, nu] in place; in the same pass `part`[k, z, u] <- the sum of the new
    y[z, a, u] over the 64 angles of segment k.  `sigma`: a float32 scalar, or an array like `y` (a step per sample)."""
    if fidelity not in L.PDHG_FID:
        raise ValueError(f"unknown PDHG data term {fidelity!r}: LS, L1 and KL are supported")
    per_sample = isinstance(sigma, torch.Tensor)
    _chk_f32(y, "y")
    if y.dim() != 3:
        raise ValueError("the stripe launches take the sinogram dual as a [nz, angles, nu] array")
    nz, na, nu = y.shape
    _pdhg_stripe_like(y, [("r", r, y.shape), ("b", b, y.shape)] + ([("sigma", sigma, y.shape)] if per_sample else [])
                      + [("sbar", sbar, (nz, nu)), ("part", part, (pdhg_stripe_segments(na), nz, nu))])
    with _on(y):
        L.check(L.lib().tomo_pdhg_sino_dual_stripe(ptr(y), ptr(r), ptr(b), ptr(sigma if per_sample else None), ptr(sbar), ptr(part),
                                                   nz, na, nu, L.PDHG_FID[fidelity], 0.0 if per_sample else float(sigma),
                                                   stream_ptr(y)))
    return y


def pdhg_stripe_update(s, sbar, part, na, tau_s, theta):
    """Step 6 of a PDHG iteration with the stripe variable (tomo_pdhg_stripe_update): c = the sum of `part` over its
    segments, s' = the soft threshold of s - tau_s c at theta; s-bar <- 2 s' - s, s <- s', in place.  `s`, `sbar`: [nz, nu];
    `part`: [ceil(na / 64), nz, nu], `na` the number of angles it was summed over."""
    _chk_f32(s, "s")
    if s.dim() != 2:
        raise ValueError("the stripe variable is a [nz, nu] array")
    nz, nu = s.shape
    _pdhg_stripe_like(s, [("sbar", sbar, (nz, nu)), ("part", part, (pdhg_stripe_segments(na), nz, nu))])
    with _on(s):
        L.check(L.lib().tomo_pdhg_stripe_update(ptr(s), ptr(sbar), ptr(part), nz, int(na), nu, float(tau_s), float(theta),
                                                stream_ptr(s)))


# ---- PDHG with the second-order TGV term in its dual ("PD_TGV", docs/kernels/pdhg.md)
def pdhg_tgv_work_arrays(shape, device, tau: bool = False):
    """The work arrays of one PDHG call with the TGV block on a volume of `shape` ([nz, ny, nx]), uninitialised, from the
    placed block of ``PDHG_SLOT``: (x-bar, g, [P_1 .. P_nd], [Q11, Q22, Q12 (, Q33, Q13, Q23)], [v_1 .. v_nd],
    [v-bar_1 .. v-bar_nd]) and the lease token of ``placed_empty``; nd = 3 if nz > 1 else 2.  The block has the size
    ``tomo_pdhg_tgv_scratch_bytes`` states.  `tau` (the diagonal preconditioner): one more array behind the others, the steps
    per voxel, returned in front of the lease; the block then has the size ``tomo_pdhg_tgv_diag_scratch_bytes`` states."""
    nd = 3 if shape[0] > 1 else 2
    nq = 6 if nd == 3 else 3
    count = 2 + 3 * nd + nq
    arrays, lease = placed_empty([(tuple(shape), torch.float32)] * (count + bool(tau)), device, slot=PDHG_SLOT)
    p, q = arrays[2:2 + nd], arrays[2 + nd:2 + nd + nq]
    v, vbar = arrays[2 + nd + nq:2 + 2 * nd + nq], arrays[2 + 2 * nd + nq:count]
    if tau:
        return arrays[0], arrays[1], p, q, v, vbar, arrays[count], lease
    return arrays[0], arrays[1], p, q, v, vbar, lease


def _pdhg_tgv_fields(x, groups, q):
    """(dx, dy, dz, nd) of `_pdhg_fields` for the nd-field `groups`, and `q` holds the 3 (nd = 2) or 6 (nd = 3) Q fields"""
    dx, dy, dz, nd = _pdhg_fields(x, groups)
    nq = 6 if nd == 3 else 3
    if len(q) != nq:
        raise ValueError(f"a volume of {dz} plane{'s' if dz > 1 else ''} takes {nq} Q fields, got {len(q)}")
    _pdhg_like(x, [(f"q{k + 1}", t) for k, t in enumerate(q)])
    return dx, dy, dz, nd


def _ptr_array(group):
    """the host array of device pointers the tomo_pdhg_tgv_* entry points take for one group of fields"""
    return (C.c_void_p * len(group))(*[t.data_ptr() for t in group])


def pdhg_tgv_dual(xbar, vbar, p, q, sigma_p, sigma_q, r1, r0):
    """Step 4 of a PDHG iteration with the TGV block (tomo_pdhg_tgv_dual): P_d <- P_d + sigma_p (F_d(x-bar) - v-bar_d),
    projected onto the ball of radius `r1`; Q <- Q + sigma_q E(v-bar), projected onto the ball of radius `r0`; in place.
    `vbar` and `p` hold nd fields like `xbar`, `q` 3 (Q11, Q22, Q12) or 6 (..., Q33, Q13, Q23)."""
    dx, dy, dz, nd = _pdhg_tgv_fields(xbar, [("vbar", vbar), ("p", p)], q)
    with _on(xbar):
        L.check(L.lib().tomo_pdhg_tgv_dual(xbar.device.index, ptr(xbar), _ptr_array(vbar), _ptr_array(p), _ptr_array(q), dx, dy, dz,
                                           nd, float(sigma_p), float(sigma_q), float(r1), float(r0), stream_ptr(xbar)))


def pdhg_tgv_primal(x, xbar, g, v, vbar, p, q, tau_x, tau_v, nonneg=False):
    """Step 5 of a PDHG iteration with the TGV block (tomo_pdhg_tgv_primal, tomo_pdhg_tgv_primal_diag): x' = x - tau_x (g -
    div P), clamped at 0 with `nonneg`; x-bar <- 2 x' - x, x <- x'; v'_d = v_d + tau_v (P_d + the backward differences of
    Q's row d), v-bar_d <- 2 v'_d - v_d, v_d <- v'_d; in place.  `tau_x`: a float32 scalar, or an array like `x` (a step per
    voxel); `tau_v` a scalar."""
    dx, dy, dz, nd = _pdhg_tgv_fields(x, [("v", v), ("vbar", vbar), ("p", p)], q)
    per_voxel = isinstance(tau_x, torch.Tensor)
    _pdhg_like(x, [("xbar", xbar), ("g", g)] + ([("tau_x", tau_x)] if per_voxel else []))
    groups = (_ptr_array(v), _ptr_array(vbar), _ptr_array(p), _ptr_array(q))
    with _on(x):
        if per_voxel:
            L.check(L.lib().tomo_pdhg_tgv_primal_diag(x.device.index, ptr(x), ptr(xbar), ptr(g), ptr(tau_x), *groups, dx, dy, dz, nd,
                                                      float(tau_v), int(bool(nonneg)), stream_ptr(x)))
        else:
            L.check(L.lib().tomo_pdhg_tgv_primal(x.device.index, ptr(x), ptr(xbar), ptr(g), *groups, dx, dy, dz, nd, float(tau_x),
                                                 float(tau_v), int(bool(nonneg)), stream_ptr(x)))


# ----------------------------------------------------------------------------- SPDHG (docs/kernels/spdhg.md)
SPDHG_SLOT = 6  # the placed block of the SPDHG driver's work arrays


def spdhg_work_arrays(shape, device, tv: bool = True):
    """The work arrays of one SPDHG call on a volume of `shape` ([nz, ny, nx]), uninitialised, from the placed block of
    ``SPDHG_SLOT``: (z, delta, [q_1 .. q_nd], [e_1 .. e_nd]) and the lease token of ``placed_empty``; nd = 3 if nz > 1 else
    2, no q and e without the TV block.  With it the block has the size ``tomo_spdhg_scratch_bytes`` states."""
    nd = 3 if shape[0] > 1 else 2
    arrays, lease = placed_empty([(tuple(shape), torch.float32)] * (2 + (2 * nd if tv else 0)), device, slot=SPDHG_SLOT)
    return arrays[0], arrays[1], arrays[2:2 + nd] if tv else [], arrays[2 + nd:] if tv else [], lease


def spdhg_sino_dual(y, r, b, fidelity: str, sigma):
    """Step 2 of an SPDHG subset update (tomo_spdhg_sino_dual): v = PDHG's sinogram dual of the data term `fidelity` ("LS",
    "L1" or "KL") on (y, r, b); `r` <- v - y, `y` <- v, both in place.  `r` = A_j x, `b` = the subset's data, `sigma` a
    float32 scalar.  Returns (y, r)."""
    if fidelity not in L.PDHG_FID:
        raise ValueError(f"unknown SPDHG data term {fidelity!r}: LS, L1 and KL are supported")
    _pdhg_flat([("y", y), ("r", r), ("b", b)])
    with _on(y):
        L.check(L.lib().tomo_spdhg_sino_dual(ptr(y), ptr(r), ptr(b), y.numel(), L.PDHG_FID[fidelity], float(sigma), stream_ptr(y)))
    return y, r


def spdhg_primal(x, z, delta, tau, w, nonneg=False):
    """Step 4 of an SPDHG subset update (tomo_spdhg_primal): z' = z + delta, zb = z' + w delta, x' = x - tau zb, clamped at 0
    with `nonneg`; `x` <- x', `z` <- z', in place.  `delta` = A_j^T of the dual's change, `w` = 1 / the block's probability."""
    _pdhg_flat([("x", x), ("z", z), ("delta", delta)])
    with _on(x):
        L.check(L.lib().tomo_spdhg_primal(ptr(x), ptr(z), ptr(delta), x.numel(), float(tau), float(w), int(bool(nonneg)),
                                          stream_ptr(x)))


def spdhg_tv_dual(x, q, e, sigma, lam, methodTV=0):
    """Step 1 of an SPDHG TV update (tomo_spdhg_tv_dual): p_d = q_d + sigma F_d(x), projected (methodTV 0: onto the ball of
    radius `lam`, 1: onto the box); `e` <- p - q, `q` <- p.  `q` and `e` hold nd fields like `x` each."""
    dx, dy, dz, nd = _pdhg_fields(x, [("q", q), ("e", e)])
    with _on(x):
        L.check(L.lib().tomo_spdhg_tv_dual(x.device.index, ptr(x), *_pdhg_ptrs(q), *_pdhg_ptrs(e), dx, dy, dz, nd, float(sigma),
                                           float(lam), int(methodTV), stream_ptr(x)))


def spdhg_tv_primal(x, z, e, tau, w, nonneg=False):
    """Steps 2 and 3 of an SPDHG TV update (tomo_spdhg_tv_primal): div = sum_d B_d(e_d); z' = z - div, zb = z' - w div,
    x' = x - tau zb, clamped at 0 with `nonneg`; `x` <- x', `z` <- z', in place.  `e`: the nd fields spdhg_tv_dual left."""
    dx, dy, dz, nd = _pdhg_fields(x, [("e", e)])
    _pdhg_like(x, [("z", z)])
    with _on(x):
        L.check(L.lib().tomo_spdhg_tv_primal(x.device.index, ptr(x), ptr(z), *_pdhg_ptrs(e), dx, dy, dz, nd, float(tau), float(w),
                                             int(bool(nonneg)), stream_ptr(x)))


def _wavelet_args(data, out, mix):
    _chk_f32(data, "data")
    if data.dim() not in (2, 3):
        raise ValueError("2D or 3D arrays must be provided only")
    for name, t in (("out", out), ("mix", mix)):
        if t is not None:
            _chk_f32(t, name)
            if tuple(t.shape) != tuple(data.shape) or t.device != data.device:
                raise ValueError(f"{name} must have the shape and the device of the data")


def wavelet_shrink(data, threshold, out=None, mix=None):
    """Wavelet shrinkage (tomo_wavelet_shrink; the algorithm: docs/kernels/wavelets.md): three db5 levels of every (y, x)
    slice of `data` (2D, or 3D = a stack of slices), soft threshold `threshold` (a float32 scalar >= 0) on the detail
    coefficients, inverse, into `out` (default: a new array; it may be `data`).  With `mix` (an array like `out`; it may be
    `out`) what is stored is ``(mix + W(data)) * 0.5``.  The coefficient pyramid lives in the TV scratch arena."""
    if out is None:
        out = torch.empty_like(data)
    _wavelet_args(data, out, mix)
    dx, dy, dz, nd = _tv_dims(data)
    with torch.cuda.device(data.device):
        L.check(L.lib().tomo_wavelet_shrink(data.device.index, ptr(data), ptr(out), ptr(mix), dx, dy, dz, nd, float(threshold),
                                            stream_ptr(data)))
    return out


def wavelet_pyramid_floats(shape) -> int:
    """floats of the coefficient pyramid of an array of `shape` (tomo_wavelet_scratch_bytes / 4)"""
    nd = len(shape)
    dz, dy, dx = (1, *shape) if nd == 2 else shape
    return int(L.lib().tomo_wavelet_scratch_bytes(dx, dy, dz, nd)) // 4


def wavelet_forward(data, threshold=0.0):
    """The thresholded coefficient pyramid of `data` as a flat float32 array (tomo_wavelet_forward; layout:
    include/tomo_mi355x.h)."""
    _wavelet_args(data, None, None)
    dx, dy, dz, nd = _tv_dims(data)
    pyr = torch.empty(wavelet_pyramid_floats(data.shape), dtype=torch.float32, device=data.device)
    with torch.cuda.device(data.device):
        L.check(L.lib().tomo_wavelet_forward(data.device.index, ptr(data), ptr(pyr), dx, dy, dz, nd, float(threshold),
                                             stream_ptr(data)))
    return pyr


def wavelet_inverse(pyramid, shape, out=None, mix=None):
    """The array of `shape` a pyramid (as `wavelet_forward` returns it) is the transform of (tomo_wavelet_inverse).  LL of
    levels 1 and 2 of `pyramid` are overwritten.  `mix` as for `wavelet_shrink`."""
    _chk_f32(pyramid, "pyramid")
    if pyramid.numel() != wavelet_pyramid_floats(shape):
        raise ValueError("the pyramid does not have the size of the pyramid of an array of this shape")
    if out is None:
        out = torch.empty(tuple(shape), dtype=torch.float32, device=pyramid.device)
    _wavelet_args(out, out, mix)
    dx, dy, dz, nd = _tv_dims(out)
    with torch.cuda.device(out.device):
        L.check(L.lib().tomo_wavelet_inverse(out.device.index, ptr(pyramid), ptr(out), ptr(mix), dx, dy, dz, nd, stream_ptr(out)))
    return out


def _nltv_tables(data, tables):
    """the three tables of an array `data`, checked: (K, *data.shape), uint16 / uint16 / float32, contiguous, on its device"""
    hi, hj, w = tables
    for name, t, dtype in (("H_i", hi, torch.uint16), ("H_j", hj, torch.uint16), ("Weights", w, torch.float32)):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype:
            raise ValueError(f"{name} must be a {str(dtype).replace('torch.', '')} array")
        if not t.is_contiguous() or t.device != data.device:
            raise ValueError(f"{name} must be C-contiguous and live on the device of the data")
        if t.dim() != data.dim() + 1 or tuple(t.shape[1:]) != tuple(data.shape) or t.shape[0] != w.shape[0]:
            raise ValueError(f"{name} must have the shape (neighbours, *data.shape) = ({int(w.shape[0])}, "
                             f"{', '.join(map(str, data.shape))}), got {tuple(t.shape)}")
    return int(w.shape[0])


def patch_select(data, searchwindow, patchwindow, neighbours, edge_parameter):
    """The neighbour tables of non-local TV (tomo_patch_select; the algorithm: docs/kernels/nltv.md): for every pixel of every
    (y, x) slice of `data` (2D, or 3D = a stack of slices along axis 0) the `neighbours` most similar pixels inside the search
    window.  Returns (H_i, H_j, Weights) of shape (neighbours, *data.shape): the x and y indices (uint16) and the weights
    (float32), 8 * neighbours bytes per voxel."""
    _chk_f32(data, "data")
    if data.dim() not in (2, 3):
        raise ValueError("2D or 3D arrays must be provided only")
    dx, dy, dz, nd = _tv_dims(data)
    K = int(neighbours)
    if not 1 <= K <= 32:
        raise ValueError("PatchSelect: the number of neighbours must lie in [1, 32]")
    shape = (K, *data.shape)
    hi = torch.empty(shape, dtype=torch.uint16, device=data.device)
    hj = torch.empty(shape, dtype=torch.uint16, device=data.device)
    w = torch.empty(shape, dtype=torch.float32, device=data.device)
    with torch.cuda.device(data.device):
        L.check(L.lib().tomo_patch_select(data.device.index, ptr(data), ptr(hi), ptr(hj), ptr(w), dx, dy, dz, nd,
                                          int(searchwindow), int(patchwindow), K, float(edge_parameter), stream_ptr(data)))
    return hi, hj, w


def nltv(data, out, H_i, H_j, Weights, lam, iterations, tolerance=0.0):
    """Non-local TV (tomo_nltv; the algorithm: docs/kernels/nltv.md): `iterations` Jacobi iterations of `data` into `out` (a
    different array: the iterations ping-pong through it; `data` and the tables are never written) over the tables of
    `patch_select`, shape (neighbours, *data.shape).  `lam` is a float32 scalar.  Returns (out, iterations_done, rel_change)
    -- the last relative change the stopping rule evaluated, NaN if none (tolerance 0 = off)."""
    _chk_f32(data, "data")
    _chk_f32(out, "out")
    if data.dim() not in (2, 3):
        raise ValueError("2D or 3D arrays must be provided only")
    if tuple(out.shape) != tuple(data.shape) or out.device != data.device:
        raise ValueError("out must have the shape and the device of the data")
    K = _nltv_tables(data, (H_i, H_j, Weights))
    dx, dy, dz, nd = _tv_dims(data)
    done, last = C.c_int(0), C.c_double(float("nan"))
    with torch.cuda.device(data.device):
        L.check(L.lib().tomo_nltv(data.device.index, ptr(data), ptr(out), ptr(H_i), ptr(H_j), ptr(Weights), dx, dy, dz, nd, K,
                                  float(lam), int(iterations), float(tolerance), C.byref(done), C.byref(last), stream_ptr(data)))
    return out, int(done.value), float(last.value)


_variant_state = threading.local()   # mirror of the library's per-thread switches, per flavour: lets `variant()` restore


def set_variant(kernel: str, variant: int):
    L.check(L.lib().tomo_set_variant(kernel.encode(), int(variant)))
    state = getattr(_variant_state, "v", None)
    if state is None:
        state = _variant_state.v = {}
    state[(L.flavour(), kernel)] = int(variant)


def get_variant(kernel: str) -> int:
    """The variant this thread last selected for `kernel` in the current library flavour (0 = default)."""
    return getattr(_variant_state, "v", {}).get((L.flavour(), kernel), 0)


class _DeviceBytes:
    """Zero-copy hand-over of library-owned device memory to torch (``torch.as_tensor`` reads ``__cuda_array_interface__``)."""

    def __init__(self, ptr: int, nbytes: int):
        self.__cuda_array_interface__ = {"shape": (int(nbytes),), "typestr": "|u1", "data": (int(ptr), False),
                                         "version": 2, "strides": None}


ARRAY_SKEW = 69888   # bytes between consecutive work arrays of a placed block (what the library uses between its own)


def placed_empty(specs, device, slot: int = 0):
    """Uninitialised work arrays inside ONE placed scratch block of the library (include/tomo_mi355x.h,
    tomo_placed_scratch): ``specs`` is a list of (shape, dtype); returns (one tensor per entry, 256-byte aligned and
    ``ARRAY_SKEW`` apart; a lease token).  The block belongs to the library (grow-only per (device, stream, slot), freed
    by ``tomo_release_scratch``): the tensors are views for the duration of ONE driver call, not allocations to keep, and
    a second ``placed_empty`` on the same (device, stream, slot) supersedes them -- ``lease_is_current(token)`` tells.
    Slots in use: the ``slot`` of the records of tomobar_amd/supp/regularisers.py, one per slab driver, ``PDHG_SLOT`` and
    ``SPDHG_SLOT``."""
    device = torch.device(device)
    sizes, total = [], 0
    for shape, dtype in specs:
        nb = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        sizes.append((total, nb))
        total += (nb + 255) // 256 * 256 + ARRAY_SKEW
    out = C.c_void_p(0)
    with torch.cuda.device(device):
        stream_id = torch.cuda.current_stream(device).cuda_stream
        L.check(L.lib().tomo_placed_scratch(device.index or 0, int(slot), total, C.c_void_p(stream_id), C.byref(out)))
        block = torch.as_tensor(_DeviceBytes(out.value, total), device=device)
    key = (L.flavour(), device.index or 0, stream_id, int(slot))
    with _lease_lock:
        _lease_generation[key] = _lease_generation.get(key, 0) + 1
        lease = (key, _lease_generation[key])
    arrays = [block[o:o + nb].view(dtype).view(tuple(shape)) for (o, nb), (shape, dtype) in zip(sizes, specs)]
    return arrays, lease


_lease_lock = threading.Lock()
_lease_generation = {}   # (flavour, device, stream, slot) -> how many times placed_empty handed the slot's block out


def lease_is_current(lease) -> bool:
    """True while nobody else has taken the same (device, stream, slot) block since ``placed_empty`` returned `lease`: the
    arrays of an older lease may have been overwritten -- or freed, if the newer request was larger -- and must not be
    read any more (the slab drivers check this before they copy their result out)."""
    key, gen = lease
    with _lease_lock:
        return _lease_generation.get(key) == gen


def reserve_tv_scratch(shape, device, method: str = "PD_TV", half: bool = False):
    """Allocate and place the library's TV scratch arena for volumes of `shape` on the current stream of `device` now
    (set-up time) instead of inside the first proximal step (include/tomo_mi355x.h, tomo_reserve_scratch)."""
    device = torch.device(device)
    nd = len(shape)
    dz, dy, dx = (1, *shape) if nd == 2 else shape
    lib = L.lib()
    kind = BY_NAME.get(method, BY_NAME["ROF_TV"])
    nbytes = getattr(lib, kind.scratch)(dx, dy, dz, nd, *([int(bool(half))] if kind.scratch_half else []))
    with torch.cuda.device(device):
        L.check(lib.tomo_reserve_scratch(device.index or 0, nbytes, C.c_void_p(torch.cuda.current_stream(device).cuda_stream)))


def reserve_tv_slices_scratch(shape, device, method: str = "PD_TV", half: bool = False):
    """`reserve_tv_scratch` for the slice-wise form of PD_TV / ROF_TV on a 3D array of `shape` (tomo_pdtv_slices_scratch_bytes /
    tomo_roftv_slices_scratch_bytes)."""
    if method not in SLICEWISE_KINDS:
        raise ValueError(f"{method} does not support slicewise=True")
    device = torch.device(device)
    dz, dy, dx = shape
    lib = L.lib()
    nbytes = (lib.tomo_pdtv_slices_scratch_bytes(dx, dy, dz, int(bool(half))) if method == "PD_TV"
              else lib.tomo_roftv_slices_scratch_bytes(dx, dy, dz))
    with torch.cuda.device(device):
        L.check(lib.tomo_reserve_scratch(device.index or 0, nbytes, C.c_void_p(torch.cuda.current_stream(device).cuda_stream)))


def reserve_wavelet_scratch(shape, device):
    """`reserve_tv_scratch` for the coefficient pyramid of the wavelet shrinkage of arrays of `shape`: it lives in the same
    arena, which is grow-only, so after both calls the arena holds the larger of the two needs."""
    device = torch.device(device)
    with torch.cuda.device(device):
        L.check(L.lib().tomo_reserve_scratch(device.index or 0, 4 * wavelet_pyramid_floats(tuple(shape)),
                                             C.c_void_p(torch.cuda.current_stream(device).cuda_stream)))


def reserve_nltv_scratch(shape, device):
    """`reserve_tv_scratch` for the one work array of the NLTV iterations on arrays of `shape` (tomo_nltv_scratch_bytes; a 3D
    shape is a stack of slices, singleton axes included)."""
    device = torch.device(device)
    nd = len(shape)
    dz, dy, dx = (1, *shape) if nd == 2 else shape
    lib = L.lib()
    with torch.cuda.device(device):
        L.check(lib.tomo_reserve_scratch(device.index or 0, lib.tomo_nltv_scratch_bytes(dx, dy, dz, nd),
                                         C.c_void_p(torch.cuda.current_stream(device).cuda_stream)))


def set_placement_tries(tries: int):
    """Candidate allocations the library scores when it places a TV scratch arena of >= 1 GiB (include/tomo_mi355x.h,
    tomo_set_placement_tries; default 8 or TOMO_MI355X_PLACE_TRIES, at most 10; 1 = plain hipMalloc)."""
    L.check(L.lib().tomo_set_placement_tries(int(tries)))


def placement_tries() -> int:
    return int(L.lib().tomo_placement_tries())


def placement_last():
    """The library's most recent arena placement search: {"bytes", "chosen", "scores_GBps", "fast"} or None if none ran
    yet.  "fast": the kept block beat an earlier candidate by the 8 % that separates the fast class of blocks from the
    slow one (False: the tries ran out first -- either no candidate was in the fast class: expect the TV launches 4-10 % slower, or
    all of them were and none stood out: compare the scores, fast blocks of a 34 GB arena score >= 5.23 TB/s)."""
    nbytes, chosen = C.c_size_t(0), C.c_int(-1)
    scores = (C.c_double * 16)()
    n = L.lib().tomo_placement_last(C.byref(nbytes), C.byref(chosen), scores, 16)
    if n <= 0:
        return None
    return {"bytes": int(nbytes.value), "chosen": int(chosen.value), "scores_GBps": [round(float(scores[i]), 1) for i in range(n)],
            "fast": bool(L.lib().tomo_placement_last_fast() == 1)}


@contextlib.contextmanager
def variant(kernel: str, value: int):
    """`with ops.variant("pdtv", 22): ...` -- select a kernel variant for a block and restore what was selected before."""
    prev = get_variant(kernel)
    set_variant(kernel, value)
    try:
        yield
    finally:
        set_variant(kernel, prev)
