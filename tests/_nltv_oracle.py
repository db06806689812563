"""numpy restatement of docs/kernels/nltv.md: the exponential ``wexp``, PatchSelect and the NLTV iteration, in the stated
order of operations.  Every function takes the dtype: float32 is what the kernels reproduce bit for bit, float64 runs
beside it to measure what the float32 rounding costs.  Every operation below is a numpy ufunc on arrays (or scalars) of
that dtype, so each one is rounded once and nothing is contracted.

A 3D array is a stack of independent (y, x) slices along axis 0."""
import numpy as np

LOG2E = 1.4426950408889634
# (-ln 2)^k / k!, k = 0 .. 7, as float64 literals
WEXP_C = (1.0, -0.6931471805599453, 0.2402265069591007, -0.05550410866482158, 0.009618129107628477,
          -0.0013333558146428443, 0.0001540353039338161, -1.5252733804059840e-05)
EPS = 1e-12


def wexp(x, dtype=np.float32):
    """exp(-x) for x >= 0 by the specification's range reduction and degree-7 polynomial"""
    x = np.asarray(x, dtype)
    y = np.minimum(x * dtype(LOG2E), dtype(126.0))
    n = np.rint(y)
    r = y - n
    p = np.full_like(r, dtype(WEXP_C[7]))
    for k in range(6, -1, -1):
        p = p * r
        p = p + dtype(WEXP_C[k])
    return np.ldexp(p, -n.astype(np.int32)).astype(dtype)


def patch_kernel(P, dtype=np.float32):
    """g[t], t = 0 .. 2P"""
    k = np.arange(-P, P + 1)
    return wexp(np.asarray(k * k, dtype) / dtype(2 * P * P), dtype)


def candidates(S):
    """the offsets (j_m, i_m) in candidate order"""
    return [(jm, im) for jm in range(-S, S + 1) for im in range(-S, S + 1) if (jm, im) != (0, 0)]


def _shifted(A, jm, im):
    """(B, ok): B[y, x] = A[y + jm, x + im] where that pixel is inside the slice (ok), else 0"""
    ny, nx = A.shape
    B = np.zeros_like(A)
    ok = np.zeros(A.shape, bool)
    y0, y1 = max(0, -jm), min(ny, ny - jm)
    x0, x1 = max(0, -im), min(nx, nx - im)
    if y0 < y1 and x0 < x1:
        B[y0:y1, x0:x1] = A[y0 + jm:y1 + jm, x0 + im:x1 + im]
        ok[y0:y1, x0:x1] = True
    return B, ok


def _filter(D, g, P, axis):
    """sum over t ascending of g[t] * D(. + t - P) along `axis`, zero outside, starting from 0"""
    n = D.shape[axis]
    pad = [(0, 0), (0, 0)]
    pad[axis] = (P, P)
    Dp = np.pad(D, pad)
    acc = np.zeros_like(D)
    for t in range(2 * P + 1):
        term = g[t] * (Dp[t:t + n, :] if axis == 0 else Dp[:, t:t + n])
        acc = acc + term
    return acc


def distances(A, S, P, dtype=np.float32):
    """(d, valid) of one slice: d[m] the patch distance of every pixel to candidate m, valid[m] where the candidate lies
    inside the slice"""
    A = np.asarray(A, dtype)
    g = patch_kernel(P, dtype)
    cand = candidates(S)
    d = np.empty((len(cand),) + A.shape, dtype)
    valid = np.empty((len(cand),) + A.shape, bool)
    for m, (jm, im) in enumerate(cand):
        B, ok = _shifted(A, jm, im)
        diff = A - B
        D = np.where(ok, diff * diff, dtype(0))
        d[m] = _filter(_filter(D, g, P, 1), g, P, 0)
        valid[m] = ok
    return d, valid


def _patch_select_2d(A, S, P, K, h, dtype):
    ny, nx = A.shape
    d, valid = distances(A, S, P, dtype)
    cand = np.array(candidates(S))
    # the K valid candidates of smallest d, ties to the earlier one: keys from the last (primary) to the first
    order = np.lexsort((np.broadcast_to(np.arange(len(cand))[:, None, None], d.shape), d, ~valid), axis=0)[:K]
    yy, xx = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    H_i = np.broadcast_to(xx, (K, ny, nx)).astype(np.uint16, order="C")
    H_j = np.broadcast_to(yy, (K, ny, nx)).astype(np.uint16, order="C")
    W = np.zeros((K, ny, nx), dtype)
    h = dtype(h)
    inv = dtype(1.0) / (h * h)
    for k in range(min(K, len(cand))):
        m = order[k]
        sel = np.take_along_axis(valid, m[None], 0)[0]
        dk = np.take_along_axis(d, m[None], 0)[0]
        H_i[k] = np.where(sel, xx + cand[m, 1], xx)
        H_j[k] = np.where(sel, yy + cand[m, 0], yy)
        W[k] = np.where(sel, wexp(dk * inv, dtype), dtype(0))
    return H_i, H_j, W


def patch_select(A, searchwindow, patchwindow, neighbours, edge_parameter, dtype=np.float32):
    """(H_i, H_j, Weights) of shape (K, *A.shape): uint16, uint16, dtype"""
    A = np.asarray(A, dtype)
    S, P, K = int(searchwindow), int(patchwindow), int(neighbours)
    assert 1 <= S <= 15 and 1 <= P <= 4 and 1 <= K <= 32 and edge_parameter > 0
    if A.ndim == 2:
        return _patch_select_2d(A, S, P, K, edge_parameter, dtype)
    per_slice = [_patch_select_2d(a, S, P, K, edge_parameter, dtype) for a in A]
    return tuple(np.stack([t[n] for t in per_slice], axis=1) for n in range(3))


def _nltv_2d(f, H_i, H_j, W, lam, iterations, dtype):
    mu = dtype(1.0) / dtype(lam)
    u = f.copy()
    for _ in range(iterations):
        s = np.zeros_like(f)
        val = np.zeros_like(f)
        nw = np.zeros_like(f)
        for k in range(W.shape[0]):
            uk = u[H_j[k], H_i[k]]
            diff = uk - u
            s = s + W[k] * (diff * diff)
            val = val + W[k] * uk
            nw = nw + W[k]
        c = dtype(2.0) / np.sqrt(s + dtype(EPS))
        u = (mu * f + c * val) / (mu + c * nw)
    return u


def nltv(f, H_i, H_j, W, lam, iterations, dtype=np.float32):
    """`iterations` Jacobi iterations from u = f; the tables have shape (K, *f.shape)"""
    f = np.asarray(f, dtype)
    W = np.asarray(W, dtype)
    H_i, H_j = np.asarray(H_i).astype(np.intp), np.asarray(H_j).astype(np.intp)
    if f.ndim == 2:
        return _nltv_2d(f, H_i, H_j, W, lam, iterations, dtype)
    return np.stack([_nltv_2d(f[z], H_i[:, z], H_j[:, z], W[:, z], lam, iterations, dtype) for z in range(f.shape[0])])


# ------------------------------------------------------------------------------------------------ test images
def terraces(shape):
    """clean piecewise-constant image: most patch distances tie, so the tie-break decides the selection"""
    ny, nx = shape[-2:]
    y, x = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    img = (0.25 * ((x // 5) % 3) + 0.5 * ((y // 4) % 2)).astype(np.float32)
    if len(shape) == 3:
        img = np.stack([np.roll(img, z, axis=1) for z in range(shape[0])])
    return np.ascontiguousarray(img)


def clean_phantom(shape):
    """discs and a ramp in [0, 1]"""
    ny, nx = shape[-2:]
    y, x = np.meshgrid(np.linspace(-1, 1, ny) if ny > 1 else np.zeros(1), np.linspace(-1, 1, nx) if nx > 1 else np.zeros(1),
                       indexing="ij")
    img = 0.2 * (x + 1) * 0.5
    img = img + 0.6 * ((x * x + y * y) < 0.6) - 0.3 * (((x - 0.2) ** 2 + (y + 0.1) ** 2) < 0.08)
    img = img + 0.3 * ((np.abs(x + 0.4) < 0.12) & (np.abs(y - 0.2) < 0.3))
    img = img.astype(np.float32)
    if len(shape) == 3:
        img = np.stack([img * np.float32(1.0 - 0.1 * z / shape[0]) for z in range(shape[0])])
    return np.ascontiguousarray(img)


def noisy_phantom(shape, sigma=0.1, seed=0):
    rng = np.random.default_rng(seed)
    return (clean_phantom(shape) + np.float32(sigma) * rng.standard_normal(shape).astype(np.float32)).astype(np.float32)
