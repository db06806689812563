"""TEST INFRASTRUCTURE: numpy restatement of the wavelet shrinkage of docs/kernels/wavelets.md (tomobar_amd/csrc/wavelet_kernels.hip): three
levels of the 2D orthonormal Daubechies-5 transform of every (y, x) slice in periodization mode, soft threshold on the
detail coefficients, inverse transform.  ``dtype=np.float64`` is the mathematical statement (the literals as float64, float64
arithmetic); ``dtype=np.float32`` reproduces the kernel bit for bit: float32 roundings of the committed literals, every
product rounded, every sum rounded, accumulation from 0 in ascending k, in the inverse the h term before the g term."""
import numpy as np

LEVELS = 3
# the literals the kernel commits (docs/kernels/wavelets.md); test_wavelet_oracle.py holds them against derive_taps()
H_LITERALS = (0.16010239797419293, 0.6038292697971896, 0.7243085284377733, 0.1384281459013205, -0.242294887066382,
              -0.03224486958463838, 0.0775714938400457, -0.006241490212798274, -0.012580751999082002, 0.0033357252854737717)


def derive_taps():
    """The db5 scaling filter in float64 from the Daubechies polynomial P(y) = sum_{k<5} C(4+k, k) y^k, y = (2 - z - 1/z)/4:
    the roots of P (numpy.roots, polished by Newton steps), of each reciprocal pair z, 1/z the one inside the unit circle
    (as the reciprocal of the larger one: no cancellation), h = (1 + z)^5 prod (z - z_i) by convolution, sum h = sqrt 2."""
    from math import comb
    p = [comb(4 + k, k) for k in range(5)][::-1]
    dp = np.polyder(p)
    y = np.roots(p)
    for _ in range(3):
        y = y - np.polyval(p, y) / np.polyval(dp, y)
    h = np.array([1.0 + 0.0j])
    for _ in range(5):
        h = np.convolve(h, [1.0, 1.0])
    for b in 2.0 - 4.0 * y:                                  # z^2 - b z + 1 = 0
        s = np.sqrt(b * b / 4.0 - 1.0 + 0.0j)
        outside = b / 2.0 + s if abs(b / 2.0 + s) >= abs(b / 2.0 - s) else b / 2.0 - s
        h = np.convolve(h, [1.0, -1.0 / outside])
    assert np.abs(h.imag).max() < 1e-14
    h = h.real
    return h * (np.sqrt(2.0) / h.sum())


def taps(dtype):
    """(h, g) as arrays of `dtype`: g[k] = (-1)^k h[9 - k]."""
    h = np.asarray(H_LITERALS, dtype=np.float64).astype(dtype)
    g = np.array([(-1) ** k * h[9 - k] for k in range(10)], dtype=dtype)
    return h, g


def _extend(x):
    """the last axis made even by one copy of its last sample"""
    return np.concatenate([x, x[..., -1:]], axis=-1) if x.shape[-1] & 1 else x


def analysis(x, dtype):
    """one axis (the last) forward: (a, d), each of ceil(n / 2) samples"""
    h, g = taps(dtype)
    xe = _extend(np.asarray(x, dtype=dtype))
    n_e = xe.shape[-1]
    m = n_e // 2
    a = np.zeros(xe.shape[:-1] + (m,), dtype=dtype)
    d = np.zeros_like(a)
    for k in range(10):
        s = xe[..., (2 * np.arange(m) + k) % n_e]
        a = a + h[k] * s
        d = d + g[k] * s
    return a, d


def synthesis(a, d, n, dtype):
    """one axis (the last) inverse of `analysis`, cropped to n samples"""
    h, g = taps(dtype)
    a, d = np.asarray(a, dtype=dtype), np.asarray(d, dtype=dtype)
    m = a.shape[-1]
    n_e = 2 * m
    xe = np.zeros(a.shape[:-1] + (n_e,), dtype=dtype)
    for k in range(10):
        j = np.arange(k & 1, n_e, 2)
        i = ((j - k) % n_e) // 2
        acc = xe[..., j] + h[k] * a[..., i]
        xe[..., j] = acc + g[k] * d[..., i]
    return xe[..., :n]


def _t(v):
    return np.swapaxes(v, -1, -2)


def forward_level(s, dtype):
    """(LL, LH, HL, HH) of the slices `s` [..., y, x]: x first, then y; first letter = the x filter"""
    lo, hi = analysis(s, dtype)
    ll, lh = (_t(v) for v in analysis(_t(lo), dtype))
    hl, hh = (_t(v) for v in analysis(_t(hi), dtype))
    return ll, lh, hl, hh


def inverse_level(ll, lh, hl, hh, ny, nx, dtype):
    """the slices of ny x nx whose forward_level the bands are: y first, then x"""
    lo = _t(synthesis(_t(ll), _t(lh), ny, dtype))
    hi = _t(synthesis(_t(hl), _t(hh), ny, dtype))
    return synthesis(lo, hi, nx, dtype)


def soft(d, t, dtype):
    v = np.abs(d) - dtype(t)
    return np.copysign(np.where(v > 0, v, dtype(0)), d).astype(dtype)


def forward(x, t=0.0, dtype=np.float32):
    """The pyramid of `x` ([y, x] or [z, y, x]): a list over the levels 1..3 of [LL, LH, HL, HH], the details thresholded
    by `t` (LL of level l is the input of level l + 1, unthresholded)."""
    s = np.asarray(x, dtype=dtype)
    levels = []
    for _ in range(LEVELS):
        ll, lh, hl, hh = forward_level(s, dtype)
        levels.append([ll, soft(lh, t, dtype), soft(hl, t, dtype), soft(hh, t, dtype)])
        s = ll
    return levels


def inverse(levels, shape, dtype=np.float32):
    """The array of `shape` from a pyramid: LL of level 3 and the details of all levels are read (LL_1, LL_2 are ignored)."""
    ny, nx = [shape[-2]], [shape[-1]]
    for _ in range(LEVELS):
        ny.append((ny[-1] + 1) // 2)
        nx.append((nx[-1] + 1) // 2)
    s = np.asarray(levels[-1][0], dtype=dtype)
    for lev in range(LEVELS, 0, -1):
        _, lh, hl, hh = levels[lev - 1]
        s = inverse_level(s, lh, hl, hh, ny[lev - 1], nx[lev - 1], dtype)
    return s


def shrink(x, t, dtype=np.float32, mix=None):
    """W_t(x); with `mix`: (mix + W_t(x)) * 0.5 in `dtype`."""
    x = np.asarray(x)
    w = inverse(forward(x, t, dtype), x.shape, dtype)
    if mix is not None:
        w = (np.asarray(mix, dtype=dtype) + w) * dtype(0.5)
    return w


def pack(levels):
    """The pyramid as the flat float array tomo_wavelet_forward writes: per slice, per level, LL, LH, HL, HH."""
    three_d = levels[0][0].ndim == 3
    nz = levels[0][0].shape[0] if three_d else 1
    per_slice = []
    for z in range(nz):
        parts = [(b[z] if three_d else b).ravel() for lev in levels for b in lev]
        per_slice.append(np.concatenate(parts))
    return np.concatenate(per_slice)


def unpack(flat, shape):
    """inverse of `pack` for an array of `shape`"""
    three_d = len(shape) == 3
    nz = shape[0] if three_d else 1
    ny, nx = shape[-2], shape[-1]
    dims = []
    for _ in range(LEVELS):
        ny, nx = (ny + 1) // 2, (nx + 1) // 2
        dims.append((ny, nx))
    per = 4 * sum(a * b for a, b in dims)
    flat = np.asarray(flat).reshape(nz, per)
    levels, at = [], 0
    for (a, b) in dims:
        bands = []
        for _ in range(4):
            blk = flat[:, at:at + a * b].reshape(nz, a, b)
            bands.append(blk.copy() if three_d else blk[0].copy())
            at += a * b
        levels.append(bands)
    return levels
