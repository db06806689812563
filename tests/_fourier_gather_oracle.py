"""TEST INFRASTRUCTURE: a per-grid-point reference of the Fourier gathering (csrc/fourier_inv.hip, gather_kernel), the cases
tests/test_fourier_gather_oracle.py (CPU) and tests/test_gpu_fourier_gather.py (MI355X) run, and the one comparison both apply.
Nothing here touches a GPU or imports the product package.

WHAT IS COMPUTED.  The frequency grid has 2n x 2n points (iy, ix); the polar samples are g[p][r] (angle p, radial sample r of
n), rr = (r - n/2) / n, coeff0 = pi / mu, coeff1 = -pi^2 / mu (pi the float32 literal of fft_us_kernels.cu:2).  With the centre
box of `center_size` points a side from base = max(0, n - center_size / 2), used when center_size >= 192
(methodsDIR_CuPy.py:23), every grid point holds  chk * sum_k w_k g[p_k][r_k],  chk = -1 where (ix ^ iy) & 1 (the first
c2dfftshift, fft_us_kernels.cu:579-603, which the kernel folds into its store), over the terms

  centre form, points inside the box (gather_kernel_center, fft_us_kernels.cu:376-517):  px = (ix - n) / 2n, py = (n - iy) / 2n;
      a ray p with v = (cos, sin) / 2 takes part when  radius_2 >= d2,  radius_2 = 2 (m + 1/2)^2 / 4n^2,  d2 = |q - (px, py)|^2,
      q = ((v . (px, py)) v) / (1/4) the foot of the point on the ray; its samples rmin <= r < rmax with dti = sqrt(radius_2 - d2),
      rmin = n/2 - 1 + floor((q_a - dti v_a / (1/2)) / (2 v_a / n)),  rmax = n/2 + 1 + floor((q_a + dti v_a / (1/2)) / (2 v_a / n)),
      a = x where |v_x| > |v_y|, else y; swapped when rmin > rmax, both clipped to 0 .. n-1;
      w = coeff0 exp(coeff1 ((px - x0)^2 + (py - y0)^2)),  x0 = clamp_half(rr cos), y0 = clamp_half(rr sin);
  square form, every other point (gather_kernel, fft_us_kernels.cu:5-113, seen from the receiving side):  a sample takes part when
      the point is ((l0 + 3n) mod 2n, (l1 + 3n) mod 2n) for a cell e0 - m <= l0 <= e0 + m, e1 - m <= l1 <= e1 + m of its footprint,
      e0 = floor(2n x0), e1 = floor(2n y0),  x0 = clamp_half(rr cos), y0 = clamp_half(-rr sin);
      w = coeff0 exp(coeff1 ((l0 / 2n - x0)^2 + (l1 / 2n - y0)^2));
  clamp_half(v) = 0.5f - 1e-5f where v >= 0.5, else v.

DECISIONS are the comparisons and floors above.  `sel` takes them in float32 IEEE arithmetic, one rounding per operation and no
contraction, from the float32 cos / sin tables the caller passes.  Beside it every decision is evaluated in float64 from the
same inputs with the error the float32 evaluation can have (u = 2^-24, first order, doubled: SAFETY), and a term whose taking
part depends on a decision closer to its boundary than that is MAYBE -- it may be there or not.  The widths, from the
operations that produce each quantity (e_x: bound of the absolute error of x; an FMA removes one rounding of a product, so a
contracted evaluation lies within the same widths):

  px, py        one division:                                   e_p   = u |p|
  dot           two products, one sum:                          e_dot = |vx| e_px + |vy| e_py + u (|vx px| + |vy py|) + u |dot|
  qx = 4 dot vx one product (the division by 1/4 is exact):      e_q   = 4 |vx| e_dot + u |qx|
  a = qx - px   one difference:                                 e_a   = e_q + e_px + u |a|          (b = qy - py alike)
  d2 = a^2 + b^2  two squares, one sum:                         e_d2  = 2 |a| e_a + 2 |b| e_b + u (a^2 + b^2) + u d2
  radius_2      exact products, one division:                   e_r2  = u radius_2
  hit           radius_2 - d2 against                           M     = SAFETY (e_d2 + e_r2)
  dti           sqrt of a difference known to within M:         [sqrt(max(diff - M, 0)) (1 - 2u), sqrt(diff + M) (1 + 2u)]
  floor argument (q_a -+ 2 dti v_a) / (2 v_a / n) = q_a n / (2 v_a) -+ n dti:  the first part to within
                SAFETY (e_q n / (2 |v_a|) + 3u |.|), the second between n times the ends of dti's interval, and 4u of both for
                the product, the difference, the divisor and the quotient; MAYBE when the two ends floor differently
  |vx| > |vy|   v = table / 2 is exact and the comparison is of two float32 numbers: no rounding, width 0
  rr cos        one division, one product:                      e_x0  = 2u |x0|;  clamp_half's >= 0.5 is near when
                | |rr cos| - 1/2 | < SAFETY e_x0; then the term's weight may also be the one of the other branch
  2n x0         one product (x0 clamped: the float32 constant, exact):  e = SAFETY (2n e_x0 + u |2n x0|); MAYBE when
                floor(arg - e) != floor(arg + e): the footprint may lie one cell to either side, which moves its edge cells only

A point is `undecided` for a lane when one of its MAYBE / near terms has a non-zero sample in that lane.  Such a point may hold
any of the `alternatives` (each MAYBE term in or out, each near term either weight).  `inconsistent` counts float32 decisions
outside what the float64 intervals allow: it must be 0, which is what proves the widths against a real float32 evaluation.

VALUE is the float64 sum of w g over the terms `sel` takes.  BOUND is the first-order forward error bound of a float32
evaluation,  sum_k |g_k| w_k (E_k + (K + 2) u)  per component (K terms: one product and at most K - 1 additions each, the
checkerboard sign is exact), with
  e_c = e_grid + e_x0 + u |c|            c = coordinate difference (grid coordinate: one division; 0 for x0 clamped)
  e_s = 2 |c0| e_c0 + 2 |c1| e_c1 + u (c0^2 + c1^2) + u s        s = c0^2 + c1^2
  E   = |coeff1| e_s + 3u |coeff1 s|  +  EXP_ULP 2u + u |coeff1 s|  +  2u
        (coeff1: a product and a division, then the product with s; the exponential; coeff0's division and the product with it).
The exponential's term is SUPPOSED, not measured and not found in the ROCm headers or documents next to the compiler: the kernel
calls __expf (a base-2 hardware exponential of x log2(e)), taken as EXP_ULP = 2 units in the last place of the result plus one
rounding of the scaled argument, |x| u."""
import ctypes
import ctypes.util
import itertools

import numpy as np

F = np.float32
U = 2.0 ** -24
SAFETY = 2.0
EXP_ULP = 2.0
PI_F = F(3.1415926535897932384626433832795)
CLAMPED = F(F(0.5) - F(1e-5))
CENTER_SIZE_MIN = 192
FLOOR_EXP = -100   # a member point has an expected weight of at least 2^-100 coeff0


def footprint(n):
    """(m, mu) as RecToolsDIRCuPy.FOURIER_INV derives them from n (methodsDIR_CuPy.py:321-322, :726-737), eps = 1e-4"""
    eps = 1e-4
    mu = -np.log(eps) / (2 * n * n)
    m = int(np.ceil(2 * n * 1 / np.pi * np.sqrt(-mu * np.log(eps) + (mu * n) * (mu * n) / 4)))
    return m, F(mu)


def libm_tables(theta):
    """cosf / sinf of the C library, the values the host code of tomo_fourier_inv computes"""
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.cosf.restype = libm.sinf.restype = ctypes.c_float
    libm.cosf.argtypes = libm.sinf.argtypes = [ctypes.c_float]
    th = np.asarray(theta, F)
    return (np.array([libm.cosf(float(t)) for t in th], F), np.array([libm.sinf(float(t)) for t in th], F))


def numpy_tables(theta):
    """the tables oracle/fourier_oracle.py computes, element by element as it does"""
    th = np.asarray(theta, F)
    return np.array([F(np.cos(t)) for t in th], F), np.array([F(np.sin(t)) for t in th], F)


def in_box(ix, iy, n, center_size):
    if center_size < CENTER_SIZE_MIN:
        return np.zeros(np.broadcast(ix, iy).shape, bool)
    base = max(0, n - center_size // 2)
    return (ix >= base) & (ix < base + center_size) & (iy >= base) & (iy < base + center_size)


def _weight(gx, gy, e_gx, e_gy, x0, y0, e_x0, e_y0, coeff1):
    """(w / coeff0, E) of a term: grid coordinates gx, gy and sample position x0, y0 in float64 with their error bounds"""
    c0, c1 = gx - x0, gy - y0
    e_c0 = e_gx + e_x0 + U * np.abs(c0)
    e_c1 = e_gy + e_y0 + U * np.abs(c1)
    s = c0 * c0 + c1 * c1
    e_s = 2 * np.abs(c0) * e_c0 + 2 * np.abs(c1) * e_c1 + U * s + U * s
    arg = coeff1 * s
    E = abs(coeff1) * e_s + 3 * U * np.abs(arg) + EXP_ULP * 2 * U + U * np.abs(arg) + 2 * U
    return np.exp(arg), E


def _sample_pos(rr32, rr64, t32, t64):
    """clamp_half(rr * t): float32 value decision, float64 position with its error, and whether the >= 0.5 is near"""
    v32 = (rr32 * t32).astype(F)
    cl32 = v32 >= F(0.5)
    v64 = rr64 * t64
    e = 2 * U * np.abs(v64)
    near = np.abs(v64 - 0.5) < SAFETY * e
    return cl32, v64, e, near


def _pos(cl, v64, e):
    return np.where(cl, float(CLAMPED), v64), np.where(cl, 0.0, e)


class Terms:
    """the terms of one geometry, ray by ray: pt = iy * 2n + ix, p, r, w (weight / coeff0 under the float32 clamp decision),
    E, sel (the float32 decisions take it), maybe (may be there or not), w2 (NaN, or the weight of the other clamp branch;
    -1: under the other branch the term is absent)"""
    FIELDS = ("pt", "p", "r", "w", "E", "sel", "maybe", "w2")

    def __init__(self, n, nproj, coeff0):
        self.n, self.nproj, self.coeff0 = n, nproj, coeff0
        self.rays = [None] * nproj
        self.inconsistent = 0



def _centre_ray(T, p, c32, s32, n, m, r2_32, coeff1, bx, by):
    """terms of ray p at the box points (bx, by: flat integer coordinates)"""
    two_n = 2 * n
    px32 = ((bx - n).astype(F) / F(two_n)).astype(F)
    py32 = ((n - by).astype(F) / F(two_n)).astype(F)
    # ---- float32 decisions
    vx, vy = F(0.5) * c32, F(0.5) * s32
    dot = (vx * px32 + vy * py32).astype(F)
    mx, my = (dot * vx / F(0.25)).astype(F), (dot * vy / F(0.25)).astype(F)
    d2 = ((mx - px32) * (mx - px32) + (my - py32) * (my - py32)).astype(F)
    hit32 = r2_32 >= d2
    dti = np.sqrt(np.maximum(r2_32 - d2, F(0)).astype(F)).astype(F)
    xdom = abs(vx) > abs(vy)
    va32, ma32 = (vx, mx) if xdom else (vy, my)
    with np.errstate(all="ignore"):
        lo32 = np.floor(((ma32 - dti * va32 / F(0.5)) / (F(2.0) * va32 / F(n))).astype(F))
        hi32 = np.floor(((ma32 + dti * va32 / F(0.5)) / (F(2.0) * va32 / F(n))).astype(F))
    rmin32 = (n // 2 - 1 + lo32).astype(np.int64)
    rmax32 = (n // 2 + 1 + hi32).astype(np.int64)
    sw = rmin32 > rmax32
    rmin32, rmax32 = np.where(sw, rmax32, rmin32), np.where(sw, rmin32, rmax32)
    rmin32, rmax32 = np.clip(rmin32, 0, n - 1), np.clip(rmax32, 0, n - 1)
    # ---- float64 intervals
    c, s = float(c32), float(s32)
    vx6, vy6 = 0.5 * c, 0.5 * s
    px, py = (bx - n) / float(two_n), (n - by) / float(two_n)
    e_px, e_py = U * np.abs(px), U * np.abs(py)
    dot6 = vx6 * px + vy6 * py
    e_dot = abs(vx6) * e_px + abs(vy6) * e_py + U * (np.abs(vx6 * px) + np.abs(vy6 * py)) + U * np.abs(dot6)
    qx, qy = 4 * dot6 * vx6, 4 * dot6 * vy6
    e_qx, e_qy = 4 * abs(vx6) * e_dot + U * np.abs(qx), 4 * abs(vy6) * e_dot + U * np.abs(qy)
    a, b = qx - px, qy - py
    e_a, e_b = e_qx + e_px + U * np.abs(a), e_qy + e_py + U * np.abs(b)
    d26 = a * a + b * b
    e_d2 = 2 * np.abs(a) * e_a + 2 * np.abs(b) * e_b + U * (a * a + b * b) + U * d26
    r2 = 2.0 * (m + 0.5) * (m + 0.5) / (4.0 * n * n)
    M = SAFETY * (e_d2 + U * r2)
    diff = r2 - d26
    can = diff >= -M
    sure = diff >= M
    T.inconsistent += int(np.count_nonzero(hit32 & ~can) + np.count_nonzero(sure & ~hit32))
    idx = np.flatnonzero(can)
    if idx.size == 0:
        return None
    diff, M, sure = diff[idx], M[idx], sure[idx]
    dlo = np.sqrt(np.maximum(diff - M, 0.0)) * (1 - 2 * U)
    dhi = np.sqrt(diff + M) * (1 + 2 * U)
    va, qa, e_qa = (vx6, qx[idx], e_qx[idx]) if xdom else (vy6, qy[idx], e_qy[idx])
    first = qa * n / (2 * va)
    e_first = SAFETY * (e_qa * n / (2 * abs(va)) + 3 * U * np.abs(first))
    e_all = SAFETY * 4 * U * (np.abs(first) + n * dhi)
    amin_lo, amin_hi = first - n * dhi - e_first - e_all, first - n * dlo + e_first + e_all
    amax_lo, amax_hi = first + n * dlo - e_first - e_all, first + n * dhi + e_first + e_all
    cl = lambda v: np.clip(v.astype(np.int64), 0, n - 1)  # noqa: E731
    rmin_lo, rmin_hi = cl(n // 2 - 1 + np.floor(amin_lo)), cl(n // 2 - 1 + np.floor(amin_hi))
    rmax_lo, rmax_hi = cl(n // 2 + 1 + np.floor(amax_lo)), cl(n // 2 + 1 + np.floor(amax_hi))
    h32, a32, b32 = hit32[idx], rmin32[idx], rmax32[idx]
    T.inconsistent += int(np.count_nonzero(h32 & ((a32 < rmin_lo) | (a32 > rmin_hi) | (b32 < rmax_lo) | (b32 > rmax_hi))))
    # ---- expand rmin_lo <= r < rmax_hi
    span = rmax_hi - rmin_lo
    k = np.arange(int(span.max()) if span.size else 0)
    rr_ = rmin_lo[:, None] + k[None, :]
    ok = k[None, :] < span[:, None]
    ii, kk = np.nonzero(ok)
    r = rr_[ii, kk]
    sel = h32[ii] & (r >= a32[ii]) & (r < b32[ii])
    certain = sure[ii] & (r >= rmin_hi[ii]) & (r < rmax_lo[ii])
    T.inconsistent += int(np.count_nonzero(certain & ~sel))
    pts = idx[ii]
    # ---- weights
    rr32 = ((r - n // 2).astype(F) / F(n)).astype(F)
    rr64 = (r - n // 2) / float(n)
    clx, x6, e_x, nearx = _sample_pos(rr32, rr64, c32, c)
    cly, y6, e_y, neary = _sample_pos(rr32, rr64, s32, s)
    x0, e_x0 = _pos(clx, x6, e_x)
    y0, e_y0 = _pos(cly, y6, e_y)
    w, E = _weight(px[pts], py[pts], e_px[pts], e_py[pts], x0, y0, e_x0, e_y0, coeff1)
    w2 = np.full(w.shape, np.nan)
    near = nearx | neary
    if near.any():
        j = np.flatnonzero(near)
        x0b, e_x0b = _pos(clx[j] ^ nearx[j], x6[j], e_x[j])
        y0b, e_y0b = _pos(cly[j] ^ neary[j], y6[j], e_y[j])
        w2[j] = _weight(px[pts[j]], py[pts[j]], e_px[pts[j]], e_py[pts[j]], x0b, y0b, e_x0b, e_y0b, coeff1)[0]
    return dict(pt=by[pts] * two_n + bx[pts], p=np.full(r.shape, p), r=r, w=w, E=E, sel=sel, maybe=~certain, w2=w2)


def _square_cells(n, m, two_n, rr32, rr64, t32, t64, flip):
    """one axis of the square form for the samples rr: per sample the cells l = e32 - m - 1 .. e32 + m + 1 with (possible,
    certain, selected) and the sample position; `flip` (bool per sample): take the other clamp branch"""
    cl32, v64, e, near = _sample_pos(rr32, rr64, t32, t64)
    cl = cl32 ^ flip
    x0, e_x0 = _pos(cl, v64, e)
    x0_32 = np.where(cl, CLAMPED, (rr32 * t32).astype(F)).astype(F)
    e32 = np.floor((F(two_n) * x0_32).astype(F)).astype(np.int64)
    A = two_n * x0
    eA = SAFETY * (two_n * e_x0 + U * np.abs(A))
    e_lo, e_hi = np.floor(A - eA).astype(np.int64), np.floor(A + eA).astype(np.int64)
    bad = int(np.count_nonzero((e32 < e_lo) | (e32 > e_hi)))
    off = np.arange(-m - 1, m + 2)
    cell = e32[:, None] + off[None, :]
    possible = (cell >= (e_lo - m)[:, None]) & (cell <= (e_hi + m)[:, None])
    certain = (cell >= (e_hi - m)[:, None]) & (cell <= (e_lo + m)[:, None])
    selected = np.broadcast_to((off >= -m) & (off <= m), cell.shape)
    return cell, possible, certain, selected, x0, e_x0, near, bad


def _square_ray(T, p, c32, s32, n, m, coeff1, center_size):
    two_n = 2 * n
    r = np.arange(n)
    rr32 = ((r - n // 2).astype(F) / F(n)).astype(F)
    rr64 = (r - n // 2) / float(n)
    c, s = float(c32), float(s32)
    none = np.zeros(n, bool)

    def enum(flipx, flipy):
        c0, p0, q0, s0, x0, e_x0, nx, b0 = _square_cells(n, m, two_n, rr32, rr64, c32, c, flipx)
        c1, p1, q1, s1, y0, e_y0, ny, b1 = _square_cells(n, m, two_n, rr32, rr64, F(-s32), -s, flipy)
        poss = p1[:, :, None] & p0[:, None, :]
        rI, i1, i0 = np.nonzero(poss)
        l0, l1 = c0[rI, i0], c1[rI, i1]
        ix, iy = (l0 + 3 * n) % two_n, (l1 + 3 * n) % two_n
        keep = ~in_box(ix, iy, n, center_size)
        rI, i1, i0, l0, l1, ix, iy = (v[keep] for v in (rI, i1, i0, l0, l1, ix, iy))
        gx, gy = l0 / float(two_n), l1 / float(two_n)
        w, E = _weight(gx, gy, U * np.abs(gx), U * np.abs(gy), x0[rI], y0[rI], e_x0[rI], e_y0[rI], coeff1)
        sel = s0[rI, i0] & s1[rI, i1]
        certain = q0[rI, i0] & q1[rI, i1]
        return dict(pt=iy * two_n + ix, r=rI, w=w, E=E, sel=sel, certain=certain), nx, ny, b0 + b1

    A, nx, ny, bad = enum(none, none)
    T.inconsistent += bad + int(np.count_nonzero(A["certain"] & ~A["sel"]))
    w2 = np.full(A["w"].shape, np.nan)
    maybe = ~A["certain"]
    out = dict(pt=A["pt"], r=A["r"], w=A["w"], E=A["E"], sel=A["sel"], maybe=maybe, w2=w2)
    near = nx | ny
    if near.any():     # the samples whose clamp is near: their terms under the other branch
        B, _, _, _ = enum(nx, ny)
        keyA = A["pt"] * n + A["r"]
        keyB = B["pt"] * n + B["r"]
        nearA, nearB = near[A["r"]], near[B["r"]]
        posB = {int(k): j for j, k in zip(np.flatnonzero(nearB), keyB[nearB])}
        seen = set()
        for j in np.flatnonzero(nearA):
            jb = posB.get(int(keyA[j]))
            seen.add(int(keyA[j]))
            if jb is None:
                w2[j] = -1.0
            else:
                w2[j] = B["w"][jb]
                if not B["certain"][jb]:
                    maybe[j] = True
        extra = [jb for k, jb in posB.items() if k not in seen]
        if extra:      # terms the other branch alone has: not selected, may be there with that branch's weight
            ex = np.array(extra)
            for k in ("pt", "r", "w", "E"):
                out[k] = np.concatenate([out[k], B[k][ex]])
            out["sel"] = np.concatenate([out["sel"], np.zeros(ex.size, bool)])
            out["maybe"] = np.concatenate([maybe, np.ones(ex.size, bool)])
            out["w2"] = np.concatenate([w2, np.full(ex.size, np.nan)])
    out["p"] = np.full(out["r"].shape, p)
    return out


def gather_terms(ct, st, n, m, mu, center_size):
    """every term of a geometry (independent of the samples' values)"""
    ct, st = np.asarray(ct, F), np.asarray(st, F)
    nproj, two_n = ct.size, 2 * n
    mu = F(mu)
    coeff0 = float(PI_F) / float(mu)
    coeff1 = -float(PI_F) * float(PI_F) / float(mu)
    T = Terms(n, nproj, coeff0)
    use_center = center_size >= CENTER_SIZE_MIN
    r2_32 = F(F(2.0) * (F(m) + F(0.5)) * (F(m) + F(0.5)) / (F(4 * n) * F(n)))
    if use_center:
        base = max(0, n - center_size // 2)
        t = base + np.arange(center_size)
        BX, BY = np.meshgrid(t, t, indexing="xy")
        bx, by = BX.ravel(), BY.ravel()
    whole = use_center and center_size == two_n
    for p in range(nproj):
        parts = []
        if use_center:
            d = _centre_ray(T, p, ct[p], st[p], n, m, r2_32, coeff1, bx, by)
            if d is not None:
                parts.append(d)
        if not whole:
            parts.append(_square_ray(T, p, ct[p], st[p], n, m, coeff1, center_size))
        if parts:
            T.rays[p] = {k: np.concatenate([d[k] for d in parts]) for k in Terms.FIELDS}
        else:
            T.rays[p] = {k: np.zeros(0, bool if k in ("sel", "maybe") else (float if k in ("w", "E", "w2") else np.int64))
                         for k in Terms.FIELDS}
    return T


class Result:
    """value [Z][2n][2n] complex128 (checkerboard sign applied), bound [Z][2n][2n][2] (real, imaginary), member and undecided
    [Z][2n][2n] bool, alternatives {(z, iy, ix): [(value, bound[2]), ...]}"""


def evaluate(T, g):
    """g: complex [nproj][n][Z], the kernel's layout.  Terms of rays whose samples are all zero in a lane are skipped."""
    g = np.asarray(g)
    nproj, n, Z = g.shape
    two_n, npt = 2 * n, 4 * n * n
    res = Result()
    value = np.zeros((Z, npt), np.complex128)
    bound = np.zeros((Z, npt, 2))
    member = np.zeros((Z, npt), bool)
    undecided = np.zeros((Z, npt), bool)
    alts = {}
    iy, ix = np.divmod(np.arange(npt), two_n)
    chk = np.where(((ix ^ iy) & 1) == 1, -1.0, 1.0)
    floor_w = 2.0 ** FLOOR_EXP
    nz_ray = np.any(g != 0, axis=1)       # [nproj][Z]
    groups = {}      # lanes by the set of their non-zero rays: the terms are put together once per set
    for z in range(Z):
        groups.setdefault(tuple(np.flatnonzero(nz_ray[:, z]).tolist()), []).append(z)
    for z, t_all in ((z, ta) for rays, zs in groups.items() if rays
                     for ta in [{k: np.concatenate([T.rays[p][k] for p in rays]) for k in Terms.FIELDS}] for z in zs):
        t = t_all
        v = g[t["p"], t["r"], z].astype(np.complex128)
        live = v != 0
        t = {k: a[live] for k, a in t.items()}
        v = v[live]
        und_t = t["maybe"] | ~np.isnan(t["w2"])
        w = t["w"] * T.coeff0
        wsel = np.where(t["sel"], w, 0.0)
        pt = t["pt"]
        value[z] = (np.bincount(pt, wsel * v.real, npt) + 1j * np.bincount(pt, wsel * v.imag, npt)) * chk
        K = np.bincount(pt, t["sel"].astype(float), npt)
        for comp, vc in enumerate((np.abs(v.real), np.abs(v.imag))):
            bound[z, :, comp] = np.bincount(pt, vc * wsel * t["E"], npt) + (K + 2) * U * np.bincount(pt, vc * wsel, npt)
        member[z] = np.bincount(pt, (t["sel"] & (t["w"] >= floor_w)).astype(float), npt) > 0
        undecided[z, pt[und_t]] = True
        uq = np.unique(pt[und_t])
        order = np.flatnonzero(np.isin(pt, uq))
        order = order[np.argsort(pt[order], kind="stable")]
        spt = pt[order]
        for q in uq:
            mine = order[np.searchsorted(spt, q, "left"):np.searchsorted(spt, q, "right")]
            at = mine[und_t[mine]]
            fixed = mine[~und_t[mine] & t["sel"][mine]]
            base_v = np.sum(w[fixed] * v[fixed])
            base_b = np.array([np.sum(np.abs(v[fixed].real) * w[fixed] * t["E"][fixed]),
                               np.sum(np.abs(v[fixed].imag) * w[fixed] * t["E"][fixed])])
            base_a = np.array([np.sum(np.abs(v[fixed].real) * w[fixed]), np.sum(np.abs(v[fixed].imag) * w[fixed])])
            kfix = int(fixed.size)
            options = []
            for j in at:
                o = [w[j]]
                if t["maybe"][j]:
                    o.append(0.0)
                if not np.isnan(t["w2"][j]):
                    o.append(0.0 if t["w2"][j] < 0 else t["w2"][j] * T.coeff0)
                options.append([(x, j) for x in dict.fromkeys(o)])
            assert len(options) <= 12, ("too many undecided terms at one point", z, int(q), len(options))
            lst = []
            for combo in itertools.product(*options):
                val, bb, aa, kk = base_v, base_b.copy(), base_a.copy(), kfix
                for x, j in combo:
                    if x != 0.0:
                        val = val + x * v[j]
                        av = np.array([abs(v[j].real), abs(v[j].imag)]) * x
                        bb += av * t["E"][j]
                        aa += av
                        kk += 1
                lst.append((val * chk[q], bb + (kk + 2) * U * aa))
            alts[(z, int(q) // two_n, int(q) % two_n)] = lst
    res.value = value.reshape(Z, two_n, two_n)
    res.bound = bound.reshape(Z, two_n, two_n, 2)
    res.member = member.reshape(Z, two_n, two_n)
    res.undecided = undecided.reshape(Z, two_n, two_n)
    res.alternatives = alts
    return res


def compare(res, got, factor, what=""):
    """the comparison both suites apply to a grid `got` [Z][2n][2n] complex: outside `undecided` membership is equal,
    non-members are exactly zero and |got - value| <= factor * bound per component; below the floor 2^FLOOR_EXP coeff0 only the
    bound is asked; inside `undecided` one of the alternatives is met.  Returns the worst |got - value| / bound outside."""
    got = np.asarray(got).astype(np.complex128)
    assert got.shape == res.value.shape, (what, got.shape, res.value.shape)
    assert np.isfinite(got.view(np.float64)).all(), (what, "not finite")
    dec = ~res.undecided
    nz = (got.real != 0) | (got.imag != 0)
    stray = dec & ~res.member & nz & (res.bound.sum(-1) == 0)
    assert not stray.any(), (what, "a point no sample reaches is not zero", np.argwhere(stray)[:5].tolist())
    lost = dec & res.member & ~nz & (np.abs(res.value) > 0)
    assert not lost.any(), (what, "a member point is zero", np.argwhere(lost)[:5].tolist())
    err = np.stack([np.abs(got.real - res.value.real), np.abs(got.imag - res.value.imag)], -1)
    tiny = np.finfo(np.float64).tiny
    ratio = np.where(dec[..., None], err / np.maximum(res.bound, tiny), 0.0)
    ratio = np.where(dec[..., None] & (err == 0), 0.0, ratio)
    bad = ratio > factor
    assert not bad.any(), (what, "beyond the bound", float(ratio.max()), np.argwhere(bad)[:5].tolist())
    for (z, iy, ix), lst in res.alternatives.items():
        gv = got[z, iy, ix]
        hit = any(abs(gv.real - val.real) <= factor * b[0] and abs(gv.imag - val.imag) <= factor * b[1] for val, b in lst)
        assert hit, (what, "an undecided point holds none of its alternatives", (z, iy, ix), gv, lst[:4])
    return float(ratio.max()) if ratio.size else 0.0


# ======================================================================================================= the cases
# grid name -> (n, center_size, what it reaches)
GRIDS = {
    "n40-c80": (40, 80, "square form only, 2n = 80 = 2.5 workgroup rows, wrap at all four edges"),
    "n96-c192": (96, 192, "centre form everywhere, at the threshold"),
    "n100-c192": (100, 192, "centre box 4 .. 195 in a 200-point grid"),
    "n100-c190": (100, 190, "below the threshold on a grid that could hold a box"),
}
# the angles of the sample impulses: unsorted, one repeated (stable order), on the boundaries the issue names, outside [-pi, pi]
SAMPLE_ANGLES = np.array([0.3, -np.pi / 4, 1e-4, -np.pi, 0.0, -np.pi / 2, 4.0, 0.3, -7.5, 2.1], F)
# which of them are PLACED ON A BOUNDARY, and the decision that sits exactly on it (exempt from the 2 % cap):
#   0      cos = 1, sin = 0: rr cos = rr and 2n x0 = 2 (r - n/2) is an integer for every sample; the floor's argument is one
#          correctly rounded product of two float32 numbers, so IEEE fixes the float32 decision -- the float64 rule cannot see it
#   1e-4   1 - 5e-9 rounds to cos = 1 in float32: the x axis as at angle 0 (sin = 1e-4 keeps the y axis off its integers)
#   -pi    cosf = -1 exactly: sample 0 has rr cos = 1/2, clamp_half acts; operands and product exact, the decision too.
#          Every other sample has 2n x0 = an integer as at angle 0
#   -pi/2  sinf = -1 exactly: the same on the y axis (y0 = -rr sin = rr)
#   -pi/4  |cos| and |sin| agree to the last place or so: the points with |kx - ky| = 11 cells lie AT the support radius
#          ((11 / sqrt 2)^2 = 60.5 = 2 (m + 1/2)^2 for m = 5), a decision no float32 evaluation is bound to
BOUNDARY_ANGLES = (0.0, float(F(1e-4)), float(F(-np.pi)), float(F(-np.pi / 2)), float(F(-np.pi / 4)))


def angle_sets():
    """name -> float32 theta as the kernel sees it"""
    lin = lambda a, b, k: np.linspace(a, b, k, endpoint=False)  # noqa: E731
    return {
        "samples": SAMPLE_ANGLES,
        "one": np.array([0.03], F),   # shallow: its outer samples leave the 192-point box of the 200-point grid
        "equal3": np.array([-1.3, -1.3, -1.3], F),
        "nine": (0.11 + lin(0, np.pi, 9)).astype(F),
        "pi65": (0.013 + lin(0, np.pi, 65)).astype(F),
        "pi130": (0.007 + lin(0, np.pi, 130)).astype(F),
        "medium97": (-(0.4 + lin(0, 1.1 * np.pi, 97))).astype(F),
        "turn24": (0.05 + lin(-np.pi, np.pi, 24)).astype(F),
    }


def sample_impulses(n, theta, seed=5):
    """64 lanes, one (p, r) each: the named radii at every angle, the rest seeded"""
    named = [0, 1, n // 2 - 1, n // 2, n // 2 + 1, n - 1]
    lanes = [(p, r) for p in range(len(theta)) for r in named][:64]
    rng = np.random.default_rng(seed)
    while len(lanes) < 64:
        pr = (int(rng.integers(len(theta))), int(rng.integers(n)))
        if pr not in lanes:
            lanes.append(pr)
    g = np.zeros((len(theta), n, 64), np.complex64)
    for z, (p, r) in enumerate(lanes):
        g[p, r, z] = 1
    return g, lanes


def ray_impulses(n, nproj):
    """ceil(nproj / 64) launches; lane z of launch k carries ray 64 k + z"""
    out = []
    for p0 in range(0, nproj, 64):
        g = np.zeros((nproj, n, 64), np.complex64)
        for z in range(min(64, nproj - p0)):
            g[p0 + z, :, z] = 1
        out.append(g)
    return out


def dense(n, nproj, zc=4, seed=11):
    rng = np.random.default_rng(seed)
    g = np.zeros((nproj, n, 64), np.complex64)
    g[:, :, :zc] = (rng.standard_normal((nproj, n, zc)) + 1j * rng.standard_normal((nproj, n, zc))).astype(np.complex64)
    return g


RAY_GRIDS = ("n96-c192", "n100-c192")
CASES = [(grid, name) for grid in GRIDS for name in angle_sets()]
CAP = 0.02


def launches(grid, setname):
    """the launches of a case: (name, g [nproj][n][64], zc, exempt) -- `exempt`: the lanes placed on a boundary (see
    BOUNDARY_ANGLES), which the 2 % cap does not cover; the dense input over the sample angles contains those rays in every lane"""
    n = GRIDS[grid][0]
    th = angle_sets()[setname]
    out = []
    if setname == "samples":
        g, lanes = sample_impulses(n, th)
        out.append(("samples", g, 64, {z for z, (p, r) in enumerate(lanes) if float(th[p]) in BOUNDARY_ANGLES}))
    elif grid in RAY_GRIDS:
        for k, g in enumerate(ray_impulses(n, len(th))):
            out.append((f"rays{k}", g, 64, set()))
    out.append(("dense", dense(n, len(th)), 4, set(range(4)) if setname == "samples" else set()))
    return out


def check_cap(res, exempt, what=""):
    """`undecided` holds at most CAP of the member points of the case and of any single lane, the exempt lanes aside"""
    Z = res.member.shape[0]
    mem = res.member.reshape(Z, -1).sum(1)
    und = (res.undecided & res.member).reshape(Z, -1).sum(1)
    keep = np.array([z not in exempt for z in range(Z)])
    assert (und[keep] <= CAP * mem[keep]).all(), (what, "a lane beyond the cap", und[keep].tolist(), mem[keep].tolist())
    assert und[keep].sum() <= CAP * mem[keep].sum(), (what, "the case beyond the cap", int(und[keep].sum()), int(mem[keep].sum()))
    return float(und[keep].sum() / max(mem[keep].sum(), 1))


def properties(grid, setname, T):
    """what the case is listed for, from the geometry"""
    n, cs, _ = GRIDS[grid]
    two_n, th = 2 * n, angle_sets()[setname]
    centre = np.concatenate([in_box(t["pt"] % two_n, t["pt"] // two_n, n, cs) for t in T.rays])
    pmask = lambda x0, iy: sum(int(in_box(np.array(x0 + q), np.array(iy), n, cs)) << q for q in range(8))  # noqa: E731
    if grid == "n40-c80":
        assert cs < CENTER_SIZE_MIN and not centre.any() and two_n % 32 == 16 and two_n // 32 == 2
    elif grid == "n96-c192":
        assert cs == CENTER_SIZE_MIN == two_n and centre.all()
    elif grid == "n100-c192":
        assert cs >= CENTER_SIZE_MIN and n - cs // 2 == 4 and centre.any() and not centre.all()
        assert pmask(0, n) == 0xf0 and pmask(192, n) == 0x0f and pmask(0, 3) == 0 and pmask(96, 196) == 0 and pmask(96, 4) == 0xff
    elif grid == "n100-c190":
        assert cs < CENTER_SIZE_MIN and n - cs // 2 > 0 and not centre.any()
    if setname == "samples":
        assert (np.diff(th) < 0).any() and len(set(th.tolist())) < th.size and (np.abs(th) > np.pi).any()
        assert all(any(float(t) == b for t in th) for b in BOUNDARY_ANGLES) and F(1e-4) in th
    elif setname == "one":
        assert th.size == 1
    elif setname == "equal3":
        assert th.size == 3 and th.min() == th.max()
    elif setname in ("pi65", "pi130"):
        assert th.size == (65 if setname == "pi65" else 130) and th.size > 64 and th.max() - th.min() < np.pi
    elif setname == "medium97":
        assert th.size == 97 and th.max() - th.min() > np.pi
    elif setname == "turn24":
        assert th.max() - th.min() > 1.9 * np.pi
