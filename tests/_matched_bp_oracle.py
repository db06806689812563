"""TEST INFRASTRUCTURE: numpy restatement of the matched back projector (include/tomo_mi355x.h, tomo_bp3d_matched;
docs/kernels/bp_matched.md) -- the exact transpose of the Joseph forward projector of oracle/tomo_oracle.c (orc_fp3d).

Two forms.  The float32 one reproduces the kernel's rounding sequence: every operation rounds once to float32, fmaf is an
exact float64 product, a float64 sum brought to round-to-odd, and one rounding to float32 (so no double rounding).  The
float64 one is the same formula without the float32 roundings, beside a float64 restatement of orc_fp3d, for the dense
transpose check.  Angle records are built the way orc_make_angles builds them.  There is no reference counterpart:
parity is formula-level, unpinned."""
import numpy as np

from oracle import tomo_oracle as O

F32 = np.float32


def fmaf(a, b, c):
    """float32 fma(a, b, c) with ONE rounding.  The product of two float32 is exact in float64; the float64 sum is turned
    into round-to-odd with the TwoSum error term, after which the rounding to float32 is the rounding of the exact value."""
    p = np.asarray(a, F32).astype(np.float64) * np.asarray(b, F32).astype(np.float64)
    c = np.asarray(c, F32).astype(np.float64)
    p, c = np.broadcast_arrays(p, c)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
    fix = (err != 0) & even & np.isfinite(s)
    s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


def angle_table(angles, cor=0.0, index=None):
    """(cs, sn, cor, scale) float32 arrays per selected angle, as orc_make_angles: float32 of the float64 cosine / sine, and
    scale = float32(1 / |sin|) where |sin| >= |cos| (x-stepping), float32(1 / |cos|) otherwise."""
    th = np.asarray(angles, np.float64).ravel()
    c_all = np.asarray(cor, np.float64)
    c_all = np.full(th.size, float(c_all)) if c_all.ndim == 0 else (c_all if c_all.ndim == 1 else c_all[:, 0])
    idx = np.arange(th.size) if index is None else np.asarray(index, np.int64)
    c, s = np.cos(th[idx]), np.sin(th[idx])
    dirx = np.abs(s) >= np.abs(c)
    scale = np.where(dirx, 1.0 / np.abs(np.where(dirx, s, 1.0)), 1.0 / np.abs(np.where(dirx, 1.0, c)))
    return {"cs": c.astype(F32), "sn": s.astype(F32), "cor": c_all[idx].astype(F32), "scale": scale.astype(F32)}


def table_of(P, subset=None):
    """The same record fields read from an oracle Projector's C-built table (tests compare the two)."""
    tab, nsel = P._sel(subset)
    rec = np.frombuffer(tab, dtype=np.dtype([("cs", "f4"), ("sn", "f4"), ("cor", "f4"), ("slope", "f4"), ("inv", "f4"),
                                             ("scale", "f4"), ("dirx", "i4"), ("src", "i4")]), count=nsel)
    return {k: rec[k].copy() for k in ("cs", "sn", "cor", "scale")}


def taps32(n, nu, tab, a, matched=True):
    """(i0, w0, w1) of every voxel (iy, ix) for angle slot `a`: the specification, one float32 rounding per operation."""
    half_n = F32(0.5) * F32(n) - F32(0.5)
    half_u = F32(0.5) * F32(nu) - F32(0.5)
    xw = (np.arange(n, dtype=F32) - half_n)[None, :]
    yw = (np.arange(n, dtype=F32) - half_n)[:, None]
    cs, sn, q = tab["cs"][a], tab["sn"][a], tab["scale"][a]
    off = F32(half_u - tab["cor"][a])
    f = fmaf(xw, cs, fmaf(yw, sn, off))
    fl = np.floor(f)
    w = (f - fl).astype(F32)
    one, zero = F32(1.0), F32(0.0)
    if matched:
        w0 = np.maximum(one - w * q, zero) * q
        w1 = np.maximum(one - (one - w) * q, zero) * q
    else:
        w0, w1 = one - w, w
    return fl.astype(np.int64), w0.astype(F32), w1.astype(F32)


def bp32(sino, n, tab, matched=True):
    """sino [nz][na][nu] float32 -> vol [nz][n][n] float32; angles ascending, tap 0 then tap 1, fmaf.  matched=False is the
    shipped (voxel-driven bilinear) projector, orc_bp3d, in the same arithmetic."""
    sino = np.ascontiguousarray(sino, F32)
    nz, na, nu = sino.shape
    assert na == len(tab["cs"]), (na, len(tab["cs"]))
    acc = np.zeros((nz, n, n), F32)
    for a in range(na):
        i0, w0, w1 = taps32(n, nu, tab, a, matched)
        row = sino[:, a, :]
        s0 = np.where(((i0 >= 0) & (i0 < nu))[None], row[:, np.clip(i0, 0, nu - 1)], F32(0))
        s1 = np.where(((i0 + 1 >= 0) & (i0 + 1 < nu))[None], row[:, np.clip(i0 + 1, 0, nu - 1)], F32(0))
        acc = fmaf(w0[None], s0, acc)
        acc = fmaf(w1[None], s1, acc)
    return acc


class MatchedProjector(O.Projector):
    """The oracle's operator pair with `bp` replaced by the float32 restatement of A^T: the outer loops of
    oracle/tomo_oracle.py (fista, admm, osem, power_method) and the loops retyped in the tests run on it unchanged."""

    def bp(self, sino, subset=None):
        sino = np.ascontiguousarray(sino, dtype=F32)
        if self.vshift is not None:
            sino = np.ascontiguousarray(self.shift_rows(sino, subset, -1.0))
        return bp32(sino, self.n, table_of(self, subset), matched=True)


# ------------------------------------------------------------------ float64 forms (dense transpose check)
def fp_matrix64(n, nu, angles, cor):
    """Dense [na * nu, n * n] float64 matrix of the Joseph forward projector: orc_fp3d restated in float64, one slice."""
    th = np.asarray(angles, np.float64)
    half_n, half_u = 0.5 * n - 0.5, 0.5 * nu - 0.5
    A = np.zeros((th.size * nu, n * n))
    for a, t in enumerate(th):
        c, s = np.cos(t), np.sin(t)
        dirx = abs(s) >= abs(c)
        slope, inv, scale = (-c / s, 1.0 / s, 1.0 / abs(s)) if dirx else (-s / c, 1.0 / c, 1.0 / abs(c))
        for iu in range(nu):
            offset = ((iu - half_u) + cor) * inv + half_n
            for k in range(n):
                f = (k - half_n) * slope + offset
                fl = np.floor(f)
                w, i0 = f - fl, int(fl)
                for i, wt in ((i0, 1.0 - w), (i0 + 1, w)):
                    if 0 <= i < n:
                        A[a * nu + iu, (i * n + k) if dirx else (k * n + i)] += wt * scale
    return A


def bp_matrix64(n, nu, angles, cor, matched=True):
    """Dense [n * n, na * nu] float64 matrix of the back projector of the specification (matched) or the shipped one."""
    th = np.asarray(angles, np.float64)
    half_n, half_u = 0.5 * n - 0.5, 0.5 * nu - 0.5
    B = np.zeros((n * n, th.size * nu))
    for a, t in enumerate(th):
        c, s = np.cos(t), np.sin(t)
        q = 1.0 / max(abs(s), abs(c))
        for iy in range(n):
            for ix in range(n):
                f = (ix - half_n) * c + ((iy - half_n) * s + (half_u - cor))
                fl = np.floor(f)
                w, i0 = f - fl, int(fl)
                w0, w1 = (max(1.0 - w * q, 0.0) * q, max(1.0 - (1.0 - w) * q, 0.0) * q) if matched else (1.0 - w, w)
                for i, wt in ((i0, w0), (i0 + 1, w1)):
                    if 0 <= i < nu:
                        B[iy * n + ix, a * nu + i] += wt
    return B


# ------------------------------------------------------------------ the adjoint gap
def normalised_gap(ax, y, x, bty):
    """|<Ax, y> - <x, B y>| / (||Ax||_2 ||y||_2), sums in float64."""
    ax, y, x, bty = (np.asarray(v, np.float64).ravel() for v in (ax, y, x, bty))
    return abs(ax @ y - x @ bty) / (np.linalg.norm(ax) * np.linalg.norm(y))


SPECIAL_ANGLES = (0.0, np.pi / 4, np.pi / 2, 3 * np.pi / 4, np.pi, -0.3, 5.5)


def gap_family(count=60, seed=2024):
    """`count` seeded geometries (n, nu, cor, angles): n in 3 .. 39, nu in n - 8 .. n + 11 (at least 2 pixels), CoR in
    +-3, angle sets that hold 0, pi/4 (the tie), pi/2, 3pi/4, pi, a negative angle and angles beyond pi."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        n = int(rng.integers(3, 40))
        nu = max(2, int(rng.integers(n - 8, n + 12)))
        cor = float(rng.uniform(-3.0, 3.0))
        extra = rng.uniform(-1.0, 2.0 * np.pi, size=int(rng.integers(3, 9)))
        out.append((n, nu, cor, np.concatenate([np.asarray(SPECIAL_ANGLES), extra])))
    return out
