"""TEST INFRASTRUCTURE: the shapes at which the register-blocked z-march kernels (ROF_TV, PD_TV, TGV, NDF, Diff4th) can be
off by one, derived from the geometry of every launch site, and two input families that reach the branches noise never
takes.  Plain Python + numpy, no GPU import: tests/test_edge_shapes.py proves on the CPU, from the grid function restated
below, that every entry has the property it is in the table for; tests/test_gpu_edge_shapes.py runs the entries on the
MI355X.

A wave owns `c` = 64 - 2 * halo columns, a lane `r` rows, a workgroup wx x wy waves = `Wc` x `Wr` voxels of a plane; a 3D
volume is cut into z-chunks none shorter than `m` planes, every chunk but the first warmed up from the planes below its
seam.  Arrays are indexed [z][y][x]."""
import collections

import numpy as np


def ceil_div(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ the grid, restated
Grid = collections.namedtuple("Grid", "gx gy tiles_per_xcd zchunk chunks blocks")


def zmarch_grid(dx, dy, nout, tile_x, wx, wy, ry, want_per_simd, min_planes, chunked=True):
    """zmarch_grid of tomobar_amd/csrc/tv_kernels.hip (the zmarch_grid of zmarch_common.h, which NDF, Diff4th, LLT_ROF and
    TGV share, is the same function with want_per_simd = 32 and min_planes = 16 written into it; tv_kernels.hip is pinned
    by hash and keeps its own), plus the chunk count the kernels derive from blocks / (8 * tiles_per_xcd)"""
    gx = ceil_div(ceil_div(dx, tile_x), wx)
    gy = ceil_div(dy, wy * ry)
    tiles_per_xcd = ceil_div(gx * gy, 8)
    chunks = 1
    if chunked:
        waves_xy = gx * gy * wx * wy
        chunks = (256 * 4 * want_per_simd + waves_xy - 1) // waves_xy
        chunks = max(min(chunks, ceil_div(nout, min_planes)), 1)
    zchunk = ceil_div(nout, chunks)
    chunks = ceil_div(nout, zchunk)
    return Grid(gx, gy, tiles_per_xcd, zchunk, chunks, 8 * tiles_per_xcd * chunks)


def chunk_sizes(g, nout):
    return [min(g.zchunk, nout - i * g.zchunk) for i in range(g.chunks)]


def pd_plan(nd, dz, iters):
    """pd_plan of tv_kernels.hip for the shipped variants: the iterations of every launch of a prox (4 = 2 + 2, 7 = 3 + 2 + 2;
    a 3D volume of dz planes takes at most dz per launch)"""
    kmax = min(3, dz) if nd == 3 else 3
    plan, rem = [], iters
    while rem > 0:
        k = 3 if (kmax >= 3 and rem >= 3 and rem != 4) else 2 if (rem >= 2 and kmax >= 2) else 1
        plan.append(k)
        rem -= k
    return plan


# ------------------------------------------------------------------------------------------------ the launch sites
class Launch:
    """Geometry of one launch site.  `cites`: (file under tomobar_amd/csrc, text of the launch line) pairs the numbers were
    read from -- tests/test_edge_shapes.py requires every text to be in its file still.  `dims`: 2 and / or 3 (the array
    ranks that reach this launch).  `k`: PD_TV iterations per launch.  `rows2d`: one tile per wave, four waves per block, no
    z-march (pd_rows2d.inl)."""

    def __init__(self, name, op, c, wx, wy, r, m, want, dims, cites, k=None, y_halo=1, rows2d=False):
        self.name, self.op, self.c, self.wx, self.wy, self.r, self.m, self.want = name, op, c, wx, wy, r, m, want
        self.dims, self.cites, self.k, self.y_halo, self.rows2d = dims, cites, k, y_halo, rows2d
        self.Wc, self.Wr = c * wx, r * wy

    def grid(self, shape, nout=None):
        dy, dx = shape[-2:]
        if self.rows2d:
            gx, gy = ceil_div(dx, self.c), ceil_div(dy, self.r)
            return Grid(gx, gy, None, 1, 1, ceil_div(gx * gy, 4))
        nout = (shape[0] if len(shape) == 3 else 1) if nout is None else nout
        return zmarch_grid(dx, dy, nout, self.c, self.wx, self.wy, self.r, self.want, self.m, len(shape) == 3)

    def wave_columns(self, dx):
        """columns each wave of the launch emits along x (every workgroup is wx waves wide, live or not)"""
        n = ceil_div(ceil_div(dx, self.c), self.wx) * self.wx
        return [max(0, min(self.c, dx - i * self.c)) for i in range(n)]

    def wave_rows(self, dy):
        """rows each wave row of the launch emits along y"""
        n = ceil_div(dy, self.Wr) * self.wy
        return [max(0, min(self.r, dy - i * self.r)) for i in range(n)]


LAUNCHES = collections.OrderedDict((L.name, L) for L in [
    # ndf_kernels.hip:43-49 (8 rows per lane, 2 x 2 waves), ndf_zmarch.inl:132 (62 columns), zmarch_common.h:52-53 (32, 16)
    Launch("ndf", "NDF", 62, 2, 2, 8, 16, 32, (2, 3), [
        ("ndf_kernels.hip", "ndf_zmarch_launch<3, NDF_HUBER, 8, 2, 2>(a, st)"),
        ("ndf_kernels.hip", "ndf_zmarch_launch<2, NDF_TUKEY, 8, 2, 2>(a, st)"),
        ("ndf_zmarch.inl", 'zmarch_grid(g, "NDF", a.dx, a.dy, a.out_end - a.out_begin, 62, WX, WY, RY, ND == 3)'),
        ("ndf_zmarch.inl", "template <int ND, int PEN, int RY, int WX, int WY>\nstatic int ndf_zmarch_launch"),
        ("zmarch_common.h", "constexpr long want_per_simd = 32;\n    constexpr int min_planes = 16;")]),
    # diff4th_kernels.hip (8 rows per lane, 2 x 2 waves), diff4th_zmarch.inl:177 (60 columns: two halo lanes either side, two
    # halo rows above and below)
    Launch("diff4th", "Diff4th", 60, 2, 2, 8, 16, 32, (2, 3), [
        ("diff4th_kernels.hip", "d4_zmarch_launch<3, 8, 2, 2>(a, st)"),
        ("diff4th_kernels.hip", "d4_zmarch_launch<2, 8, 2, 2>(a, st)"),
        ("diff4th_zmarch.inl", 'zmarch_grid(g, "Diff4th", a.dx, a.dy, a.out_end - a.out_begin, 60, WX, WY, RY, ND == 3)'),
        ("diff4th_zmarch.inl", "template <int ND, int RY, int WX, int WY>\nstatic int d4_zmarch_launch"),
        ("zmarch_common.h", "constexpr long want_per_simd = 32;\n    constexpr int min_planes = 16;")], y_halo=2),
    # tgv_kernels.hip:41-44 (dual and primal: 4 rows per lane, 2 x 2 waves), tgv_dual.inl:139 / tgv_primal.inl:141 (63)
    Launch("tgv", "TGV", 63, 2, 2, 4, 16, 32, (2, 3), [
        ("tgv_kernels.hip", "tgv_dual_launch<3, 4, 2, 2>(a, st) : tgv_dual_launch<2, 4, 2, 2>(a, st)"),
        ("tgv_kernels.hip", "tgv_primal_launch<3, 4, 2, 2>(a, st) : tgv_primal_launch<2, 4, 2, 2>(a, st)"),
        ("tgv_dual.inl", 'zmarch_grid(g, "TGV", a.dx, a.dy, a.dz, 63, WX, WY, RY, ND == 3)'),
        ("tgv_primal.inl", 'zmarch_grid(g, "TGV", a.dx, a.dy, a.dz, 63, WX, WY, RY, ND == 3)'),
        ("tgv_dual.inl", "template <int ND, int RY, int WX, int WY>\nstatic int tgv_dual_launch"),
        ("tgv_primal.inl", "template <int ND, int RY, int WX, int WY>\nstatic int tgv_primal_launch"),
        ("zmarch_common.h", "constexpr long want_per_simd = 32;\n    constexpr int min_planes = 16;")]),
    # tv_kernels.hip:763 (8 rows per lane, 2 x 2 waves), rof_zmarch.inl:253 (60 columns, 32 waves per SIMD, chunks >= 32)
    Launch("rof", "ROF_TV", 60, 2, 2, 8, 32, 32, (2, 3), [
        ("tv_kernels.hip", "return rof_zmarch_launch<ND, HALF, 3, 8, 2, 2>(a, st);"),
        ("rof_zmarch.inl", "template <int ND, bool HALF, int FAST, int RY, int WX, int WY>\nstatic int rof_zmarch_launch"),
        ("rof_zmarch.inl", 'zmarch_grid(g, "ROF_TV", a.dx, a.dy, a.out_end - a.out_begin, 60, WX, WY, RY, 32, 32, ND == 3)')]),
    # tv_kernels.hip:573-583: BOTH dual types of the shipped library run K = 3 at 8 rows per lane, 2 x 2 waves (the 4-row
    # instantiation of binary16 duals at :566 is the compiler-IEEE build of the dev flavour only); pd_zmarch_xk.inl:428-431
    # (64 - 2K = 58 columns, chunks >= 24 K = 72)
    Launch("pd_xk3", "PD_TV", 58, 2, 2, 8, 72, 32, (3,), [
        ("tv_kernels.hip", "pd_zmarch_xk_launch<T, NN, AN, 2, 3, 8, 2, 2, true, 10, true>(a, st) : pd_zmarch_xk_launch<T, NN, AN, 2, 3, 8, 2, 2, true, 10>(a, st)"),
        ("tv_kernels.hip", "pd_zmarch_xk_launch<T, true, AN, 1, 3, 8, 2, 2, true, 10, true>(b, st) : pd_zmarch_xk_launch<T, true, AN, 1, 3, 8, 2, 2, true, 10>(b, st)"),
        ("pd_zmarch_xk.inl", "template <typename T, bool NONNEG, bool ANISO, int FAST, int K, int RY, int WX, int WY, bool LAG = false, int LREG = 0, bool FIRST = false>\nstatic int pd_zmarch_xk_launch(PdArgs a, hipStream_t st, long want_per_simd = 32, int min_chunk = 24)"),
        ("pd_zmarch_xk.inl", 'zmarch_grid(g, "PD_TV", a.dx, a.dy, a.out_end - a.out_begin, 64 - 2 * K, WX, WY, RY, want_per_simd, min_chunk * K)')], k=3),
    # tv_kernels.hip:599: 4 rows per lane, 2 waves in x, 4 in y with relaxed arithmetic (float32 duals of the default), else 2;
    # pd_zmarch_x2.inl:205 (60 columns, chunks >= 48)
    Launch("pd_x2_relaxed", "PD_TV", 60, 2, 4, 4, 48, 32, (3,), [
        ("tv_kernels.hip", "pd_zmarch_x2_launch<T, NN, AN, decltype(f)::value, 4, 2, decltype(f)::value == 1 ? 4 : 2>(a, st)"),
        ("pd_zmarch_x2.inl", "template <typename T, bool NONNEG, bool ANISO, int FAST, int RY, int WX, int WY>\nstatic int pd_zmarch_x2_launch"),
        ("pd_zmarch_x2.inl", 'zmarch_grid(g, "PD_TV", a.dx, a.dy, a.out_end - a.out_begin, 60, WX, WY, RY, 32, 48)')], k=2),
    Launch("pd_x2_exact", "PD_TV", 60, 2, 2, 4, 48, 32, (3,), [
        ("tv_kernels.hip", "pd_zmarch_x2_launch<T, NN, AN, decltype(f)::value, 4, 2, decltype(f)::value == 1 ? 4 : 2>(a, st)"),
        ("pd_zmarch_x2.inl", 'zmarch_grid(g, "PD_TV", a.dx, a.dy, a.out_end - a.out_begin, 60, WX, WY, RY, 32, 48)')], k=2),
    # tv_kernels.hip:612: 8 rows per lane, 4 x 2 waves; pd_zmarch2.inl:146 (62 columns, 48 waves per SIMD, chunks >= 32)
    Launch("pd_single", "PD_TV", 62, 4, 2, 8, 32, 48, (3,), [
        ("tv_kernels.hip", "pd_zmarch2_launch<T, 3, NN, AN, F, 8, true, 4, 2>(a, st)"),
        ("pd_zmarch2.inl", "template <typename T, int ND, bool NONNEG, bool ANISO, int FAST, int RY, bool LOCKSTEP, int WX = 1, int WY = 4>\nstatic int pd_zmarch2_launch"),
        ("pd_zmarch2.inl", 'zmarch_grid(g, "PD_TV", a.dx, a.dy, a.out_end - a.out_begin, 62, WX, WY, RY, 48, 32, ND == 3)')], k=1),
] + [
    # tv_kernels.hip:603-605 (K = 3, 2, 1 at 8 rows), pd_rows2d.inl:102-106 (64 - 2K columns, (tiles + 3) / 4 blocks of 256)
    Launch(f"pd_rows2d_k{k}", "PD_TV", 64 - 2 * k, 1, 1, 8, None, None, (2,), [
        ("tv_kernels.hip", f"pd_rows2d_launch<T, NN, AN, F, {k}, 8>(a, st)"),
        ("pd_rows2d.inl", "const int gx = ceil_div(a.dx, 64 - 2 * K), gy = ceil_div(a.dy, RY);"),
        ("pd_rows2d.inl", "<<<(unsigned)((tiles + 3) / 4), 256, 0, st>>>"),
        ("pd_rows2d.inl", "const int tile = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);")], k=k, rows2d=True)
    for k in (1, 2, 3)
])


# ------------------------------------------------------------------------------------------------ the properties
def _first(n, *head):
    """[head..., 0, 0, ...] of length n"""
    return list(head) + [0] * (n - len(head))


def _x_props(L):
    c, wx = L.c, L.wx
    cols = L.wave_columns
    p = collections.OrderedDict()
    p["x: the array ends one column before the first wave's last emitting lane"] = lambda s: cols(s[-1]) == _first(wx, c - 1)
    p["x: the array ends on the first wave's last emitting lane"] = lambda s: cols(s[-1]) == _first(wx, c)
    p["x: the last wave has one column"] = lambda s: cols(s[-1]) == _first(max(wx, 2), c, 1)
    p["x: the array ends one column before the workgroup's last"] = lambda s: cols(s[-1]) == [c] * (wx - 1) + [c - 1]
    p["x: the array ends on the workgroup's last column"] = lambda s: cols(s[-1]) == [c] * wx
    p["x: the second workgroup has one column"] = lambda s: cols(s[-1]) == [c] * wx + _first(wx, 1)
    for w in range(2, wx):   # the ragged inner waves of a workgroup more than two waves wide
        p[f"x: wave {w} of the workgroup lacks its last column"] = lambda s, w=w: cols(s[-1]) == _first(wx, *([c] * (w - 1) + [c - 1]))
        p[f"x: wave {w + 1} of the workgroup has one column"] = lambda s, w=w: cols(s[-1]) == _first(wx, *([c] * w + [1]))
    if L.rows2d:
        p["x: one live wave in the last block"] = lambda s: (L.grid(s).gx * L.grid(s).gy) % 4 == 1 and L.grid(s).blocks > 1
    return p


def _y_props(L):
    r, wy = L.r, L.wy
    rows = L.wave_rows
    p = collections.OrderedDict()
    p["y: the array ends one row before a lane's last row"] = lambda s: rows(s[-2]) == _first(wy, r - 1)
    p["y: the last row of a lane is the array's last"] = lambda s: rows(s[-2]) == _first(wy, r)
    p["y: the last wave row has one row"] = lambda s: rows(s[-2]) == _first(max(wy, 2), r, 1)
    p["y: the array ends one row before the workgroup's last"] = lambda s: rows(s[-2]) == [r] * (wy - 1) + [r - 1]
    p["y: the array ends on the workgroup's last row"] = lambda s: rows(s[-2]) == [r] * wy
    p["y: the second workgroup has one row"] = lambda s: rows(s[-2]) == [r] * wy + _first(wy, 1)
    if L.y_halo == 2:
        p["y: both neighbours two rows away clamp onto the tile"] = lambda s: any(y - 2 < 0 and y + 2 > s[-2] - 1 for y in range(s[-2]))
    return p


PD_THIN_PLANS = {1: [1] * 7, 2: [2, 2, 2, 1], 3: [3, 2, 2], 4: [3, 2, 2]}   # a prox of 7 iterations on dz planes


def _z_props(L):
    m = L.m
    sizes = lambda s: chunk_sizes(L.grid(s), s[0])  # noqa: E731
    p = collections.OrderedDict()
    p["z: one chunk, one plane short of the shortest chunk"] = lambda s: s[0] == m - 1 and sizes(s) == [m - 1]
    p["z: one chunk of the shortest length"] = lambda s: sizes(s) == [m]
    p["z: the first split, two chunks of m/2 + 1 and m/2"] = lambda s: sizes(s) == [ceil_div(m + 1, 2), (m + 1) // 2] and s[0] == m + 1
    p["z: two chunks of m and m - 1"] = lambda s: sizes(s) == [m, m - 1]
    p["z: two chunks of the shortest length"] = lambda s: sizes(s) == [m, m]
    p["z: three chunks"] = lambda s: s[0] == 2 * m + 1 and len(sizes(s)) == 3 and L.grid(s).tiles_per_xcd == 1
    p["z: four chunks"] = lambda s: s[0] == 3 * m + 1 and len(sizes(s)) == 4
    p["z: 9 xy tiles, tiles_per_xcd = 2, seven dead workgroups in each of three chunks"] = lambda s: (
        L.grid(s).gx * L.grid(s).gy == 9 and L.grid(s).tiles_per_xcd == 2 and L.grid(s).chunks == 3 and L.grid(s).blocks == 48)
    if L.k is not None:
        for dz in sorted({1, 2, 3, L.k, L.k + 1}):
            p[f"z: a thin volume of {dz} planes, 7 iterations = {'+'.join(map(str, PD_THIN_PLANS[dz]))}"] = (
                lambda s, dz=dz: s[0] == dz and pd_plan(3, dz, 7) == PD_THIN_PLANS[dz] and L.grid(s).chunks == 1)
    return p


def properties(L, group):
    """{property: predicate(shape)} every launch must realise in `group` ("x", "y" or "z"; rows2d has no z)"""
    if group == "z" and L.rows2d:
        return {}
    return {"x": _x_props, "y": _y_props, "z": _z_props}[group](L)


# ------------------------------------------------------------------------------------------------ the table
Case = collections.namedtuple("Case", "launch group shape claims")


def _cases_of(L):
    c, r, m, Wc, Wr = L.c, L.r, L.m, L.Wc, L.Wr
    xs = list(zip(_x_props(L), (c - 1, c, c + 1, Wc - 1, Wc, Wc + 1)))
    for w in range(2, L.wx):
        xs += [(f"x: wave {w} of the workgroup lacks its last column", w * c - 1),
               (f"x: wave {w + 1} of the workgroup has one column", w * c + 1)]
    ys = list(zip(_y_props(L), (r - 1, r, r + 1, Wr - 1, Wr, Wr + 1)))
    out = []
    for nd in L.dims:
        lead = (3,) if nd == 3 else ()
        for claim, dx in xs:
            out.append(("x", lead + (r + 1, dx), claim))
        for claim, dy in ys:
            out.append(("y", lead + (dy, c + 1), claim))
        if L.y_halo == 2:
            for dy in (2, 3):
                out.append(("y", lead + (dy, c), "y: both neighbours two rows away clamp onto the tile"))
    if L.rows2d:
        out.append(("x", (r, 4 * c + 1), "x: one live wave in the last block"))   # 5 tiles in one row of tiles
    else:
        zp = list(_z_props(L))
        for claim, dz in zip(zp, (m - 1, m, m + 1, 2 * m - 1, 2 * m, 2 * m + 1, 3 * m + 1)):
            out.append(("z", (dz, 9, 11), claim))
        # nine workgroups side by side; ROF_TV needs two rows (reflecting boundary), one is enough for the others
        out.append(("z", (2 * m + 1, 2 if L.op == "ROF_TV" else 1, 8 * Wc + 1), zp[7]))
        if L.k is not None:
            for dz in sorted({1, 2, 3, L.k, L.k + 1}):
                out.append(("z", (dz, 9, 11), f"z: a thin volume of {dz} planes, 7 iterations = {'+'.join(map(str, PD_THIN_PLANS[dz]))}"))
    # one entry per (group, shape): shapes that coincide (one wave per workgroup) carry every claim made for them
    merged = collections.OrderedDict()
    for group, shape, claim in out:
        merged.setdefault((group, shape), []).append(claim)
    return [Case(L.name, group, shape, tuple(claims)) for (group, shape), claims in merged.items()]


CASES = [case for L in LAUNCHES.values() for case in _cases_of(L)]
GROUPS = ("x", "y", "z")


def cases(launch, group=None, nd=None):
    return [k for k in CASES if k.launch == launch and group in (None, k.group) and nd in (None, len(k.shape))]


def groups_of(launch):
    return [g for g in GROUPS if cases(launch, g)]


# ------------------------------------------------------------------------------------------------ chunked z-slabs
# Two ranks, 2 m + 1 local planes each: a slab launch over all local planes is three chunks, the first of which starts at
# out_begin = the ghost planes below (rank 1); in the "ranges" schedule the boundary ranges are `boundary` planes below /
# above an interior boundary and the interior launch, which starts past them, is still chunked.  `ghost`: planes below /
# above (tomobar_amd/slab.py: NdfSlab, Diff4thSlab, RofSlab, PdSlab).  PD_TV slab launches: K = 3 and K = 2 over ranges
# (tomo_pdtv_multi_slab_range), the single iteration over all local planes (tomo_pdtv_iter_slab).
Slab = collections.namedtuple("Slab", "shape world launches ghost boundary")
SLABS = {
    "NDF": Slab((66, 9, 11), 2, ("ndf",), (1, 1), (1, 1)),
    "Diff4th": Slab((66, 9, 11), 2, ("diff4th",), (2, 2), (2, 2)),
    "ROF_TV": Slab((130, 9, 11), 2, ("rof",), (2, 1), (1, 2)),
    "PD_TV": Slab((290, 9, 11), 2, ("pd_xk3",), (3, 3), (3, 3)),
}


def slab_launch_chunks(op, schedule):
    """chunk sizes of the largest launch of every rank under `schedule` ("plain": all local planes; "ranges": the interior),
    from the restated grid"""
    s = SLABS[op]
    L = LAUNCHES[s.launches[0]]
    nz, dy, dx = s.shape
    out = []
    for rank in range(s.world):
        nzl = nz // s.world + (1 if rank < nz % s.world else 0)
        nout = nzl
        if schedule == "ranges":
            nout -= (s.boundary[0] if rank > 0 else 0) + (s.boundary[1] if rank < s.world - 1 else 0)
        out.append(chunk_sizes(L.grid((nout, dy, dx), nout), nout))
    return out


# ------------------------------------------------------------------------------------------------ input families
def terraces(shape, block=8, scale=1.0):
    """piecewise-constant blocks with integer levels 3 ((x // block + 2 (y // block) + 3 (z // block)) mod 5) - 6, times
    `scale`: the values -6, -3, 0, 3, 6 -- zero, negative values and exact ties between neighbours (most forward
    differences are exactly zero)"""
    idx = np.indices(shape)
    level = sum(w * (i // block) for w, i in zip((1, 2, 3), idx[::-1]))
    return np.ascontiguousarray(((3 * (level % 5) - 6) * scale).astype(np.float32))


def step_noise(shape, seed=5):
    """the noise-on-a-step input of test_pdtv_vs_oracle / test_roftv_vs_oracle (tests/test_gpu_parity.py)"""
    rng = np.random.default_rng(seed)
    return (rng.random(shape) * 0.3 + (np.indices(shape)[-1] > shape[-1] // 2)).astype(np.float32)


SCALE_EXPONENTS = (-14, 10)


def scaled(x, e):
    """x * 2**e, exact in float32 (no value of the inputs used leaves the normal range)"""
    return np.ascontiguousarray(np.ldexp(np.asarray(x, np.float32), e).astype(np.float32))


def zero_share(x):
    """share of the forward differences (neighbour present) of x that are exactly zero"""
    zero = total = 0
    for ax in range(x.ndim):
        d = np.diff(x, axis=ax)
        zero += int(np.count_nonzero(d == 0))
        total += d.size
    return zero / max(total, 1)
