"""TEST INFRASTRUCTURE: the edge shapes of the LLT_ROF z-march launch, derived with the unchanged machinery of
tests/_edge_shapes.py (its table is left as it is: this module builds one more `Launch` and its cases beside it).  Plain
Python + numpy, no GPU import: tests/test_llt_rof_edge_shapes.py proves on the CPU that every entry has the property it is
listed for; tests/test_gpu_llt_rof_edges.py runs the entries on the MI355X."""
from _edge_shapes import (GROUPS, SCALE_EXPONENTS, Launch, Slab, _cases_of, chunk_sizes, properties, scaled,  # noqa: F401
                          terraces, zero_share)

# llt_rof_kernels.hip (8 rows per lane, 2 x 2 waves), llt_rof_zmarch.inl (60 columns: two halo lanes either side, two halo
# rows above and below for E2), zmarch_common.h (32 waves per SIMD wanted, no chunk shorter than 16 planes)
LAUNCH = Launch("llt_rof", "LLT_ROF", 60, 2, 2, 8, 16, 32, (2, 3), [
    ("llt_rof_kernels.hip", "lr_zmarch_launch<3, 8, 2, 2>(a, st)"),
    ("llt_rof_kernels.hip", "lr_zmarch_launch<2, 8, 2, 2>(a, st)"),
    ("llt_rof_zmarch.inl", 'zmarch_grid(g, "LLT_ROF", a.dx, a.dy, a.out_end - a.out_begin, 60, WX, WY, RY, ND == 3)'),
    ("llt_rof_zmarch.inl", "template <int ND, int RY, int WX, int WY>\nstatic int lr_zmarch_launch"),
    ("zmarch_common.h", "constexpr long want_per_simd = 32;\n    constexpr int min_planes = 16;")], y_halo=2)

CASES = _cases_of(LAUNCH)


def cases(group=None, nd=None):
    return [k for k in CASES if group in (None, k.group) and nd in (None, len(k.shape))]


def groups():
    return [g for g in GROUPS if cases(g)]


# Two ranks, 2 m + 1 = 33 local planes each (tests/_edge_shapes.py, "chunked z-slabs"): two ghost planes below / above, two
# boundary planes below / above an interior boundary (tomobar_amd/slab.py: LltRofSlab)
SLAB = Slab((66, 9, 11), 2, ("llt_rof",), (2, 2), (2, 2))


def slab_launch_chunks(schedule):
    """chunk sizes of the largest launch of every rank under `schedule` ("plain": all local planes; "ranges": the interior),
    from the restated grid (slab_launch_chunks of tests/_edge_shapes.py for this launch)"""
    nz, dy, dx = SLAB.shape
    out = []
    for rank in range(SLAB.world):
        nzl = nz // SLAB.world + (1 if rank < nz % SLAB.world else 0)
        nout = nzl
        if schedule == "ranges":
            nout -= (SLAB.boundary[0] if rank > 0 else 0) + (SLAB.boundary[1] if rank < SLAB.world - 1 else 0)
        out.append(chunk_sizes(LAUNCH.grid((nout, dy, dx), nout), nout))
    return out


TERRACE_SHAPES = [(20, 24, 70), (40, 130)]


def terrace_shapes():
    """every shape the GPU tests run `terraces` on"""
    seen = []
    for case in CASES:
        if case.shape not in seen:
            seen.append(case.shape)
    return seen + TERRACE_SHAPES + [SLAB.shape]
