"""CPU tests of tests/_llt_rof_edge_shapes.py, as tests/test_edge_shapes.py has them for the other z-march launches: the
table of LLT_ROF edge shapes has the properties it claims under the restated grid, every property is realised, the geometry
is still what the launch lines say, the slab entry is z-chunked, and `terraces` reaches -- on the numpy oracle alone -- the
exact-zero quotients 0 / sqrt(eps) and 0 / (0 + eps)."""
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _edge_shapes as E  # noqa: E402
import _llt_rof_edge_shapes as LE  # noqa: E402
from _llt_rof_oracle import ORACLE as D  # noqa: E402
from _tgv_oracle import phantom  # noqa: E402

CSRC = os.path.join(ROOT, "tomobar_amd", "csrc")


def test_geometry_is_what_the_launch_lines_say():
    for fname, text in LE.LAUNCH.cites:
        with open(os.path.join(CSRC, fname)) as fh:
            assert text in fh.read(), (fname, text)


def test_the_shared_table_is_untouched():
    assert "llt_rof" not in E.LAUNCHES and "LLT_ROF" not in E.SLABS
    assert not any(c.launch == "llt_rof" for c in E.CASES)


def test_grid_restatement_on_a_known_launch():
    """(40, 150, 200) is three chunks of 14, 14 and 12 planes on 2 x 10 workgroup tiles (tests/test_gpu_llt_rof.py)"""
    g = LE.LAUNCH.grid((40, 150, 200))
    assert (g.gx, g.gy) == (2, 10) and E.chunk_sizes(g, 40) == [14, 14, 12] and g.blocks == 8 * 3 * 3
    g = LE.LAUNCH.grid((150, 200))
    assert g.chunks == 1 and g.zchunk == 1


def test_every_entry_has_the_property_it_claims():
    L = LE.LAUNCH
    assert LE.CASES
    for case in LE.CASES:
        props = LE.properties(L, case.group)
        assert case.claims and len(case.shape) in L.dims, case
        for claim in case.claims:
            assert props[claim](case.shape), (case, L.grid(case.shape), L.wave_columns(case.shape[-1]), L.wave_rows(case.shape[-2]))
        assert int(np.prod(case.shape)) <= 300_000, case


def test_every_property_is_claimed_by_an_entry():
    L = LE.LAUNCH
    for group in LE.GROUPS:
        for nd in L.dims:
            if group == "z" and nd == 2:
                continue
            claimed = {c for case in LE.cases(group, nd) for c in case.claims}
            missing = [p for p in LE.properties(L, group) if p not in claimed]
            assert not missing, (group, nd, missing)
    assert LE.groups() == ["x", "y", "z"]


def test_the_table_holds_the_shapes_the_geometry_gives():
    shapes = lambda group, nd=None: [c.shape for c in LE.cases(group, nd)]  # noqa: E731
    assert shapes("x", 3) == [(3, 9, d) for d in (59, 60, 61, 119, 120, 121)]
    assert shapes("x", 2) == [(9, d) for d in (59, 60, 61, 119, 120, 121)]
    assert shapes("y", 3) == [(3, d, 61) for d in (7, 8, 9, 15, 16, 17)] + [(3, 2, 60), (3, 3, 60)]
    assert shapes("z") == [(d, 9, 11) for d in (15, 16, 17, 31, 32, 33, 49)] + [(33, 1, 961)]
    # the same geometry as Diff4th's launch: the same shapes
    assert [c.shape for c in LE.CASES] == [c.shape for c in E.cases("diff4th")]


def test_the_slab_shape_is_chunked_on_every_launch():
    from tomobar_amd import slab as S
    s, L = LE.SLAB, LE.LAUNCH
    nzl = s.shape[0] // s.world
    assert s.shape[0] % s.world == 0 and nzl == 2 * L.m + 1
    plain = LE.slab_launch_chunks("plain")
    assert all(len(sizes) == 3 for sizes in plain), plain
    interior = LE.slab_launch_chunks("ranges")
    assert all(len(sizes) >= 2 for sizes in interior), interior
    for rank in range(s.world):
        lo, hi = rank > 0, rank < s.world - 1
        me = types.SimpleNamespace(nzl=nzl, has_lo=lo, has_hi=hi, lo=s.ghost[0] if lo else 0, hi=s.ghost[1] if hi else 0)
        edges, (b0, b1) = S.LltRofSlab.boundary_ranges(me)
        assert (b0, nzl - b1) == (s.boundary[0] if lo else 0, s.boundary[1] if hi else 0), (rank, edges, b0, b1)
        assert all(1 <= z1 - z0 <= 3 for z0, z1 in edges) and sum(interior[rank]) == b1 - b0
    assert S.LLT_ROF_GHOST == s.ghost[0] == s.ghost[1]


def test_terraces_reach_the_exact_zero_quotients_at_every_shape_used():
    """s == 0 (R_d = 0 / sqrt(eps)) on at least a quarter -- and fewer than all -- of the voxels entering the first
    iteration at every shape `terraces` is run on, and |h1| < 1e-6 (E_1 = 0 / (0 + eps)) likewise; the noise input all but
    never gets there"""
    for shape in LE.terrace_shapes():
        stats = {}
        out = D.run(LE.terraces(shape), iterations=2, stats=stats, **D.PARAMS["A"])
        assert np.all(np.isfinite(out)), shape
        assert 0.25 <= stats["s_zero", 1] < 1.0, (shape, stats)
        assert 0.25 <= stats["h1_tiny", 1], (shape, stats)
        assert stats["s_zero", 2] < stats["s_zero", 1], (shape, stats)   # the flat interiors are eaten from the block edges
        if shape in LE.TERRACE_SHAPES:
            print(f"LLT_ROF terraces {shape}: s == 0 on {stats['s_zero', 1]:.3f} of the voxels entering iteration 1, "
                  f"{stats['s_zero', 2]:.3f} entering iteration 2")
    stats = {}
    D.run(phantom((7, 13, 37)), iterations=1, stats=stats, **D.PARAMS["A"])
    assert stats["s_zero", 1] < 0.01


def test_scaled_inputs_move_the_data_across_eps():
    """the phantom's s = |forward differences|^2 is of the order of 1e1: times 2^-14 it is of the order of eps = 1e-8 (the
    median within a factor of 100 of it, so eps is a visible part of n = sqrt(s + eps)), times 2^10 eps lies below half an
    ulp of s on nearly every voxel (s + eps == s); both inputs stay in the normal range"""
    f = phantom((7, 13, 37))
    eps = np.float32(1e-8)
    med, absorbed = {}, {}
    for e in LE.SCALE_EXPONENTS:
        x = LE.scaled(f, e)
        assert np.array_equal(np.ldexp(x.astype(np.float64), -e), f.astype(np.float64))
        assert np.all((np.abs(x) >= np.finfo(np.float32).tiny) | (x == 0))
        s = sum(np.diff(x, axis=ax, append=np.take(x, [-1], axis=ax)) ** 2 for ax in range(3)).astype(np.float32)
        med[e] = float(np.median(s))
        absorbed[e] = float(np.count_nonzero(s + eps == s)) / s.size
    print(f"median s: {med}; share of voxels with s + eps == s: {absorbed}")
    assert 1e-10 < med[-14] < 1e-6 and absorbed[-14] == 0.0
    assert absorbed[10] > 0.99
