"""CPU tests of tests/_edge_shapes.py: the table of edge shapes has the properties it claims under the restated grid, every
launch realises every property, the geometry is still what the launch lines say, and the `terraces` input reaches -- on the
numpy oracles alone -- the branches it is there for."""
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from _diff4th_oracle import ORACLE as D  # noqa: E402
import _edge_shapes as E  # noqa: E402
from _ndf_oracle import ORACLE as N  # noqa: E402
import _tgv_oracle as T  # noqa: E402

CSRC = os.path.join(ROOT, "tomobar_amd", "csrc")


# ------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("launch", list(E.LAUNCHES))
def test_geometry_is_what_the_launch_lines_say(launch):
    """the numbers of a table entry were read from these lines: a launch site that changes its tiling fails here until the
    table follows"""
    for fname, text in E.LAUNCHES[launch].cites:
        with open(os.path.join(CSRC, fname)) as fh:
            assert text in fh.read(), (launch, fname, text)


def test_grid_restatement_on_known_launches():
    """the chunkings the existing tests document: (40, 150, 200) is three chunks of 14, 14 and 12 planes on 2 x 10 (NDF,
    Diff4th) or 2 x 19 (TGV) workgroup tiles; a 1024^3 NDF iteration is 9 x 64 tiles = 2304 waves,
    so ceil(32768 / 2304) = 15 chunks of ceil(1024 / 15) = 69 planes"""
    for name, tiles in (("ndf", (2, 10)), ("diff4th", (2, 10)), ("tgv", (2, 19))):
        g = E.LAUNCHES[name].grid((40, 150, 200))
        assert (g.gx, g.gy) == tiles and E.chunk_sizes(g, 40) == [14, 14, 12], (name, g)
        assert g.tiles_per_xcd == E.ceil_div(tiles[0] * tiles[1], 8) and g.blocks == 8 * g.tiles_per_xcd * 3
    g = E.LAUNCHES["ndf"].grid((1024, 1024, 1024))
    assert (g.gx, g.gy, g.tiles_per_xcd) == (9, 64, 72) and g.zchunk == 69 and g.chunks == 15
    g = E.LAUNCHES["tgv"].grid((150, 200))   # 2D: one chunk whatever the size
    assert g.chunks == 1 and g.zchunk == 1
    g = E.LAUNCHES["pd_rows2d_k3"].grid((24, 19))
    assert (g.gx, g.gy, g.blocks) == (1, 3, 1)


@pytest.mark.parametrize("launch", list(E.LAUNCHES))
def test_every_entry_has_the_property_it_claims(launch):
    L = E.LAUNCHES[launch]
    entries = E.cases(launch)
    assert entries
    for case in entries:
        props = E.properties(L, case.group)
        assert case.claims and len(case.shape) in L.dims, case
        for claim in case.claims:
            assert props[claim](case.shape), (case, L.grid(case.shape), L.wave_columns(case.shape[-1]), L.wave_rows(case.shape[-2]))
        assert int(np.prod(case.shape)) <= 300_000, case      # every case stays small


@pytest.mark.parametrize("launch", list(E.LAUNCHES))
def test_every_property_is_claimed_by_an_entry_of_every_launch(launch):
    L = E.LAUNCHES[launch]
    for group in E.GROUPS:
        for nd in L.dims:
            if group == "z" and nd == 2:
                continue
            claimed = {c for case in E.cases(launch, group, nd) for c in case.claims}
            missing = [p for p in E.properties(L, group) if p not in claimed]
            assert not missing, (launch, group, nd, missing)
    assert E.groups_of(launch) == (["x", "y"] if L.rows2d else ["x", "y", "z"])


def test_the_table_holds_the_shapes_the_geometry_gives():
    """spot checks in plain numbers, so that a slip in the derivation shows"""
    shapes = lambda name, group, nd=None: [c.shape for c in E.cases(name, group, nd)]  # noqa: E731
    assert shapes("ndf", "x", 3) == [(3, 9, d) for d in (61, 62, 63, 123, 124, 125)]
    assert shapes("tgv", "y", 2) == [(d, 64) for d in (3, 4, 5, 7, 8, 9)]
    assert shapes("diff4th", "y", 3) == [(3, d, 61) for d in (7, 8, 9, 15, 16, 17)] + [(3, 2, 60), (3, 3, 60)]
    assert shapes("ndf", "z") == [(d, 9, 11) for d in (15, 16, 17, 31, 32, 33, 49)] + [(33, 1, 993)]
    assert shapes("rof", "z")[-1] == (65, 2, 961)
    assert shapes("pd_single", "x") == [(3, 9, d) for d in (61, 62, 63, 247, 248, 249, 123, 125, 185, 187)]
    assert shapes("pd_x2_relaxed", "y") == [(3, d, 61) for d in (3, 4, 5, 15, 16, 17)]
    assert shapes("pd_x2_exact", "y") == [(3, d, 61) for d in (3, 4, 5, 7, 8, 9)]
    assert shapes("pd_xk3", "z") == [(d, 9, 11) for d in (71, 72, 73, 143, 144, 145, 217)] + [(145, 1, 929)] + [(d, 9, 11) for d in (1, 2, 3, 4)]
    assert shapes("pd_rows2d_k3", "x") == [(9, 57), (9, 58), (9, 59), (8, 233)]
    assert E.chunk_sizes(E.LAUNCHES["ndf"].grid((17, 9, 11)), 17) == [9, 8]          # "two chunks of 9 and 8"


def test_pd_plan_restatement_equals_the_slab_drivers_plan():
    from tomobar_amd.slab import pd_launch_plan
    for dz in (1, 2, 3, 4, 50):
        for iters in range(0, 14):
            assert E.pd_plan(3, dz, iters) == pd_launch_plan(iters, False, kmax=min(3, dz)), (dz, iters)
    assert E.pd_plan(2, 1, 7) == [3, 2, 2] and E.pd_plan(2, 1, 1) == [1]
    for dz, plan in E.PD_THIN_PLANS.items():
        assert E.pd_plan(3, dz, 7) == plan


# ------------------------------------------------------------------------------------------------ chunked z-slabs
@pytest.mark.parametrize("op", sorted(E.SLABS))
def test_slab_shapes_are_chunked_on_every_launch(op):
    from tomobar_amd import slab as S
    s = E.SLABS[op]
    L = E.LAUNCHES[s.launches[0]]
    nzl = s.shape[0] // s.world
    assert s.shape[0] % s.world == 0 and nzl == 2 * L.m + 1
    plain = E.slab_launch_chunks(op, "plain")
    assert all(len(sizes) == 3 for sizes in plain), plain          # three chunks, rank 1's first starts at the ghost planes
    interior = E.slab_launch_chunks(op, "ranges")
    assert all(len(sizes) >= 2 for sizes in interior), interior    # the interior launch (out_begin > 0 on rank 1) is chunked
    # the boundary planes the table takes off are the ones the slab classes hand out
    cls = {"NDF": S.NdfSlab, "Diff4th": S.Diff4thSlab, "ROF_TV": S.RofSlab, "PD_TV": S.PdSlab}[op]
    for rank in range(s.world):
        lo, hi = rank > 0, rank < s.world - 1
        me = types.SimpleNamespace(nzl=nzl, has_lo=lo, has_hi=hi, lo=s.ghost[0] if lo else 0, hi=s.ghost[1] if hi else 0)
        edges, (b0, b1) = cls.boundary_ranges(me)
        assert (b0, nzl - b1) == (s.boundary[0] if lo else 0, s.boundary[1] if hi else 0), (op, rank, edges, b0, b1)
        assert all(1 <= z1 - z0 <= 3 for z0, z1 in edges) and sum(interior[rank]) == b1 - b0
    if op == "PD_TV":   # the K = 2 and the single-iteration launches of a slab run are chunked as well
        for name, nout in (("pd_x2_relaxed", nzl - 3), ("pd_x2_exact", nzl - 3), ("pd_single", nzl)):
            assert E.LAUNCHES[name].grid((nout,) + s.shape[1:], nout).chunks >= 2, name


# ------------------------------------------------------------------------------------------------ the input families
TERRACE_SHAPES = [(20, 24, 70), (40, 130)]


def test_terraces_values_and_scaled():
    x = E.terraces((20, 24, 70))
    assert x.dtype == np.float32 and set(np.unique(x)) == {-6.0, -3.0, 0.0, 3.0, 6.0}
    assert x[0, 0, 0] == -6 and x[0, 0, 8] == -3 and x[0, 8, 0] == 0 and x[8, 0, 0] == 3 and x[8, 8, 8] == -3
    assert np.array_equal(E.terraces((24, 70)), x[0])
    assert np.array_equal(E.terraces((5, 9), scale=0.25), 0.25 * E.terraces((5, 9)))
    for e in E.SCALE_EXPONENTS:
        y = E.scaled(E.step_noise((6, 9, 13)) - np.float32(0.6), e)
        assert y.dtype == np.float32 and np.array_equal(np.ldexp(y.astype(np.float64), -e), (E.step_noise((6, 9, 13)) - np.float32(0.6)))
        assert np.all((np.abs(y) >= np.finfo(np.float32).tiny) | (y == 0))


@pytest.mark.parametrize("shape", TERRACE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_terraces_run_finite_through_the_three_oracles(shape):
    f = E.terraces(shape)
    share = E.zero_share(f)
    print(f"terraces {shape}: {share:.3f} of the forward differences are exactly zero")
    assert 0.85 < share < 0.93
    runs = [(f"NDF {k}", lambda n, p=p: N.run(f, iterations=n, **p)) for k, p in sorted(N.PARAMS.items())]
    runs += [(f"Diff4th {k}", lambda n, p=p: D.run(f, iterations=n, **p)) for k, p in sorted(D.PARAMS.items())]
    runs += [(f"TGV {k}", lambda n, p=p: T.tgv(f, iterations=n, **p)) for k, p in (("A", T.PARAMS_A), ("B", T.PARAMS_B))]
    for what, run in runs:
        for n in (1, 4):
            out = run(n)
            assert out.dtype == np.float32 and np.all(np.isfinite(out)), (what, n)
            assert not np.array_equal(out, f), (what, n)


def _terrace_shapes(names, op_min=1):
    seen = []
    for name in names:
        for case in E.cases(name):
            if case.shape not in seen and min(case.shape) >= op_min:
                seen.append(case.shape)
    return seen


def test_terraces_reach_the_zero_difference_paths_at_every_shape_used():
    """at least half -- and fewer than all -- of the forward differences are exactly zero at every shape the GPU tests run
    `terraces` on; NDF's oracle counts the same share on its own differences, and Tukey's rejected range is entered"""
    for shape in _terrace_shapes(E.LAUNCHES) + TERRACE_SHAPES + [s.shape for s in E.SLABS.values()]:
        share = E.zero_share(E.terraces(shape))
        assert 0.5 <= share < 1.0, (shape, share)
    for shape in _terrace_shapes(["ndf"]) + TERRACE_SHAPES:
        for pname, p in sorted(N.PARAMS.items()):
            stats = {}
            N.run(E.terraces(shape), iterations=1, stats=stats, **p)
            assert stats["zero"] == E.zero_share(E.terraces(shape)) and 0.5 <= stats["zero"] < 1.0, (shape, pname, stats)
            assert stats["above"] > 0.0 if pname in "CD" else True, (shape, pname, stats)   # sigma = 4 (Tukey) / 0.5: steps of 3 and 6
    for shape in TERRACE_SHAPES:
        stats = {}
        T.tgv(E.terraces(shape), iterations=1, stats=stats, **T.PARAMS_A)
        assert 0.0 < stats["n_gt_1"] < 0.5, stats    # the projection is active at the block edges only: P = 0 elsewhere


def test_terraces_reach_the_masked_quotient_of_diff4th():
    """G == 0 on at least a quarter -- and fewer than all -- of the voxels entering Diff4th's first iteration at every shape
    used; the shares docs/kernels/diff4th.md quotes"""
    for shape in _terrace_shapes(["diff4th"]) + TERRACE_SHAPES + [E.SLABS["Diff4th"].shape]:
        stats = {}
        D.run(E.terraces(shape), iterations=2, stats=stats, **D.PARAMS["A"])
        assert 0.25 <= stats["g_zero", 1] < 1.0, (shape, stats)
        assert stats["g_zero", 2] < stats["g_zero", 1], (shape, stats)   # the flat interiors are eaten from the block edges
        if shape in TERRACE_SHAPES:
            print(f"Diff4th terraces {shape}: G == 0 on {stats['g_zero', 1]:.3f} of the voxels in iteration 1, "
                  f"{stats['g_zero', 2]:.3f} in iteration 2")
    stats = {}
    D.run(T.phantom((7, 13, 37)), iterations=1, stats=stats, **D.PARAMS["A"])
    assert stats["g_zero", 1] == 0.0     # the noise input never takes the masked branch
