"""MI355X tests of the LLT_ROF z-march at the shapes of tests/_llt_rof_edge_shapes.py: the array ends on, one before and one
past the last emitting lane of a wave / the last column of a workgroup, the same in rows, both neighbours two rows away
clamp onto the tile, the z-chunk count changes, and a slab launch with ghost planes is z-chunked -- on the noise phantom, on
`terraces` (exact zeros and ties: the 0 / (0 + eps) and 0 / sqrt(eps) quotients) and on the phantom scaled by 2^-14 and 2^10
(s of the order of eps, and eps below half an ulp of s).  Bit equality with tests/_llt_rof_oracle.py throughout.
tests/test_llt_rof_edge_shapes.py proves on the CPU that the shapes and the inputs have the properties they are here for."""
import functools
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _llt_rof_edge_shapes as LE  # noqa: E402
import _march_gpu as G  # noqa: E402
from _llt_rof_oracle import ORACLE as D  # noqa: E402
from _march_gpu import same_bits  # noqa: E402
from _tgv_oracle import phantom  # noqa: E402

COUNTS = (1, 2, 5)   # the direct input-to-output launch and both parities of the ping-pong
KINDS = ["phantom", "terraces", "scaled"]


def _run(f_host, p, n):
    """n iterations on the GPU into a NaN-filled output; the input's bits are checked afterwards"""
    return G.march("LLT_ROF", f_host, p, n)[0]


def _fields(kind, shape):
    """[(label, input)]"""
    if kind == "phantom":
        return [("phantom", phantom(shape))]
    if kind == "terraces":
        return [("terraces", LE.terraces(shape))]
    return [(f"phantom*2^{e}", LE.scaled(phantom(shape), e)) for e in LE.SCALE_EXPONENTS]


@functools.lru_cache(maxsize=None)
def _want(kind, shape, pname):
    """[(label, input, {n: the float32 numpy oracle after n iterations})], computed once per session and never modified"""
    out = []
    for label, f in _fields(kind, shape):
        res = D.many(f, D.PARAMS[pname], COUNTS)
        for v in res.values():
            v.setflags(write=False)
        f.setflags(write=False)
        out.append((label, f, res))
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pname", sorted(D.PARAMS))
@pytest.mark.parametrize("group", LE.groups())
def test_march_edges_equal_the_oracle(group, pname, kind):
    """every 2D and 3D edge shape of the group, after 1, 2 and 5 iterations, bit for bit"""
    for case in LE.cases(group):
        for label, f, want in _want(kind, case.shape, pname):
            for n in COUNTS:
                same_bits(_run(np.array(f), D.PARAMS[pname], n), want[n], (case, label, pname, n))


def test_terraces_take_the_zero_quotients_at_every_shape_used():
    """from the oracle: s == 0 on at least a quarter of the voxels entering iteration 1 at every `terraces` shape"""
    for shape in LE.terrace_shapes():
        stats = {}
        D.run(LE.terraces(shape), iterations=1, stats=stats, **D.PARAMS["A"])
        assert 0.25 <= stats["s_zero", 1] < 1.0, (shape, stats)


@pytest.mark.parametrize("pname", sorted(D.PARAMS))
@pytest.mark.parametrize("shape", LE.TERRACE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_terraces_over_several_blocks(shape, pname):
    """(20, 24, 70) and (40, 130): more than one wave in x and y, three z-levels of blocks"""
    f = LE.terraces(shape)
    want = D.many(f, D.PARAMS[pname], COUNTS)
    for n in COUNTS:
        same_bits(_run(f, D.PARAMS[pname], n), want[n], (shape, pname, n))


# ------------------------------------------------------------------------------------------------ chunked z-slabs
@pytest.mark.parametrize("kind", ["phantom", "terraces"])
@pytest.mark.parametrize("schedule", ["plain", "ranges"])
def test_llt_rof_chunked_slabs_equal_whole_volume(schedule, kind, iters=6):
    """two ranks of 33 local planes: every slab launch is z-chunked (three chunks over all local planes, rank 1's first
    starting at its ghost planes; the interior launch of the "ranges" schedule starts past the boundary planes and is still
    chunked)"""
    from tomobar_amd.slab import slab_bounds
    s = LE.SLAB
    for sizes in LE.slab_launch_chunks(schedule):
        assert len(sizes) >= (3 if schedule == "plain" else 2), (schedule, sizes)
    f = phantom(s.shape) if kind == "phantom" else LE.terraces(s.shape)
    want = D.run(f, iterations=iters, **D.PARAMS["A"])
    vd = torch.from_numpy(f).cuda()
    got = G.run_slabs("LLT_ROF", vd, [slab_bounds(s.shape[0], s.world, r) for r in range(s.world)], schedule, "A", iters)
    same_bits(got, want, (s.shape, schedule, kind))
