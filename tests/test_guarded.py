"""CPU tests of tests/_guarded.py: a single stray element is found wherever it lands and reported at the right offset, writes
inside the view raise nothing, the view starts where `shift` says, the width rule gives the stated numbers, and the numbers
of the rule are still what the kernel sources say."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _guarded as G  # noqa: E402

CSRC = os.path.join(ROOT, "tomobar_amd", "csrc")
DTYPES = [np.float32, np.uint16, np.uint8]
SHAPES = [(3, 9, 11), (7,), (5, 70)]


def cpu(a_or_shape, **kw):
    return G.guarded(a_or_shape, device="cpu", **kw)


def _filled(shape, dtype):
    n = int(np.prod(shape))
    return (np.arange(n) % 251 + 1).astype(dtype).reshape(shape)


def _first_of_view(g):
    """index into g.buf of the view's first element"""
    isz = g.dtype.itemsize
    return (g.view.data_ptr() - g.buf.data_ptr()) // isz


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_a_single_stray_element_is_found_and_located(dtype, shift):
    for shape in SHAPES:
        a = _filled(shape, dtype)
        probe = cpu(a, dtype=dtype, shift=shift)
        first, total = _first_of_view(probe), probe.buf.numel()
        # position in the allocation -> the offset intact() must report
        places = {"one before the view": (first - 1, -1), "one after the view": (first + a.size, a.size),
                  "the first of the allocation": (0, -first), "the last of the allocation": (total - 1, total - 1 - first)}
        for what, (pos, offset) in places.items():
            g = cpu(a, dtype=dtype, shift=shift)
            assert g.intact() == (True, None) and g.intact() and g.unchanged()
            assert _first_of_view(g) == first and g.buf.numel() == total      # the layout does not depend on the allocation
            flat = g.buf.numpy()                                              # shares the memory of the CPU tensor
            flat[pos] = 1
            res = g.intact()
            assert not res and res == (False, offset), (what, shape, res, offset)
            assert g.unchanged()
            with pytest.raises(AssertionError, match="guard band"):
                g.check(what)
        # two stray elements: the first is reported
        g = cpu(a, dtype=dtype, shift=shift)
        g.buf.numpy()[first + a.size + 5] = 1
        g.buf.numpy()[3] = 1
        assert g.intact() == (False, 3 - first)


def test_the_band_is_compared_as_integers():
    """a NaN with another payload, and the default NaN, are damage although no float comparison tells them from the band"""
    for bits in (0x7FC00000, 0x7FC0BEEE, 0xFFC0BEEF):
        g = cpu((4, 5))
        g.buf.numpy().view(np.uint32)[2] = bits
        assert not g.intact()
    g = cpu((4, 5))
    band = g.buf.numpy()[:8]
    assert np.isnan(band).all() and (band.view(np.uint32) == 0x7FC0BEEF).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_writes_inside_the_view_raise_nothing(dtype):
    for shape in SHAPES:
        a = _filled(shape, dtype)
        g = cpu(a, dtype=dtype)
        assert np.array_equal(g.host(), a) and g.host().dtype == np.dtype(dtype)
        g.view.copy_(torch.from_numpy(_filled(shape, dtype)[..., ::-1].copy()))      # every element
        assert g.intact() and not g.unchanged()
        g.check("every element written")
        with pytest.raises(AssertionError, match="read-only"):
            g.check("every element written", read_only=True)
        # the band's own pattern as a value of the view: the view is not the band
        pat = np.array([G.PATTERN[g.dtype.itemsize]], G._UINT[g.dtype.itemsize]).view(dtype)[0]
        v = g.view.numpy()
        v[...] = pat
        assert g.intact()
        assert (g.host().view(G._UINT[g.dtype.itemsize]) == G.PATTERN[g.dtype.itemsize]).all()


def test_contents():
    g = cpu((3, 4))
    assert g.view.dtype == torch.float32 and tuple(g.view.shape) == (3, 4) and g.view.is_contiguous()
    assert (g.host().view(np.uint32) == 0x7FC00000).all()          # the default NaN: what a kernel never wrote shows
    assert (cpu((3, 4), fill=2.5).host() == 2.5).all()
    assert (cpu((6,), dtype=np.uint16).host() == 0).all() and (cpu((6,), dtype=np.uint8, fill=7).host() == 7).all()
    t = cpu(np.arange(12, dtype=np.uint16).reshape(3, 4))          # an integer table keeps its type
    assert t.view.dtype == torch.uint16 and t.dtype == np.uint16 and np.array_equal(t.host(), np.arange(12).reshape(3, 4))
    i = cpu(np.arange(5, dtype=np.int32))
    assert i.view.dtype == torch.int32 and (i.buf.numpy().view(np.uint32)[:4] == 0x7FC0BEEF).all()
    d = cpu(np.arange(5, dtype=np.float64))                        # float64 input becomes float32
    assert d.view.dtype == torch.float32 and np.array_equal(d.host(), np.arange(5, dtype=np.float32))
    with pytest.raises(AssertionError):
        cpu((3,)).unchanged()
    # every element outside the view holds the pattern
    for dtype in DTYPES:
        g = cpu(_filled((5, 7), dtype), dtype=dtype, shift=1)
        flat, first = g.buf.numpy().view(G._UINT[g.dtype.itemsize]), _first_of_view(g)
        assert (flat[:first] == G.PATTERN[g.dtype.itemsize]).all() and (flat[first + 35:] == G.PATTERN[g.dtype.itemsize]).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_shift_places_the_view_4k_bytes_past_a_16_byte_boundary(dtype):
    for shape in SHAPES + [(4099,), (1,)]:
        for k in (0, 1, 2, 3):
            g = cpu(shape, dtype=dtype, shift=k)
            assert g.view.data_ptr() % 16 == 4 * k, (shape, k)
            first = _first_of_view(g)
            assert first >= G.band_width(shape) and g.buf.numel() - first - g.view.numel() >= G.band_width(shape)
    with pytest.raises(AssertionError):
        cpu((3,), shift=4)


def test_width_rule():
    assert G.band_width((3, 9, 11)) == 3 * 9 * 11 + 16 * 9 * 11 == 1881
    assert G.band_width((4099,)) == 4099                 # 1-D: plane = 0
    assert G.band_width((1, 5, 70)) == 350 + 16 * 350 == 5950
    assert G.band_width((7,)) == 1024 and G.band_width((2, 3)) == 1024 == 256 * 4
    assert G.band_width((100,), planes=45 * 19) == 100 + 16 * 45 * 19      # a flat buffer of documented size
    assert G.WORKGROUP_FLOAT4 == 1024 and G.DEEPEST_TILE_PLANES == 16
    g = cpu((3, 9, 11))
    first = _first_of_view(g)
    assert first >= 1881 and g.buf.numel() - (first + 297) >= 1881


def test_the_numbers_of_the_rule_are_what_the_sources_say():
    """the width rule was read from these lines: a kernel that deepens its tile or widens its block fails here until the
    rule follows"""
    for fname, text in G.CITES:
        with open(os.path.join(CSRC, fname)) as fh:
            assert text in fh.read(), (fname, text)
