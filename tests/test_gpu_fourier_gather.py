"""MI355X: the gathering kernel of the Fourier reconstruction (csrc/fourier_inv.hip, gather_kernel) grid point by grid point.

`tomo_fourier_gather` (libtomo_mi355x_dev.so) runs the table set-up and the launch of tomo_fourier_inv on the test's own
arrays.  Every launch is compared with tests/_fourier_gather_oracle.py -- which tests/test_fourier_gather_oracle.py proves on the
CPU, on these very inputs -- by that module's `compare`: outside `undecided` membership is equal, non-members are exactly
zero and every value lies within 4 x the forward error bound (the margin the relaxed PD_TV is granted over its +-1 ulp family,
over a bound the float32 CPU oracle meets at 1 x); inside `undecided` the value is one of the listed alternatives.  The cos /
sin tables are the C library's cosf / sinf through ctypes, what the host code computes.

The 64 slice-pair lanes of a launch carry 64 experiments: sample impulses (one (angle, radius) per lane: the footprint of one
sample, so a miss, a double count or the neighbouring sample's weight is an error of order one whatever the weight), ray
impulses (one angle per lane: the hit test and the angular pruning) and dense complex normal samples with zc = 4 (values,
summation, the zc < 64 store mask).  g and f sit in guard bands, f NaN-filled and 64 planes deep: the bands must be intact, g
unchanged, the planes z >= zc still NaN.  Rows of f are exactly 2n wide, so a store at x >= 2n would land in the next row, which
the values show, or in the band."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = [pytest.mark.gpu, pytest.mark.dev_variants]
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _fourier_gather_oracle as G  # noqa: E402
from _guarded import guarded  # noqa: E402


def _launch(g, zc, theta, n, m, mu, center_size, what):
    """f [zc][2n][2n] complex64 of one launch on guarded arrays; the checks on the arrays themselves"""
    from tomobar_amd import _lib as L
    nproj = theta.size
    assert g.shape == (nproj, n, 64) and g.dtype == np.complex64
    src = guarded(np.ascontiguousarray(g).view(np.float32).reshape(nproj, n, 128))
    dst = guarded((64, 2 * n, 4 * n))
    th = np.ascontiguousarray(theta, np.float32)
    L.check(L.lib().tomo_fourier_gather(src.view.device.index, src.view.data_ptr(), dst.view.data_ptr(), zc, nproj, n, m,
                                        float(mu), center_size, th.ctypes.data,
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    src.check((what, "g"), read_only=True)
    dst.check((what, "f"))
    f = dst.host()
    assert np.isnan(f[zc:]).all(), (what, "a plane z >= zc was written")
    return f[:zc].view(np.complex64).reshape(zc, 2 * n, 2 * n)


@pytest.mark.parametrize("grid,setname", G.CASES, ids=[f"{a}-{b}" for a, b in G.CASES])
def test_gather_point_by_point(grid, setname):
    n, cs, _ = G.GRIDS[grid]
    th = G.angle_sets()[setname]
    m, mu = G.footprint(n)
    T = G.gather_terms(*G.libm_tables(th), n, m, mu, cs)
    assert T.inconsistent == 0
    for name, g, zc, exempt in G.launches(grid, setname):
        what = (grid, setname, name)
        res = G.evaluate(T, g[:, :, :zc])
        G.check_cap(res, exempt, what)
        got = _launch(g, zc, th, n, m, mu, cs, what)
        worst = G.compare(res, got, 4.0, what)
        print(f"fourier gather {grid} {setname} {name}: worst |got - value| / bound = {worst:.3f}, "
              f"{int(res.undecided.sum())} undecided of {int(res.member.sum())} member points")


def test_bad_arguments_are_refused():
    from tomobar_amd import _lib as L
    lib = L.lib()
    th = np.zeros(3, np.float32)
    g = torch.zeros((3, 40, 128), device="cuda")
    f = torch.zeros((64, 80, 160), device="cuda")
    ok = [0, g.data_ptr(), f.data_ptr(), 4, 3, 40, 5, 1e-3, 80, th.ctypes.data, None]
    for pos, bad in ((1, None), (2, None), (9, None), (3, 0), (3, 65), (4, 0), (5, 41), (6, 0), (6, 65), (7, 0.0), (8, 81), (8, -1)):
        args = list(ok)
        args[pos] = bad
        assert lib.tomo_fourier_gather(*args) == L.E_INVALID, (pos, bad)
    assert lib.tomo_fourier_gather(*ok) == L.OK
    torch.cuda.synchronize()
