"""CPU: proves tests/_fourier_gather_oracle.py and its cases before a GPU sees them.  The numpy restatement of the reference's
two gathering kernels (oracle/fourier_oracle.py gather_scatter / gather_center, float32) stands in for the HIP kernel on every
launch of every case and must satisfy what tests/test_gpu_fourier_gather.py asks of the kernel -- at 1 x the bound, where the
kernel is granted 4 x --, the float32 decisions must lie inside the float64 intervals (`inconsistent == 0`), `undecided` must
stay within its cap, and every case must have the property it is listed for."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _fourier_gather_oracle as G  # noqa: E402


def float32_oracle(g, theta, n, m, mu, center_size):
    """f [Z][2n][2n] complex64 of oracle/fourier_oracle.py for samples g [nproj][n][Z], checkerboard sign applied.  Only the
    rays with a non-zero sample are handed over: a ray of zeros adds w * 0 = 0 to every sum, which changes no bit, and the
    scatter form costs a second per ray"""
    from oracle import fourier_oracle as FO
    rays = np.flatnonzero(np.any(g != 0, axis=(1, 2)))
    gz = np.ascontiguousarray(np.transpose(g[rays], (2, 0, 1)))
    th = np.asarray(theta, np.float32)[rays]
    f = np.zeros((gz.shape[0], 2 * n, 2 * n), np.complex64)
    if center_size >= FO.CENTER_SIZE_MIN:
        if center_size != 2 * n:
            FO.gather_scatter(gz, f, th, m, mu, n, center_size, only_outside=True)
        FO.gather_center(gz, f, th, m, mu, n, center_size)
    else:
        FO.gather_scatter(gz, f, th, m, mu, n)
    ii = np.arange(2 * n)
    return f * np.where(((ii[None, :] ^ ii[:, None]) & 1) == 1, np.float32(-1), np.float32(1))


@pytest.mark.parametrize("grid,setname", G.CASES, ids=[f"{a}-{b}" for a, b in G.CASES])
def test_float32_oracle_meets_the_reference(grid, setname):
    n, cs, _ = G.GRIDS[grid]
    th = G.angle_sets()[setname]
    m, mu = G.footprint(n)
    assert m == 5
    T = G.gather_terms(*G.numpy_tables(th), n, m, mu, cs)
    assert T.inconsistent == 0
    G.properties(grid, setname, T)
    for name, g, zc, exempt in G.launches(grid, setname):
        res = G.evaluate(T, g[:, :, :zc])
        G.check_cap(res, exempt, (grid, setname, name))
        got = float32_oracle(g[:, :, :zc], th, n, m, mu, cs)
        worst = G.compare(res, got, 1.0, (grid, setname, name))
        assert worst <= 1.0
        if name == "samples":     # a footprint is one weight per member point
            count = res.member.reshape(zc, -1).sum(1)
            for z, (p, r) in enumerate(G.sample_impulses(n, th)[1]):
                # the centre form's rmax is clipped to n - 1 and exclusive: the last radial sample reaches no box point
                if cs >= G.CENTER_SIZE_MIN and r == n - 1:
                    assert cs != 2 * n or count[z] == 0, (z, p, r, count[z])
                else:
                    assert count[z] > 0, (z, p, r, count[z])
            if cs < G.CENTER_SIZE_MIN:  # periodic wrap at all four edges
                ever = res.member.any(axis=0)
                assert ever[0].any() and ever[-1].any() and ever[:, 0].any() and ever[:, -1].any()


def test_compare_refuses_what_it_must():
    """a dropped term, a doubled one, the neighbouring sample's weight and a stray value all fail, whatever the weight"""
    grid, setname = "n100-c192", "nine"
    n, cs, _ = G.GRIDS[grid]
    th = G.angle_sets()[setname]
    m, mu = G.footprint(n)
    T = G.gather_terms(*G.numpy_tables(th), n, m, mu, cs)
    g = np.zeros((th.size, n, 2), np.complex64)
    g[3, 40, 0] = 1
    g[3, 41, 1] = 1
    res = G.evaluate(T, g)
    good = res.value.astype(np.complex64)
    assert G.compare(res, good, 1.0) <= 1.0
    mem = np.argwhere(res.member[0] & ~res.undecided[0] & res.member[1] & ~res.undecided[1])
    weakest = min(mem, key=lambda q: abs(good[0, q[0], q[1]]))
    strongest = max(mem, key=lambda q: abs(good[0, q[0], q[1]]))
    assert abs(good[0][tuple(weakest)]) < 1e-9 * abs(good[0][tuple(strongest)])
    for q in (tuple(weakest), tuple(strongest)):
        for wrong in (0.0, 2 * good[0][q], good[1][q]):
            bad = good.copy()
            bad[0][q] = wrong
            with pytest.raises(AssertionError):
                G.compare(res, bad, 4.0)
    out = np.argwhere(~res.member[0] & ~res.undecided[0])[0]
    bad = good.copy()
    bad[0, out[0], out[1]] = 1e-30
    with pytest.raises(AssertionError):
        G.compare(res, bad, 4.0)


def test_dev_entry_is_bound_in_the_dev_library_alone():
    from tomobar_amd import _lib
    assert "tomo_fourier_gather" in _lib.DEV_SIGNATURES and "tomo_fourier_gather" not in _lib.SIGNATURES
    assert not hasattr(_lib.lib(), "tomo_fourier_gather")
    with _lib.use_flavour("dev") as dev:
        assert dev.tomo_fourier_gather.argtypes == _lib.DEV_SIGNATURES["tomo_fourier_gather"][1]
