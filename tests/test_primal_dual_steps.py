"""No GPU: the step rules of PDHG and SPDHG (tomobar_amd/primal_dual_steps.py, what the drivers call) against the scalars the
oracles under tests/ form for themselves, bit for bit and as ``numpy.float32`` objects, over a grid of operator norms, angle
counts, dimensions, regularisers, ratios and the stripe variable."""
import itertools
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _pdhg_diag_oracle as D  # noqa: E402
import _pdhg_oracle as P  # noqa: E402
import _pdhg_stripe_oracle as S  # noqa: E402
import _pdhg_tgv_oracle as G  # noqa: E402
import _spdhg_oracle as SP  # noqa: E402
from tomobar_amd.primal_dual_steps import pdhg_steps, spdhg_steps  # noqa: E402

F = np.float32
LIPSCHITZ = (1e-3, 1.0, 1234.567, 3.1e6)
N_ANGLES = (1, 90, 1800)
ND = (2, 3)
BLOCKS = (None, "PD_TV", "PD_TGV")
RATIOS = (0.25, 1.0, 3.7, 4)     # the 4 is an int on purpose: what a caller's dictionary may hold
MU = (0.05, 2.5)
SUBSETS = (1, 3, 4, 6)
GRID = list(itertools.product(LIPSCHITZ, N_ANGLES, ND, BLOCKS, RATIOS))
SHORT = {None: None, "PD_TV": "TV", "PD_TGV": "TGV"}     # the stripe oracle's names of the regularisers


def same(got, want, what):
    assert type(got) is np.float32 and type(want) is np.float32, (what, type(got), type(want))
    assert got.view(np.uint32) == want.view(np.uint32), (what, float(got), float(want))


def float32_but(st, absent):
    """every field an ``numpy.float32``, those named in `absent` None"""
    for name, v in st._asdict().items():
        assert (v is None) if name in absent else (type(v) is np.float32), (name, type(v))


def test_the_module_needs_nothing_but_numpy():
    import tomobar_amd.primal_dual_steps as M
    mods = {v.__name__.split(".")[0] for v in vars(M).values() if isinstance(v, types.ModuleType)}
    assert mods == {"numpy"}, mods


@pytest.mark.parametrize("stripes", [False, True], ids=["no stripes", "stripes"])
def test_the_scalar_rule_equals_the_oracles(stripes):
    for L, na, nd, block, ratio in GRID:
        what = (L, na, nd, block, ratio, stripes)
        st = pdhg_steps(L, na, nd, block, ratio, False, stripes)
        float32_but(st, {"theta", "numer_sigma", "numer_tau", "col_add"})
        if stripes:
            sigma, tau = P.scalars(None, nd, ratio=ratio, L_K=S.lipschitz(L, na, nd, SHORT[block]))
            sigma_p, sigma_q, tau_v = sigma, sigma, tau
        elif block == "PD_TGV":
            sigma_p, sigma_q, tau, tau_v = G.scalars(L, nd, ratio)
            sigma = sigma_p
        else:
            sigma, tau = P.scalars(L, nd, block == "PD_TV", ratio)
            sigma_p, sigma_q, tau_v = sigma, sigma, tau
        for name, want in (("sigma", sigma), ("tau", tau), ("sigma_p", sigma_p), ("sigma_q", sigma_q), ("tau_v", tau_v), ("tau_s", tau)):
            same(getattr(st, name), want, what + (name,))


@pytest.mark.parametrize("stripes", [False, True], ids=["no stripes", "stripes"])
def test_the_diagonal_rule_equals_the_oracles(stripes):
    for L, na, nd, block, ratio in GRID:
        what = (L, na, nd, block, ratio, stripes)
        st = pdhg_steps(L, na, nd, block, ratio, True, stripes)
        float32_but(st, {"tau", "theta"})
        a, t, sigma_G, w = D.host_scalars(nd, block is not None, ratio)
        sigma_p, sigma_q, tau_v = G.diag_scalars(nd, ratio)
        for name, want in (("numer_sigma", a), ("numer_tau", t), ("sigma", sigma_G), ("col_add", w), ("sigma_p", sigma_p),
                           ("sigma_q", sigma_q), ("tau_v", tau_v), ("tau_s", F(t / F(na)))):
            same(getattr(st, name), want, what + (name,))
        assert st == pdhg_steps(None, na, nd, block, ratio, True, stripes), what     # the operator norm is not read


@pytest.mark.parametrize("diagonal", [False, True], ids=["scalar", "diagonal"])
def test_the_stripe_threshold_equals_the_oracle(diagonal):
    for (L, na, nd, block, ratio), mu in itertools.product(GRID, MU):
        st = pdhg_steps(L, na, nd, block, ratio, diagonal, True, mu)
        same(st.theta, S.threshold(st.tau_s, mu), (L, na, nd, block, ratio, diagonal, mu))
        assert st[:6] == pdhg_steps(L, na, nd, block, ratio, diagonal, True)[:6]     # the steps do not depend on mu


@pytest.mark.parametrize("tv", [True, False], ids=["TV", "no TV"])
def test_the_spdhg_rule_equals_the_oracle(tv):
    for L, nd, m, ratio in itertools.product(LIPSCHITZ, ND, SUBSETS, RATIOS):
        got, want = spdhg_steps(L, nd, m, tv, ratio), SP.scalars(L, nd, m, tv, ratio)
        assert len(got) == len(want) == 5
        for name, g, w in zip(("sigma_A", "sigma_G", "tau", "w_A", "w_G"), got, want):
            same(g, w, (L, nd, m, tv, ratio, name))
