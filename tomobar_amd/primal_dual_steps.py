"""The step rules of PDHG and SPDHG (docs/kernels/pdhg.md, spdhg.md) as pure host functions: numpy only, no device and no
library, so tests/test_primal_dual_steps.py holds them to the oracles' scalars bit for bit.  The drivers are held to their
oracles bit for bit too, hence float32 throughout: one rounding per operation, in the order written here."""
from typing import NamedTuple, Optional

import numpy as np
from numpy import float32

C = float32(0.95)   # sigma tau |K|^2 = C^2 < 1


class PdhgSteps(NamedTuple):
    sigma: float32                 # the sinogram block's step (scalar rule only) and the TV block's
    tau: Optional[float32]         # the primal step; None with the diagonal rule: an array there, built by the driver
    sigma_p: float32               # the TGV block: the two dual steps and the step of v
    sigma_q: float32
    tau_v: float32
    tau_s: float32                 # the stripe variable's step
    theta: Optional[float32]       # its threshold tau_s mu; None without `stripe_lambda`
    # the diagonal rule alone: sigma_i = numer_sigma / (A 1)_i and tau_j = numer_tau / ((A^T 1)_j + col_add)
    numer_sigma: Optional[float32] = None
    numer_tau: Optional[float32] = None
    col_add: Optional[float32] = None


def pdhg_steps(lipschitz, n_angles, nd, block, ratio, diagonal, stripes, stripe_lambda=None) -> PdhgSteps:
    """`block`: None, "PD_TV" or "PD_TGV", what ``_regularisation_["method"]`` holds after ``dicts_check``; `ratio`: sigma / tau;
    `stripes`: the stripe variable is on, mu = `stripe_lambda`.  `lipschitz` (|A|^2) is not read with the diagonal rule."""
    rho = float32(ratio)
    tv, tgv = block == "PD_TV", block == "PD_TGV"
    if diagonal:
        # Pock and Chambolle's diagonal steps (alpha = 1): sigma_i = c rho / (A 1)_i for the sinogram block, c rho / 2 for the
        # TV block (a forward-difference row has the absolute sum 2), tau_j = (c / rho) / ((A^T 1)_j + 2 nd)
        numer_sigma, numer_tau = C * rho, C / rho
        sigma = numer_sigma / float32(2)
        # the TGV block: a P row holds a forward difference and -I (absolute sum 3), a Q row sums to 2; a v_d column
        # meets -I once, Q_dd's difference and, for each e != d, the two rows Q_de stands for: 1 + 2 + 2 (nd - 1)
        sigma_p, sigma_q, tau_v = numer_sigma / float32(3), sigma, numer_tau / float32(2 * nd + 1)
        # with the stripe variable a row of [A S] gains one entry 1 and a column of S sums to the number of angles
        tau, tau_s = None, numer_tau / float32(n_angles)
        arrays = (numer_sigma, numer_tau, float32(2 * nd) if tv or tgv else float32(0))
    else:
        # sigma tau L_K = 0.95^2 with L_K = |A|^2 + |grad|^2 <= L_A + 4 nd; the TGV block [[grad, -I], [0, E]] has the
        # squared norm <= 12 (2D), 16 (3D)
        L_K = float32(lipschitz)
        if stripes:   # |[A S]|^2 <= |A|^2 + |S|^2 and |S|^2 is the number of angles, exactly
            L_K = L_K + float32(n_angles)
        if tv:
            L_K = L_K + float32(4 * nd)
        if tgv:
            L_K = L_K + float32(16 if nd == 3 else 12)
        s = C / np.sqrt(L_K)
        sigma, tau = s * rho, s / rho
        sigma_p, sigma_q, tau_v, tau_s = sigma, sigma, tau, tau
        arrays = ()
    theta = None if stripe_lambda is None else tau_s * float32(stripe_lambda)
    return PdhgSteps(sigma, tau, sigma_p, sigma_q, tau_v, tau_s, theta, *arrays)


def spdhg_steps(lipschitz, nd, m, tv, ratio):
    """(sigma_A, sigma_G, tau, w_A, w_G): the dual steps of a subset and of the TV block, the primal step and the weights 1 / p_j
    of the two kinds of update; sigma_j tau |K_j|^2 <= 0.95^2 p_j with p = 1 / E per subset and 1 / 2 for the TV block, E = the
    block updates of one epoch of `m` subsets.  `lipschitz` bounds every subset's |A_j|^2, `ratio` is `PDHG_ratio`."""
    gamma = float32(ratio)
    n_A, n_G = np.sqrt(float32(lipschitz)), np.sqrt(float32(4 * nd))
    w_A, w_G = float32(2 * m if tv else m), float32(2)
    tau = (C / gamma) / (w_A * n_A)
    if tv:
        tau = min(tau, (C / gamma) / (w_G * n_G))
    return (C * gamma) / n_A, (C * gamma) / n_G, tau, w_A, w_G
