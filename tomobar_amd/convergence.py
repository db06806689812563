"""The stopping rule behind ``_algorithm_["tolerance"]`` and ``_regularisation_["tolerance"]`` (host arithmetic only).

The reference accepts both keys and, in this version, reads neither; the rule is this project's (formula-level parity,
unpinned; docs/kernels/convergence.md).  For iterates ``v_0, v_1, ...`` (float32) and a check interval ``c``::

    num_n = sum (v_n - v_{n-c})^2      den_n = sum v_n^2      (float64 sums of the float32 values: ops.rel_change)
    d_n   = sqrt(num_n / den_n)        (0 when num_n = 0; +inf when den_n = 0 < num_n)
    stop after iterate n  <=>  tolerance > 0  and  d_n < tolerance

Outer loops compare consecutive outer iterations (c = 1, the same phase of two passes over the subsets); the TV operators
compare every ``INNER_INTERVAL`` iterations and only where at least ``INNER_MIN_SAVED`` requested iterations remain.
Over z-slabs ``num`` and ``den`` are summed over the ranks before the division, so every rank takes the whole-volume
decision.
"""

from __future__ import annotations

import math

INNER_INTERVAL = 6    # iterations between two checks of a TV operator (every check synchronises the stream once)
INNER_MIN_SAVED = 3   # ... and a check that could save fewer iterations than this is not made


def relative_change(num: float, den: float) -> float:
    if num == 0.0:
        return 0.0
    if den == 0.0:
        return math.inf
    return math.sqrt(num / den)


def inner_check_due(n: int, iterations: int) -> bool:
    """True if a TV operator asked for `iterations` evaluates the rule after its n-th iteration."""
    return n > 0 and n % INNER_INTERVAL == 0 and iterations - n >= INNER_MIN_SAVED


def check_tolerance(value, name: str) -> float:
    """0.0 for a missing key / None ("off"); ValueError for a negative or non-finite value."""
    if value is None:
        return 0.0
    try:
        tol = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a number >= 0") from None
    if not math.isfinite(tol) or tol < 0.0:
        raise ValueError(f"{name} must be a finite number >= 0 (0 switches early stopping off), got {value!r}")
    return tol
