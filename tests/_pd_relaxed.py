"""TEST INFRASTRUCTURE: what the shipped float32 PD_TV (relaxed arithmetic, `tomo_set_variant("pdtv", 0)`) is held to,
element for element.  Nothing here touches a GPU on import; tests/test_pd_relaxed_oracle.py proves the helper on the CPU,
tests/test_gpu_pdtv_default.py and the `pd_arith` sites of the other GPU files use it on the MI355X.

The relaxed kernels differ from something a CPU reproduces bit for bit in ONE operation: v_rsq_f32 in the projection of an
isotropic dual that left the unit ball (pd_dual_t<..., FAST = 1> of tomobar_amd/csrc/tv_kernels.hip, pd_dual2 of
tv_slices.hip).  The ISA manual gives it 1 ulp.  oracle.pd_tv_relaxed restates everything else and puts the reciprocal
square root on RN(1 / sqrt(x)) or one float32 below / above it.  Three tiers follow:

  1. methodTV = 1, and isotropic inputs on which no dual ever leaves the unit ball: the model has no hardware-dependent
     operation; `check_elementwise` is bit equality (B = 0).
  2. one explicit step (tomo_pdtv_iter_slab): `deduce_offsets` reads from the duals the kernel returned which of the three
     candidates the hardware used at every voxel, `replay` runs the model with exactly those and demands bit equality.
  3. everything else: `envelope` = B, the largest element-wise distance of ten members of the family of offset patterns from
     the model; `check_elementwise` asserts max|got - model| <= 4 B.  Margin 4: ten members sample a set of
     3^(voxels x iterations) patterns of which the hardware's is one more; the two biased members (all -1, all +1) cover an
     error that accumulates linearly and not as a random walk.  B comes from the model alone, never from the kernel."""
import collections

import numpy as np

from oracle import tomo_oracle as O

# scal = (sigma, tau, lt, theta) as np.float32; slices: every x[k] is a 2D image of its own (tomo_pdtv_slices)
Params = collections.namedtuple("Params", "scal iters methodTV nonneg slices", defaults=(False,))
SEEDS = tuple(range(1, 9))
MARGIN = 4
WIDTH = 1    # candidates of v_rsq_f32: RN(1 / sqrt(x)) and WIDTH floats either side (the ISA manual's 1 ulp)
STATS = []   # (what, B in ulp of max|model|, max|got - model| / B or None where B = 0): printed by the GPU file


def params(lam, iters, methodTV=0, nonneg=0, lipschitz=8.0, slices=False):
    return Params(O.pd_scalars(lam, lipschitz), int(iters), int(bool(methodTV)), int(bool(nonneg)), bool(slices))


def _run(x, p, mode, seed=0, counts=False, fault=None):
    x = np.ascontiguousarray(x, dtype=np.float32)
    kw = dict(iterations=p.iters, methodTV=p.methodTV, nonneg=p.nonneg, mode=mode, scalars=p.scal, squeeze=False)
    if not p.slices:
        return O.pd_tv_relaxed(x, seed=seed, return_counts=counts, fault=fault, **kw)
    assert x.ndim == 3 and fault is None
    res = [O.pd_tv_relaxed(x[k], seed=seed + 1000 * k, return_counts=True, **kw) for k in range(x.shape[0])]
    out = np.stack([r[0] for r in res])
    if not counts:
        return out
    return out, {key: sum(r[1][key] for r in res) for key in res[0][1]}


def model(x, p, counts=False, fault=None):
    """the relaxed model with every reciprocal square root on RN(1 / sqrt(x)); `counts`: also the branch counters"""
    return _run(x, p, "model", counts=counts, fault=fault)


def family(x, p):
    """(model, [ten members]): all one ulp down, all one ulp up, eight seeded patterns"""
    return model(x, p), [_run(x, p, "down"), _run(x, p, "up")] + [_run(x, p, "seeded", seed=s) for s in SEEDS]


def _dist(a, b):
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max()) if a.size else 0.0


def envelope(x, p, with_model=False):
    """B: the largest element-wise distance of any member from the model.  Where no voxel-iteration of the model takes
    nrm > 1 the members ARE the model (the offset is never read) and B = 0 without running them."""
    m, c = model(x, p, counts=True)
    if c["saturated"] == 0:
        B = 0.0
    else:
        B = max(_dist(v, m) for v in family(x, p)[1])
    return (B, m) if with_model else B


def ulp_of_max(m):
    """one unit in the last place of max|m| (float32)"""
    return float(np.spacing(np.float32(np.abs(m).max()))) if m.size else 0.0


def check_elementwise(got, x, p, what=""):
    """max|got - model| <= 4 B; with B = 0 that is bit equality.  Returns (distance, B)."""
    got = np.asarray(got, dtype=np.float32)
    B, m = envelope(x, p, with_model=True)
    got = got.reshape(m.shape)
    d = _dist(got, m)
    u = ulp_of_max(m)
    STATS.append((what, B / u if u else 0.0, (d / B) if B else None))
    if B == 0.0:
        if not np.array_equal(got.view(np.uint32), m.view(np.uint32)):
            bad = np.argwhere(got.view(np.uint32) != m.view(np.uint32))
            raise AssertionError((what, "the model has no hardware-dependent operation here: bit equality is required",
                                  f"{len(bad)} of {got.size} values differ, first at {tuple(bad[0])}", d))
        return d, B
    if not d <= MARGIN * B:
        at = np.unravel_index(int(np.argmax(np.abs(got.astype(np.float64) - m))), m.shape)
        raise AssertionError((what, f"max|got - model| = {d:.3e} at {tuple(int(i) for i in at)} > {MARGIN} B = {MARGIN * B:.3e}"))
    return d, B


def summary(mark, label):
    """one line over STATS[mark:]: how many comparisons were bit equality, the largest B and the largest |got - model| / B"""
    rows = STATS[mark:]
    env = [r for r in rows if r[2] is not None]
    line = f"PD_TV default vs relaxed model [{label}]: {len(rows)} comparisons, {len(rows) - len(env)} of them bit equality (B = 0)"
    if env:
        line += (f"; {len(env)} within the envelope: B up to {max(r[1] for r in env):.1f} ulp of max|model|, "
                 f"largest |got - model| / B = {max(r[2] for r in env):.2f} (bound {MARGIN})")
    return line


# ------------------------------------------------------------------------------------------------ one step, exactly
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def deduce_offsets(inp, u_in, p_in, p_out, scal, width=WIDTH, what=""):
    """One isotropic step from (u_in, p_in) gave the duals `p_out` (three arrays): per voxel, the offset in
    {0, -1, +1, ...} (|offset| <= width, 0 tried first, so every unsaturated voxel gets 0) under which all three of the
    model's dual components equal p_out's bits.  Where two offsets give the same bits the first tried is returned.  Raises
    with the coordinates of every voxel no candidate matches.  Returns (offsets int8, saturated int8)."""
    order = [0] + [s * k for k in range(1, width + 1) for s in (-1, 1)]
    shape = np.asarray(u_in).shape
    found = np.zeros(shape, bool)
    offs = np.zeros(shape, np.int8)
    sat = None
    for o in order:
        _, cand, sat = O.pd_step_relaxed(inp, u_in, p_in, *scal, 0, 0, offsets=np.full(shape, o, np.int8))
        hit = np.ones(shape, bool)
        for c in range(3):
            hit &= _bits(cand[c]) == _bits(p_out[c])
        new = hit & ~found
        offs[new] = o
        found |= hit
    if not found.all():
        bad = np.argwhere(~found)
        raise AssertionError((what, f"{len(bad)} of {found.size} voxels match no candidate within {width} ulp "
                                    f"({int((~found & (sat == 0)).sum())} of them unsaturated)", [tuple(int(i) for i in b) for b in bad]))
    return offs, sat


Trajectory = collections.namedtuple("Trajectory", "states offsets saturated")


def replay(x, p, n, step_fn, state=None, width=WIDTH, what=""):
    """n single isotropic 3D steps from `state` = (U, [P1, P2, P3]) (default: U = x, P = 0).  Every step runs
    step_fn(x, U, P) -> (U_out, [P_out]) (the GPU), deduces the offsets from P_out, runs the model step with them and asserts
    bit equality of U_out and P_out.  Returns Trajectory(states[0..n], offsets[0..n-1], saturated[0..n-1])."""
    assert not p.methodTV and not p.slices and np.asarray(x).ndim == 3
    x = np.ascontiguousarray(x, dtype=np.float32)
    U, P = (x.copy(), [np.zeros_like(x) for _ in range(3)]) if state is None else state
    states, history, sats = [(U, P)], [], []
    for i in range(n):
        u_gpu, p_gpu = step_fn(x, U, P)
        offs, sat = deduce_offsets(x, U, P, p_gpu, p.scal, width, (what, "step", i))
        u_m, p_m, _ = O.pd_step_relaxed(x, U, P, *p.scal, 0, p.nonneg, offsets=offs)
        for c in range(3):
            assert np.array_equal(_bits(p_m[c]), _bits(p_gpu[c])), (what, "step", i, "P", c)
        if not np.array_equal(_bits(u_m), _bits(u_gpu)):
            bad = np.argwhere(_bits(u_m) != _bits(np.asarray(u_gpu)))
            raise AssertionError((what, "step", i, f"U_out: {len(bad)} of {u_m.size} values differ from the model replayed "
                                                   f"with the hardware's own offsets, first at {tuple(bad[0])}"))
        U, P = u_m, p_m
        states.append((U, P))
        history.append(offs)
        sats.append(sat)
    return Trajectory(states, history, sats)


def offset_histogram(traj_or_pairs):
    """{offset: count} over the SATURATED voxel-steps of trajectories (or (offsets, saturated) pairs)"""
    hist = collections.Counter()
    items = traj_or_pairs if isinstance(traj_or_pairs, list) else [traj_or_pairs]
    for t in items:
        pairs = zip(t.offsets, t.saturated) if isinstance(t, Trajectory) else [t]
        for offs, sat in pairs:
            vals, cnt = np.unique(offs[sat != 0], return_counts=True)
            for v, k in zip(vals, cnt):
                hist[int(v)] += int(k)
    return dict(hist)


# ------------------------------------------------------------------------------------------------ inputs
def quiet(shape, seed=3):
    """noise of amplitude 1e-3 around zero (negative values for the clip, no ties): at lambda = 0.04 (sigma = 31.25) no dual
    leaves the unit ball in any of the iterations the tests run -- tests/test_pd_relaxed_oracle.py checks the counter"""
    rng = np.random.default_rng(seed)
    return ((rng.random(shape) - 0.5) * 2e-3).astype(np.float32)


def mixed(shape, seed=5):
    """inputs on which both branches of the projection are well populated and, with nonneg, the clip too.  The noise-on-a-step
    input of tests/_edge_shapes.py alone saturates 98-100 % of the voxel-iterations at lambda = 0.04 (sigma = 31.25 times a
    noise of amplitude 0.3), so it is mixed with `terraces`: terraces(scale = 0.25) + 0.1 (step_noise - 0.6).  Inside a
    terrace sigma |grad| straddles 1, at its edges it is far above; about half the values are negative.  Measured on the CPU
    over the shapes below and 1, 2, 3, 5, 6, 7 iterations: 12-88 % saturated, 45 % or more clipped."""
    import _edge_shapes as E
    return (E.terraces(shape, scale=0.25) + np.float32(0.1) * (E.step_noise(shape, seed) - np.float32(0.6))).astype(np.float32)


# ------------------------------------------------------------------------------------------------ what the GPU tests run
LAM = 0.04                       # the regularisation parameter of test_pdtv_vs_oracle / test_pdtv_edges
# pd_plan never leaves a remainder of 1 behind a fused launch (4 = 2 + 2, 7 = 3 + 2 + 2), so: 1 = the single-iteration march,
# 2 = K = 2 alone, 3 = K = 3 FIRST, 5 = 3 + 2 (FIRST, then the 2 x 4-wave K = 2 form on stored duals), 6 = 3 + 3 (FIRST, then
# the steady K = 3 form), 7 = 3 + 2 + 2 (a K = 2 launch that stores its duals and one that does not)
ITERS = (1, 2, 3, 5, 6, 7)


def chain_shape():
    """the local planes of one rank of SLABS["PD_TV"]: 2 m + 1 planes, three z-chunks in the K = 3 march"""
    import _edge_shapes as E
    s = E.SLABS["PD_TV"]
    return (s.shape[0] // s.world,) + tuple(s.shape[1:])


# one step, exactly: the chain's shape, and 2 x 2 workgroups of the single-iteration march plus one column / one row
STEP_SHAPES = (chain_shape(), (5, 17, 249))
# the chain: three z-chunks; and two workgroups in x and in y of both fused marches (116 / 120 columns, 16 rows) plus one
CHAIN_SHAPES = (chain_shape(), (4, 17, 121))
CHAIN_COUNTS = (7, 5)
# 2D and slice-wise, saturated: every x / y edge shape of pd_rows2d; the slice-wise shapes of tests/_slicewise_cases.py with
# at least seven rows and columns (a 2-wide image has no interior: every difference is a boundary rule)
def sat_2d_shapes():
    import _edge_shapes as E
    return sorted({c.shape for k in (1, 2, 3) for c in E.cases(f"pd_rows2d_k{k}")})


def sat_slice_shapes():
    import _slicewise_cases as S
    return sorted({s for s, _ in S.PD_CASES if min(s[1:]) >= 7})
