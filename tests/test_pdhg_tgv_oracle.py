"""PD_TGV in PDHG without a GPU: properties of the numpy restatement (tests/_pdhg_tgv_oracle.py; the algorithm is the
specification, docs/kernels/pdhg.md) on the inputs of tests/_pdhg_tgv_cases.py, and the host surface of the feature --
dictionary defaults, the refusals, the C-ABI's argument checks and scratch sizes (the library loads and validates without a
device)."""
import ctypes as C
import types

import numpy as np
import pytest

import _pdhg_cases as K
import _pdhg_diag_oracle as D
import _pdhg_oracle as P
import _pdhg_tgv_cases as T
import _pdhg_tgv_oracle as G


# ------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("name", list(T.CASES))
def test_float32_against_float64(name):
    """the float32 arithmetic the kernels reproduce holds the project's parity bar against the same algorithm in double
    (largest value seen: 1.1e-6, L1 + TGV after 300 iterations; docs/kernels/pdhg.md)"""
    f32, f64 = T.run(name, "float32", K.COUNTS)[0], T.run(name, "float64", K.COUNTS)[0]
    for n in K.COUNTS:
        r = G.rel_l2(f32[n], f64[n])
        print(f"PDHG {name} after {n}: float32 vs float64 rel-L2 = {r:.2e}")
        assert f32[n].dtype == np.float32 and f64[n].dtype == np.float64
        assert f32[n].shape == (K.NZ, K.N, K.N) and np.abs(f64[n]).max() > 0
        assert r <= 1e-5, (name, n, r)


@pytest.mark.parametrize("shape, bound", [((1, 9, 9), 12.0), ((6, 6, 6), 16.0)], ids=["2D", "3D"])
def test_block_norm_is_below_the_constant_of_the_step_sizes(shape, bound):
    """L_R: the squared norm of [[grad, -I], [0, E]] (measured: 11.08 on 9 x 9, 15.04 on 6 x 6 x 6)"""
    value = G.norm2(G.block_matrix(shape))
    print(f"|[[grad, -I], [0, E]]|^2 on {shape}: {value:.4f} (L_R = {bound})")
    assert 0.5 * bound < value <= bound, (shape, value)
    assert G.scalars(100.0, P.nd_of(shape))[0] == np.float32(0.95) / np.sqrt(np.float32(100.0) + np.float32(bound))


def test_block_matrix_is_the_operator_the_updates_apply():
    """the dense block against the stencils of the two updates: K (x, v) and K^T (p, q), off-diagonal Q counted twice"""
    shape = (3, 4, 5)
    rng = np.random.default_rng(5)
    x, v = rng.standard_normal(shape), [rng.standard_normal(shape) for _ in range(3)]
    zeros = [np.zeros(shape) for _ in range(3)]
    # sigma = 1 from zero duals with radii beyond reach: p = grad x - v, q = E v
    p, q = G.tgv_dual(x, v, zeros, [np.zeros(shape) for _ in range(6)], 1.0, 1.0, 1e9, 1e9)
    got = G.block_matrix(shape) @ np.concatenate([x.ravel()] + [c.ravel() for c in v])
    Q = dict(zip(G.qkeys(3), q))
    want = [c.ravel() for c in p] + [Q[min(d, e), max(d, e)].ravel() for d in (1, 2, 3) for e in (1, 2, 3)]
    assert np.allclose(got, np.concatenate(want), rtol=0, atol=1e-12)
    # tau = 1 from x = v = 0, g = 0: x' = div p = -grad^T p, v' = p + the backward differences of q = -(K^T (p, q))_v -- away
    # from the last index of an axis, where B_d keeps a[i] that the transpose of F_d (whose last row is 0) does not have
    xn, _, vn, _ = G.tgv_primal(np.zeros(shape), np.zeros(shape), zeros, p, q, 1.0, 1.0, False)
    back = (G.block_matrix(shape).T @ np.concatenate(want)).reshape((4,) + shape)
    for got_field, want_field in zip(back, [xn] + vn):
        assert np.allclose(got_field[:-1, :-1, :-1], -want_field[:-1, :-1, :-1], rtol=0, atol=1e-12)


def test_diagonal_steps_keep_the_preconditioned_norm_below_one():
    """|Sigma^1/2 K T^1/2|^2 <= c^2 = 0.9025 for the dense K = [A; block] of the 32 x 32 case (measured: 0.788)"""
    shape = (1, K.N, K.N)
    nd, nvox = 2, K.N * K.N
    A = K.dense().A
    Kmat = np.vstack([np.hstack([A, np.zeros((A.shape[0], nd * nvox))]), G.block_matrix(shape)])
    a, t, _, w = D.host_scalars(nd, True, 1.0, np.float64)
    sigma_p, sigma_q, tau_v = G.diag_scalars(nd, 1.0, np.float64)
    assert (sigma_p, sigma_q, tau_v) == (a / 3.0, a / 2.0, t / 5.0) and w == 4.0
    sigma = np.concatenate([D.diag_steps(np.abs(A).sum(1), a), np.full(nd * nvox, sigma_p), np.full(nd * nd * nvox, sigma_q)])
    tau = np.concatenate([D.diag_steps(np.abs(A).sum(0), t, w), np.full(nd * nvox, tau_v)])
    value = G.norm2(np.sqrt(sigma)[:, None] * Kmat * np.sqrt(tau)[None, :])
    print(f"|Sigma^1/2 K T^1/2|^2 = {value:.4f}")
    assert 0.5 < value <= 0.9025, value
    # Pock and Chambolle's lemma (alpha = 1) row by row and column by column: sigma_i sum_j |K_ij| <= c, tau_j sum_i |K_ij| <= c
    assert (sigma * np.abs(Kmat).sum(1)).max() <= 0.95 * (1 + 1e-12)
    assert (tau * np.abs(Kmat).sum(0)).max() <= 0.95 * (1 + 1e-12)


@pytest.mark.parametrize("name", list(T.CASES))
def test_z_constant_volume_gives_the_2d_bits_plane_for_plane(name):
    """z-terms come last in every sum: with the same L_K, nd = 3 on z-constant data is nd = 2 of one plane"""
    kw, positive = T.CASES[name]
    plane = np.ascontiguousarray(K.sinogram(1, positive=positive))
    stack = np.ascontiguousarray(np.broadcast_to(plane[0], (K.NZ,) + plane.shape[1:]))
    L_K = np.float32(K.lipschitz()) + np.float32(16)
    want = G.pdhg_tgv(K.matched(1), plane, None, 25, nd=2, L_K=L_K, **kw)
    got = G.pdhg_tgv(K.matched(K.NZ), stack, None, 25, nd=3, L_K=L_K, **kw)
    assert got.dtype == want.dtype == np.float32 and np.abs(want).max() > 0
    for z in range(K.NZ):
        assert np.array_equal(got[z].view(np.uint32), want[0].view(np.uint32)), z


@pytest.mark.parametrize("name", list(T.CASES))
def test_joint_objective_falls_along_the_checkpoints(name):
    kw, positive = T.CASES[name]
    b = K.sinogram(positive=positive)
    state, obj = {}, []
    for n, x in enumerate(G.pdhg_tgv_iterates(K.dense(), b, K.lipschitz(), iterations=max(K.CHECKPOINTS), dtype=np.float64,
                                              state=state, **kw), 1):
        if n in K.CHECKPOINTS:
            obj.append(G.objective(K.dense(), x, state["v"], b, kw["fidelity"], kw["lam"], kw["alpha1"], kw["alpha0"]))
    print(f"PDHG {name}: joint objective at {K.CHECKPOINTS} = {['%.8g' % v for v in obj]}")
    assert all(np.isfinite(obj))
    assert all(later < earlier for earlier, later in zip(obj, obj[1:])), obj


def test_tgv_beats_tv_on_ramps_and_plateaus():
    """a piecewise-affine phantom: after 1000 float64 iterations LS + TGV is closer to it than LS + TV for every lambda of
    the grid (measured: 0.02493 against 0.02794 at lambda = 0.25, a ratio of 0.892)"""
    tgv, tv = T.stair_errors()
    best = min(tv.values())
    print(f"staircase: LS + TGV error {tgv:.5f}; LS + TV errors {tv}; ratio {tgv / best:.3f}")
    assert min(tv, key=tv.get) not in (T.STAIR_TV_LAMBDAS[0], T.STAIR_TV_LAMBDAS[-1]), "the grid does not bracket TV's best lambda"
    assert tgv < best, (tgv, tv)


@pytest.mark.parametrize("name", list(T.CASES))
def test_diagonal_steps_reach_one_percent_sooner(name):
    """the first 2D float64 iterate within 1 % of the iterate after 6000 scalar-step iterations, looked for over 2500
    iterations (measured, scalar / diagonal: LS 1748 / 168, L1 none / 1362, KL 427 / 166).  Asserted with a margin of a quarter:
    diagonal <= 0.75 scalar, the scalar run counted as 2500 where it does not get there -- the least gain seen is below 0.55."""
    scalar, diagonal = T.iterations_to_one_percent(name)
    print(f"PDHG {name}: iterations to 1 %: scalar steps {scalar}, diagonal steps {diagonal}")
    assert diagonal is not None
    assert diagonal <= 0.75 * (T.RATE_LIMIT if scalar is None else scalar), (scalar, diagonal)


def test_kernel_test_inputs_exercise_both_branches_of_both_projections():
    """a condition on the INPUTS of the GPU tests: on the noise input each of the two projections of step 4 changes between
    10 % and 90 % of the voxels in the first step"""
    for shape in K.MARCH_SHAPES:
        for per_voxel in (False, True):
            for nonneg in (0, 1):
                res, shares = T.march_oracle("noise", shape, nonneg, per_voxel)
                assert all(0.1 <= s <= 0.9 for s in shares), (shape, shares)
        res, _ = T.march_oracle("terraces", shape, 1, False)
        assert all(np.isfinite(f["x"]).all() and np.isfinite(f["v"][0]).all() for f in res.values())
    assert len({float(T.MARCH_SIGMA_P), float(T.MARCH_SIGMA_Q), float(T.MARCH_TAU_X), float(T.MARCH_TAU_V)}) == 4


def test_scalars_are_float32_and_follow_the_specification():
    sp, sq, tx, tv = G.scalars(734.7, 3, 4.0)
    s = np.float32(0.95) / np.sqrt(np.float32(734.7) + np.float32(16))
    assert all(type(v) is np.float32 for v in (sp, sq, tx, tv))
    assert sp == sq == np.float32(s * np.float32(4)) and tx == tv == np.float32(s / np.float32(4))
    assert G.scalars(734.7, 2)[0] == np.float32(0.95) / np.sqrt(np.float32(734.7) + np.float32(12))
    r1, r0 = G.radii(0.3, 1.5, 2.5)
    assert (r1, r0) == (np.float32(0.3) * np.float32(1.5), np.float32(0.3) * np.float32(2.5))
    sp, sq, tv = G.diag_scalars(3, 4.0)
    a, t = np.float32(0.95) * np.float32(4), np.float32(0.95) / np.float32(4)
    assert (sp, sq, tv) == (a / np.float32(3), a / np.float32(2), t / np.float32(7))


# ------------------------------------------------------------------------------------------------ host surface
def _self(**kw):
    base = dict(Atools=types.SimpleNamespace(device_index=0), OS_number=1, slab=None, adjoint="matched", nonneg_regul=0)
    return types.SimpleNamespace(**dict(base, **kw))


def _dicts(data=None, algo=None, reg=None, method_run="PDHG", me=None):
    import torch
    import tomobar_amd.ops as ops
    from tomobar_amd.supp.dicts import dicts_check
    d = dict({"projection_data": torch.zeros((2, 3, 4), dtype=torch.float32)}, **(data or {}))
    keep = ops.to_device
    ops.to_device = lambda x, index: x   # no GPU here: the projections stay where they are
    try:
        return dicts_check(me or _self(), d, algo, reg, method_run=method_run)
    finally:
        ops.to_device = keep


def test_dicts_check_defaults():
    _, a, r = _dicts(reg={"method": "PD_TGV"})
    assert r == {"method": "PD_TGV", "regul_param": 0.001, "TGV_alpha1": 1.0, "TGV_alpha2": 2.0}   # nothing else is filled
    assert a["PDHG_ratio"] == 1.0 and a["PDHG_preconditioner"] is None
    _, a, r = _dicts({"data_fidelity": "KL"}, {"PDHG_preconditioner": "diagonal"},
                     {"method": "PD_TGV", "regul_param": 0.3, "TGV_alpha1": 0.5, "TGV_alpha2": 4.0, "methodTV": 7})
    assert (r["regul_param"], r["TGV_alpha1"], r["TGV_alpha2"]) == (0.3, 0.5, 4.0) and a["PDHG_preconditioner"] == "diagonal"
    assert r["methodTV"] == 7                    # not read: not even checked
    _, _, r = _dicts(reg={"method": "PD_TV"})    # and PD_TV is what it was
    assert r == {"method": "PD_TV", "regul_param": 0.001, "methodTV": 0}


PDHG_TEXT = r"PDHG takes _regularisation_\['method'\] = None or 'PD_TV' \(the TV term in its dual\) or 'PD_TGV' \(the TGV term in its dual\), not "
SPDHG_TEXT = r"SPDHG takes _regularisation_\['method'\] = None or 'PD_TV' \(the TV term in its dual\), not 'PD_TGV'"
REFUSED = [
    ("TGV", dict(reg={"method": "TGV"}), PDHG_TEXT + "'TGV'"),
    ("lower case", dict(reg={"method": "pd_tgv"}), PDHG_TEXT + "'pd_tgv'"),
    ("wavelets suffix", dict(reg={"method": "PD_TGV_WAVELETS"}), PDHG_TEXT + "'PD_TGV_WAVELETS'"),
    ("ROF_TV", dict(reg={"method": "ROF_TV"}), "None or 'PD_TV'"),
    ("SPDHG", dict(reg={"method": "PD_TGV"}, method_run="SPDHG"), SPDHG_TEXT),
    ("slicewise", dict(reg={"method": "PD_TGV", "slicewise": True}), "PDHG does not support slicewise=True"),
    ("half precision", dict(reg={"method": "PD_TGV", "half_precision": True}), "PDHG does not support half_precision=True"),
    ("lambda 0", dict(reg={"method": "PD_TGV", "regul_param": 0.0}), r"\['regul_param'\] must be positive"),
    ("alpha1 0", dict(reg={"method": "PD_TGV", "TGV_alpha1": 0.0}), r"\['TGV_alpha1'\] must be positive"),
    ("alpha2 negative", dict(reg={"method": "PD_TGV", "TGV_alpha2": -1.0}), r"\['TGV_alpha2'\] must be positive"),
    ("alpha2 nan", dict(reg={"method": "PD_TGV", "TGV_alpha2": float("nan")}), r"\['TGV_alpha2'\] must be positive"),
    ("z-slab", dict(reg={"method": "PD_TGV"}, me=_self(slab=object())), "z-slab"),
    ("ordered subsets", dict(reg={"method": "PD_TGV"}, me=_self(OS_number=4)), "ordered-subsets"),
]


@pytest.mark.parametrize("what, kw, text", REFUSED, ids=[r[0] for r in REFUSED])
def test_dicts_check_refusals(what, kw, text):
    with pytest.raises(ValueError, match=text):
        _dicts(**kw)


@pytest.mark.parametrize("driver", ["FISTA", "ADMM", "OSEM"])
def test_the_prox_drivers_still_read_the_string_as_the_tgv_prox(driver):
    from tomobar_amd.supp.regularisers import kind_of
    _, _, r = _dicts(reg={"method": "PD_TGV"}, method_run=driver)
    assert kind_of(r["method"]).name == "TGV" and r["TGV_alpha1"] == 1.0 and r["TGV_alpha2"] == 2.0 and "iterations" in r


# ------------------------------------------------------------------------------------------------ C-ABI
def test_scratch_bytes_is_the_placed_block_of_the_work_arrays():
    from tomobar_amd import _lib, ops
    lib = _lib.lib()
    skew = ops.ARRAY_SKEW
    for dx, dy, dz in [(37, 13, 7), (64, 64, 64), (1, 1, 1), (200, 150, 40)]:
        arr3 = (dx * dy * dz * 4 + 255) // 256 * 256
        arr2 = (dx * dy * 4 + 255) // 256 * 256
        assert lib.tomo_pdhg_tgv_scratch_bytes(dx, dy, dz, 3) == 17 * (arr3 + skew)   # x-bar, g, P, v, v-bar (3 each), Q (6)
        assert lib.tomo_pdhg_tgv_scratch_bytes(dx, dy, dz, 2) == 11 * (arr2 + skew)   # dz is ignored in 2D
        assert lib.tomo_pdhg_tgv_diag_scratch_bytes(dx, dy, dz, 3) == 18 * (arr3 + skew)
        assert lib.tomo_pdhg_tgv_diag_scratch_bytes(dx, dy, dz, 2) == 12 * (arr2 + skew)


def test_invalid_arguments_are_refused_before_the_device_is_touched():
    from tomobar_amd import _lib
    lib = _lib.lib()
    a = [0x1000 * k for k in range(1, 21)]   # never dereferenced: every case fails validation
    x, xb, g, tau = a[0], a[1], a[2], a[3]
    v, vb, p, q = a[4:7], a[7:10], a[10:13], a[13:19]
    arr = lambda ptrs: None if ptrs is None else (C.c_void_p * len(ptrs))(*ptrs)  # noqa: E731
    vp = C.c_void_p

    def dual(xb=xb, vb=vb, p=p, q=q, dx=4, dy=4, dz=4, nd=3, sp=0.5, sq=0.25, r1=1.0, r0=2.0):
        return lib.tomo_pdhg_tgv_dual(0, vp(xb), arr(vb), arr(p), arr(q), dx, dy, dz, nd, sp, sq, r1, r0, None)

    def primal(x=x, xb=xb, g=g, v=v, vb=vb, p=p, q=q, dx=4, dy=4, dz=4, nd=3, tx=0.5, tv=0.25):
        return lib.tomo_pdhg_tgv_primal(0, vp(x), vp(xb), vp(g), arr(v), arr(vb), arr(p), arr(q), dx, dy, dz, nd, tx, tv, 0, None)

    def diag(x=x, xb=xb, g=g, tau=tau, v=v, vb=vb, p=p, q=q, dx=4, dy=4, dz=4, nd=3, tv=0.25):
        return lib.tomo_pdhg_tgv_primal_diag(0, vp(x), vp(xb), vp(g), vp(tau), arr(v), arr(vb), arr(p), arr(q), dx, dy, dz, nd, tv, 0, None)

    swap = lambda group, k, value: group[:k] + [value] + group[k + 1:]  # noqa: E731
    bad = [(dual, dict(nd=1)), (dual, dict(nd=4)), (dual, dict(dx=0)), (dual, dict(dy=-1)), (dual, dict(dz=0)),
           (dual, dict(dx=1 << 15, dy=1 << 14)),                                 # the 2^29 plane limit
           (dual, dict(sp=0.0)), (dual, dict(sq=-1.0)), (dual, dict(sq=float("nan"))), (dual, dict(r1=0.0)), (dual, dict(r0=float("inf"))),
           (dual, dict(xb=0)), (dual, dict(vb=None)), (dual, dict(p=swap(p, 2, 0))), (dual, dict(q=swap(q, 5, 0))),
           (dual, dict(q=swap(q, 3, q[0]))), (dual, dict(p=swap(p, 0, xb))), (dual, dict(q=swap(q, 1, vb[2]))), (dual, dict(p=swap(p, 1, q[4]))),
           (primal, dict(nd=5)), (primal, dict(dx=0)), (primal, dict(dx=1 << 15, dy=1 << 14)),
           (primal, dict(tx=0.0)), (primal, dict(tv=0.0)), (primal, dict(tx=float("inf"))), (primal, dict(tv=float("nan"))),
           (primal, dict(x=0)), (primal, dict(g=0)), (primal, dict(v=None)), (primal, dict(q=swap(q, 4, 0))),
           (primal, dict(xb=x)), (primal, dict(g=xb)), (primal, dict(v=swap(v, 1, x))), (primal, dict(vb=swap(vb, 0, v[0]))),
           (primal, dict(p=swap(p, 2, xb))), (primal, dict(q=swap(q, 5, vb[1]))), (primal, dict(q=swap(q, 2, g))),
           (diag, dict(tau=0)), (diag, dict(tau=x)), (diag, dict(tau=xb)), (diag, dict(tau=g)), (diag, dict(tau=v[2])), (diag, dict(tau=q[0])),
           (diag, dict(tv=0.0)), (diag, dict(nd=0)), (diag, dict(vb=swap(vb, 2, 0)))]
    for fn, kw in bad:
        assert fn(**kw) == _lib.E_INVALID, (fn.__name__, kw)
        with pytest.raises(ValueError):
            _lib.check(fn(**kw))
