"""MI355X tests of SPDHG: the four shipped kernels and the driver against the float32 numpy restatement
tests/_spdhg_oracle.py, bit for bit (there is no reference implementation: formula-level parity, unpinned;
docs/kernels/spdhg.md), on the inputs of tests/_spdhg_cases.py and tests/_pdhg_cases.py."""
import os
import sys
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _cupy_standin  # noqa: E402
from _gpu_compare import host, same_bits  # noqa: E402
from _guarded import guarded  # noqa: E402
import _pdhg_cases as K  # noqa: E402
import _pdhg_driver_geometries as GEO  # noqa: E402
import _pdhg_oracle as P  # noqa: E402
import _spdhg_cases as SK  # noqa: E402
import _spdhg_oracle as S  # noqa: E402


# ------------------------------------------------------------------------------------------------ subset step 2
SINO_EXTENTS = [(1,), (3,), (63,), (64,), (65,), (4099,), (5, 23, 48)]


def _sino_inputs(shape):
    rng = np.random.default_rng(41)
    y = (2.0 * rng.standard_normal(shape)).astype(np.float32)      # reaches beyond +-1: the L1 clip
    r = rng.uniform(-1.0, 9.0, shape).astype(np.float32)
    b = rng.uniform(-2.0, 8.0, shape).astype(np.float32)           # negative entries: the KL clamp
    return y, r, b


@pytest.mark.parametrize("sigma", [0.035, 1.5])
@pytest.mark.parametrize("fidelity", P.FIDELITIES)
@pytest.mark.parametrize("shape", SINO_EXTENTS, ids=lambda s: "x".join(map(str, s)))
def test_sino_dual_equals_the_oracle(shape, fidelity, sigma):
    from tomobar_amd import ops
    y, r, b = _sino_inputs(shape)
    sigma = np.float32(sigma)
    want_y, want_d = S.sino_step(y, r, b, fidelity, sigma)
    assert want_y.dtype == want_d.dtype == np.float32
    if fidelity == "L1" and y.size > 8:
        assert (np.abs(want_y) == 1).any() and (np.abs(want_y) < 1).any()
    yg, rg, bg = guarded(y), guarded(r), guarded(b)
    yd, rd, bd = yg.view, rg.view, bg.view
    out = ops.spdhg_sino_dual(yd, rd, bd, fidelity, sigma)
    assert out[0] is yd and out[1] is rd
    same_bits(host(yd), want_y, (shape, fidelity, float(sigma), "y"))
    same_bits(host(rd), want_d, (shape, fidelity, float(sigma), "d"))
    assert yg.intact() and rg.intact() and bg.intact() and bg.unchanged()
    # a second application on a fresh projection: the dual is really updated in place
    r2 = (r[::-1] if r.ndim == 1 else r[::-1, ::-1]).copy()
    rd.copy_(torch.from_numpy(r2))
    ops.spdhg_sino_dual(yd, rd, bd, fidelity, sigma)
    want_y2, want_d2 = S.sino_step(want_y, r2, b, fidelity, sigma)
    same_bits(host(yd), want_y2, (shape, fidelity, "second application", "y"))
    same_bits(host(rd), want_d2, (shape, fidelity, "second application", "d"))
    assert yg.intact() and rg.intact() and bg.intact() and bg.unchanged()


@pytest.mark.parametrize("fidelity", P.FIDELITIES)
def test_sino_dual_on_arrays_that_are_not_16_byte_aligned(fidelity):
    """the scalar form: every array starts 4 bytes past a 16-byte boundary"""
    from tomobar_amd import ops
    y, r, b = _sino_inputs((4100,))
    sigma = np.float32(0.4)
    yg, rg, bg = (guarded(a, shift=1) for a in (y, r, b))
    yd, rd, bd = yg.view, rg.view, bg.view
    assert all(t.data_ptr() % 16 == 4 and t.is_contiguous() for t in (yd, rd, bd))
    ops.spdhg_sino_dual(yd, rd, bd, fidelity, sigma)
    want_y, want_d = S.sino_step(y, r, b, fidelity, sigma)
    same_bits(host(yd), want_y, (fidelity, "y"))
    same_bits(host(rd), want_d, (fidelity, "d"))
    assert yg.intact() and rg.intact() and bg.intact() and bg.unchanged()


# ------------------------------------------------------------------------------------------------ subset step 4
PRIMAL_EXTENTS = [(1,), (63,), (64,), (65,), (4099,), (5, 13, 37)]


def _primal_inputs(shape):
    rng = np.random.default_rng(53)
    x = rng.standard_normal(shape).astype(np.float32)
    z = (3.0 * rng.standard_normal(shape)).astype(np.float32)
    delta = (2.0 * rng.standard_normal(shape)).astype(np.float32)
    return x, z, delta


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("w", SK.PRIMAL_WEIGHTS, ids=lambda w: f"w{int(w)}")
@pytest.mark.parametrize("nonneg", [0, 1])
@pytest.mark.parametrize("shape", PRIMAL_EXTENTS, ids=lambda s: "x".join(map(str, s)))
def test_streaming_primal_equals_the_oracle(shape, nonneg, w, shift):
    from tomobar_amd import ops
    x, z, delta = _primal_inputs(shape)
    tau = np.float32(0.05)
    want_x, want_z = S.primal_step(x, z, delta, tau, w, nonneg)
    if x.size > 8:   # a condition on the inputs: the clamp acts on some voxels and not on others
        free = S.primal_step(x, z, delta, tau, w, 0)[0]
        assert (free < 0).any() and (free > 0).any()
    xg, zg, dg = (guarded(a, shift=shift) for a in (x, z, delta))
    xd, zd, dd = xg.view, zg.view, dg.view
    assert all(t.data_ptr() % 16 == 4 * shift for t in (xd, zd, dd))
    ops.spdhg_primal(xd, zd, dd, tau, w, nonneg)
    same_bits(host(xd), want_x, (shape, nonneg, float(w), "x"))
    same_bits(host(zd), want_z, (shape, nonneg, float(w), "z"))
    assert xg.intact() and zg.intact() and dg.intact() and dg.unchanged()
    ops.spdhg_primal(xd, zd, dd, tau, w, nonneg)
    want_x, want_z = S.primal_step(want_x, want_z, delta, tau, w, nonneg)
    same_bits(host(xd), want_x, (shape, nonneg, float(w), "second application", "x"))
    same_bits(host(zd), want_z, (shape, nonneg, float(w), "second application", "z"))


# ------------------------------------------------------------------------------------------------ the TV update
@pytest.mark.parametrize("shape", K.MARCH_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tv_pair_equals_the_oracle(shape):
    from tomobar_amd import ops
    nd = 3 if shape[0] > 1 else 2
    z0 = SK.tv_z0(shape)
    for kind in ("noise", "terraces"):
        x0 = K.march_input(kind, shape)
        lam = K.MARCH_LAMBDA[kind]
        for methodTV in (0, 1):
            for nonneg in (0, 1):
                want, share = SK.tv_oracle(kind, shape, methodTV, nonneg)
                if kind == "noise":   # a condition on the inputs: both branches of the projection run
                    assert 0.1 <= share <= 0.9, (shape, methodTV, share)
                xg, zg = guarded(x0), guarded(z0)
                x, z = xg.view, zg.view
                qs = [guarded(np.zeros(shape, np.float32)) for _ in range(nd)]
                es = [guarded(np.full(shape, 7.0, np.float32)) for _ in range(nd)]   # e is written, never read first
                q, e = [b.view for b in qs], [b.view for b in es]
                for n in range(1, max(K.MARCH_COUNTS) + 1):
                    ops.spdhg_tv_dual(x, q, e, K.MARCH_SIGMA, lam, methodTV)
                    if n == 1:
                        same_bits(host(x), x0, (shape, kind, "the dual launch wrote x"))
                    ops.spdhg_tv_primal(x, z, e, K.MARCH_TAU, SK.TV_W, nonneg)
                    if n in K.MARCH_COUNTS:
                        what = (shape, kind, methodTV, nonneg, n)
                        wx, wz, wq, we = want[n]
                        same_bits(host(x), wx, what + ("x",))
                        same_bits(host(z), wz, what + ("z",))
                        for d in range(nd):
                            same_bits(host(q[d]), wq[d], what + (f"q{d + 1}",))
                            same_bits(host(e[d]), we[d], what + (f"e{d + 1}",))
                assert all(b.intact() for b in [xg, zg] + qs + es), (shape, kind, "a guard was written")


# ------------------------------------------------------------------------------------------------ refusals, the block
def test_wrappers_refuse_what_they_cannot_run():
    from tomobar_amd import ops
    y, r, b = (torch.zeros(8, device="cuda") for _ in range(3))
    with pytest.raises(ValueError, match="LS, L1 and KL"):
        ops.spdhg_sino_dual(y, r, b, "PWLS", 0.5)
    with pytest.raises(ValueError, match="size"):
        ops.spdhg_sino_dual(y, r[:4], b, "LS", 0.5)
    with pytest.raises(ValueError, match="sigma"):
        ops.spdhg_sino_dual(y, r, b, "LS", 0.0)
    with pytest.raises(ValueError, match="alias"):
        ops.spdhg_sino_dual(y, y, b, "LS", 0.5)
    with pytest.raises(ValueError, match="alias"):
        ops.spdhg_sino_dual(y, r, r, "LS", 0.5)
    with pytest.raises(ValueError, match="float32"):
        ops.spdhg_sino_dual(y, r.double(), b, "LS", 0.5)
    x, z, dl, q1, q2, q3, e1, e2, e3 = (torch.zeros((3, 4, 5), device="cuda") for _ in range(9))
    with pytest.raises(ValueError, match="tau"):
        ops.spdhg_primal(x, z, dl, 0.0, 4.0)
    with pytest.raises(ValueError, match="weight"):
        ops.spdhg_primal(x, z, dl, 0.1, 0.0)
    with pytest.raises(ValueError, match="alias"):
        ops.spdhg_primal(x, x, dl, 0.1, 4.0)
    with pytest.raises(ValueError, match="size"):
        ops.spdhg_primal(x, z, dl[:2], 0.1, 4.0)
    with pytest.raises(ValueError, match="3 dual fields"):
        ops.spdhg_tv_dual(x, [q1, q2], [e1, e2, e3], 0.25, 1.0)
    with pytest.raises(ValueError, match="3 dual fields"):
        ops.spdhg_tv_dual(x, [q1, q2, q3], [e1, e2], 0.25, 1.0)
    with pytest.raises(ValueError, match="lambda"):
        ops.spdhg_tv_dual(x, [q1, q2, q3], [e1, e2, e3], 0.25, 0.0)
    with pytest.raises(ValueError, match="sigma"):
        ops.spdhg_tv_dual(x, [q1, q2, q3], [e1, e2, e3], -0.25, 1.0)
    with pytest.raises(ValueError, match="alias"):
        ops.spdhg_tv_dual(x, [q1, q2, q1], [e1, e2, e3], 0.25, 1.0)
    with pytest.raises(ValueError, match="alias"):
        ops.spdhg_tv_dual(x, [q1, q2, q3], [e1, e2, q3], 0.25, 1.0)
    with pytest.raises(ValueError, match="methodTV"):
        ops.spdhg_tv_dual(x, [q1, q2, q3], [e1, e2, e3], 0.25, 1.0, 2)
    with pytest.raises(ValueError, match="shape"):
        ops.spdhg_tv_dual(x, [q1, q2, q3[:2]], [e1, e2, e3], 0.25, 1.0)
    with pytest.raises(ValueError, match="3 dual fields"):
        ops.spdhg_tv_primal(x, z, [e1, e2], 0.25, 2.0)
    with pytest.raises(ValueError, match="alias"):
        ops.spdhg_tv_primal(x, z, [e1, e2, z], 0.25, 2.0)
    with pytest.raises(ValueError, match="alias"):
        ops.spdhg_tv_primal(x, x, [e1, e2, e3], 0.25, 2.0)
    with pytest.raises(ValueError, match="shape"):
        ops.spdhg_tv_primal(x, z[:2], [e1, e2, e3], 0.25, 2.0)
    with pytest.raises(ValueError, match="tau"):
        ops.spdhg_tv_primal(x, z, [e1, e2, e3], float("nan"), 2.0)
    with pytest.raises(ValueError, match="weight"):
        ops.spdhg_tv_primal(x, z, [e1, e2, e3], 0.25, -2.0)
    torch.cuda.synchronize()
    assert all(float(t.abs().max()) == 0.0 for t in (y, r, b, x, z, dl, q1, q2, q3, e1, e2, e3))   # nothing was launched


def test_work_arrays_come_from_one_placed_block_of_the_stated_size():
    from tomobar_amd import _lib, ops
    shape = (5, 13, 37)
    z, delta, q, e, lease = ops.spdhg_work_arrays(shape, "cuda:0", True)
    arrs = [z, delta] + q + e
    assert len(q) == len(e) == 3
    assert all(tuple(a.shape) == shape and a.dtype == torch.float32 and a.is_contiguous() for a in arrs)
    step = (5 * 13 * 37 * 4 + 255) // 256 * 256 + ops.ARRAY_SKEW
    assert [a.data_ptr() - z.data_ptr() for a in arrs] == [k * step for k in range(8)] and z.data_ptr() % 256 == 0
    assert _lib.lib().tomo_spdhg_scratch_bytes(37, 13, 5, 3) == 8 * step
    assert ops.lease_is_current(lease)
    # a block of its own: PDHG's work arrays do not supersede it
    ops.pdhg_work_arrays(shape, "cuda:0", True)
    assert ops.lease_is_current(lease)
    _, _, q2, e2, lease2 = ops.spdhg_work_arrays((1, 13, 37), "cuda:0", True)
    assert len(q2) == len(e2) == 2 and not ops.lease_is_current(lease) and ops.lease_is_current(lease2)
    assert ops.spdhg_work_arrays(shape, "cuda:0", False)[2:4] == ([], [])


# ------------------------------------------------------------------------------------------------ the driver
LABELS = GEO.LABELS
EPOCHS = 6
TV = {"method": "PD_TV", "regul_param": 0.002}


class Geometry(GEO.Geometry):
    def tools(self, OS_number, adjoint="matched"):
        from tomobar_amd.methodsIR_CuPy import RecToolsIRCuPy
        return RecToolsIRCuPy(self.n, self.pad, self.nz if self.nz > 1 else None, 0.0, self.angles, self.n, 0,
                              OS_number, adjoint=adjoint)

    def projector(self, m):
        return S.matched(self.nz, self.size, self.size, self.angles, m)


@pytest.fixture(scope="module")
def geometries(oracle, golden_dir):
    """the geometries of tests/test_gpu_pdhg.py: `golden` (4 x 24^2, its padded and 2D forms) and `n48` (5 x 48^2, 23 angles:
    uneven subsets, the trim rule acts); L_A bounds the whole operator, hence every subset's"""
    return GEO.build(oracle, golden_dir, Geometry)


def _x0(shape):
    """a start with negative voxels: with nonnegativity the initial clamp acts"""
    return (0.05 * np.random.default_rng(47).random(shape) - 0.02).astype(np.float32)


# name -> (geometry, OS_number, _data_ keys, _algorithm_ keys, _regularisation_)
DRIVER_CASES = {
    "LS+TV nonneg OS4": ("golden", 4, {}, {"nonnegativity": True}, TV),
    "L1+aniso OS4 48": ("n48", 4, {"data_fidelity": "L1"}, {}, {"method": "PD_TV", "regul_param": 0.02, "methodTV": 1}),
    "KL+TV nonneg OS3": ("golden", 3, {"data_fidelity": "KL"}, {"nonnegativity": True}, {"method": "PD_TV", "regul_param": 0.001}),
    "no regulariser OS6": ("n48", 6, {}, {}, None),
    "OS1+TV": ("golden", None, {}, {}, TV),
    "initialise": ("golden", 4, {}, {"initialise": "x0", "nonnegativity": True}, TV),
    "ratio 4": ("n48", 4, {"data_fidelity": "L1"}, {"PDHG_ratio": 4}, {"method": "PD_TV", "regul_param": 0.02}),
    "seed 7": ("golden", 4, {}, {"SPDHG_seed": 7}, TV),
    "mask 0.85": ("golden", 4, {}, {"recon_mask_radius": 0.85}, TV),
    "detector padding": ("golden_pad", 4, {}, {}, TV),
    "2D": ("golden_2d", 3, {"data_fidelity": "KL"}, {}, {"method": "PD_TV", "regul_param": 0.002, "methodTV": 1}),
}


def _oracle_kw(geo, d, a, r):
    x0 = _x0((geo.nz, geo.size, geo.size)) if a.get("initialise") == "x0" else None
    return dict(fidelity=d.get("data_fidelity", "LS"), lam=None if r is None else r["regul_param"],
                methodTV=0 if r is None else r.get("methodTV", 0), nonneg=a.get("nonnegativity", False),
                ratio=a.get("PDHG_ratio", 1.0), x0=x0, seed=a.get("SPDHG_seed", 0))


def _oracle_run(oracle, geo, os_number, d, a, r, iterations=EPOCHS, L=None, state=None):
    m = os_number or 1
    b = oracle.pad_detector(geo.sino, geo.pad)
    x = S.spdhg(geo.projector(m), b, geo.L_A if L is None else L, m, iterations, state=state, **_oracle_kw(geo, d, a, r))
    if geo.pad:
        return np.ascontiguousarray(oracle.crop_recon(x, geo.n))     # a cropped result is not masked
    radius = a.get("recon_mask_radius")
    return x if radius is None else oracle.circular_mask(x, radius).astype(np.float32)


def _algorithm(geo, a, **kw):
    algo = dict({"iterations": EPOCHS, "lipschitz_const": geo.L_A, "recon_mask_radius": None}, **a)
    if algo.get("initialise") == "x0":
        algo["initialise"] = torch.from_numpy(_x0((geo.nz, geo.size, geo.size))).cuda()
    return dict(algo, **kw)


@pytest.mark.parametrize("name", list(DRIVER_CASES))
def test_driver_equals_the_oracle_loop(name, geometries, oracle):
    gname, os_number, d, a, r = DRIVER_CASES[name]
    geo = geometries[gname]
    state = {}
    want = _oracle_run(oracle, geo, os_number, d, a, r, state=state)
    rt = geo.tools(os_number)
    data = geo.data(**d)
    given = data["projection_data"]
    got = rt.SPDHG(data, _algorithm(geo, a), None if r is None else dict(r))
    assert isinstance(got, torch.Tensor) and tuple(got.shape) == (geo.nz, geo.n, geo.n)
    assert rt.Atools.kernel_path("bp").startswith("matched")
    run = rt.last_run
    assert run["method"] == "SPDHG" and run["iterations_done"] == EPOCHS and not run["converged"]
    assert run["block_updates"] == state["block_updates"] and sum(run["block_updates"]) == EPOCHS * S.n_blocks(os_number or 1, r is not None)
    assert np.abs(want).max() > 0
    same_bits(host(got), want, name)
    assert np.array_equal(host(given), geo.sino), "the caller's projection data must not be written"
    if name == "initialise":   # a condition on the input: the initial clamp acted
        assert (_x0(want.shape) < 0).any()


def test_the_subsets_of_n48_are_uneven(geometries):
    """a condition on the input: 23 angles in 4 and 6 subsets leave subsets of different sizes (the trim rule acts)"""
    geo = geometries["n48"]
    for m in (4, 6):
        A = geo.tools(m).Atools
        sizes = [A.sino_shape(j)[1] for j in range(m)]
        assert len(set(sizes)) == 2 and sum(sizes) == 23, sizes
        assert [len(idx) for idx in geo.projector(m).subsets] == sizes


def test_another_seed_is_another_run(geometries, oracle):
    gname, os_number, d, a, r = DRIVER_CASES["seed 7"]
    geo = geometries[gname]
    assert not np.array_equal(S.draws(7, 4, True, EPOCHS), S.draws(0, 4, True, EPOCHS))
    seven = host(geo.tools(os_number).SPDHG(geo.data(), _algorithm(geo, a), dict(r)))
    zero = host(geo.tools(os_number).SPDHG(geo.data(), _algorithm(geo, {}), dict(r)))
    again = host(geo.tools(os_number).SPDHG(geo.data(), _algorithm(geo, {"SPDHG_seed": 0}), dict(r)))
    assert not np.array_equal(seven, zero)
    assert np.array_equal(zero, again)


def test_lipschitz_constant_is_the_largest_power_method_value_of_the_subsets(geometries, oracle):
    geo = geometries["golden"]
    rt = geo.tools(4)
    rt.power_seed = 5
    values = [rt._power_iterations(j) for j in range(4)]
    assert rt.powermethod({"projection_data": None}) == values[0]     # the public method keeps returning subset 0's
    assert len(set(values)) > 1 and all(v > 0 for v in values)
    algo = {"iterations": 2, "recon_mask_radius": None}
    got = rt.SPDHG(geo.data(), algo, dict(TV))
    assert algo["lipschitz_const"] == max(values)
    want = _oracle_run(oracle, geo, 4, {}, {}, TV, iterations=2, L=max(values))
    same_bits(host(got), want, "power method")


def test_a_run_stopped_by_the_tolerance_is_the_run_of_that_many_epochs(geometries, oracle):
    geo = geometries["golden"]
    gname, os_number, d, a, r = DRIVER_CASES["LS+TV nonneg OS4"]
    total = 16
    its = S.spdhg_many(geo.projector(os_number), geo.sino, geo.L_A, os_number, range(1, total + 1), **_oracle_kw(geo, d, a, r))
    from _tgv_oracle import rel_d
    seq = [rel_d(its[1], np.zeros_like(its[1]))] + [rel_d(its[k], its[k - 1]) for k in range(2, total + 1)]
    j = 12
    tol = float(np.sqrt(seq[j - 2] * seq[j - 1]))
    stop = next(k for k, v in enumerate(seq, 1) if v < tol)
    # conditions on the input: the run stops inside the loop and no value lies within 1 % of the threshold
    assert 3 <= stop < total and all(abs(v - tol) >= 0.01 * tol for v in seq), (stop, tol, seq)
    rt = geo.tools(os_number)
    got = host(rt.SPDHG(geo.data(**d), _algorithm(geo, a, iterations=total, tolerance=tol), dict(r)))
    run = rt.last_run
    print(f"SPDHG tolerance {tol:.4e}: stopped after {run['iterations_done']} epochs (oracle {stop})")
    assert run["converged"] and run["iterations_done"] == stop and len(run["rel_change"]) == stop
    assert sum(run["block_updates"]) == stop * S.n_blocks(os_number, True)
    plain = host(geo.tools(os_number).SPDHG(geo.data(**d), _algorithm(geo, a, iterations=stop), dict(r)))
    assert np.array_equal(got, plain)
    same_bits(got, its[stop], "stopped run against the oracle")


def test_refusals_on_a_real_object(geometries):
    geo = geometries["golden"]
    algo = {"iterations": 2, "lipschitz_const": geo.L_A}
    with pytest.raises(ValueError, match='construct with adjoint="matched"'):
        geo.tools(4, adjoint="unmatched").SPDHG(geo.data(), dict(algo))
    rt = geo.tools(4)
    rt.slab = types.SimpleNamespace(world=2, rank=0)
    with pytest.raises(ValueError, match="z-slab"):
        rt.SPDHG(geo.data(), dict(algo))
    rt = geo.tools(4)
    for d, reg, text in (({"data_fidelity": "PWLS"}, None, "PWLS"), ({"data_fidelity": "SWLS"}, None, "SWLS"),
                         ({"ringGH_lambda": 0.01}, None, "ringGH_lambda"), ({"huber_threshold": 1.0}, None, "huber_threshold"),
                         ({"studentst_threshold": 1.0}, None, "studentst_threshold"),
                         ({}, {"method": "ROF_TV"}, "None or 'PD_TV'"), ({}, {"method": "PD_TV_WAVELETS"}, "None or 'PD_TV'"),
                         ({}, {"method": "NLTV"}, "None or 'PD_TV'"),
                         ({}, {"method": "PD_TV", "slicewise": True}, "slicewise"),
                         ({}, {"method": "PD_TV", "half_precision": True}, "half_precision")):
        with pytest.raises(ValueError, match=text):
            rt.SPDHG(geo.data(**d), dict(algo), reg)
    with pytest.raises(ValueError, match="SPDHG_seed"):
        rt.SPDHG(geo.data(), dict(algo, SPDHG_seed=-1))
    with pytest.raises(ValueError, match="should be provided as 'LS', 'PWLS', 'KL'"):
        rt.FISTA(geo.data(data_fidelity="L1"), dict(algo))
    # PDHG keeps refusing the subsets, with its own message
    with pytest.raises(ValueError, match="There is no ordered-subsets implementation of PDHG, please set OS_number=None"):
        rt.PDHG(geo.data(), dict(algo))
    # the object still reconstructs afterwards
    assert np.isfinite(host(rt.SPDHG(geo.data(), dict(algo)))).all()


def test_layouts_are_planar_again_after_a_call_that_raises_inside_the_loop(geometries, monkeypatch):
    from tomobar_amd import ops
    geo = geometries["golden"]
    rt = geo.tools(4)
    A = rt.Atools
    algo = {"iterations": 4, "lipschitz_const": geo.L_A, "recon_mask_radius": None}
    want = host(rt.SPDHG(geo.data(), dict(algo), dict(TV)))
    real, calls = ops.spdhg_primal, []

    def failing(*args, **kw):
        calls.append(1)
        if len(calls) == 2:
            raise RuntimeError("stop here")
        return real(*args, **kw)

    monkeypatch.setattr(ops, "spdhg_primal", failing)
    A.set_volume_layout("zquad", require_ok=False)       # what an interrupted driver could have left behind
    with pytest.raises(RuntimeError, match="stop here"):
        rt.SPDHG(geo.data(), dict(algo), dict(TV))
    assert len(calls) == 2
    assert A.residual_layout() == "planar" and A.volume_layout() == "planar"
    monkeypatch.setattr(ops, "spdhg_primal", real)
    assert np.array_equal(host(rt.SPDHG(geo.data(), dict(algo), dict(TV))), want)


def test_a_cupy_caller_gets_cupy_back(geometries, monkeypatch):
    cupy = _cupy_standin.install(monkeypatch)
    geo = geometries["golden"]
    rt = geo.tools(4)
    algo = {"iterations": 3, "lipschitz_const": geo.L_A}
    sino_t = torch.from_numpy(geo.sino.copy()).cuda()
    keep = sino_t.clone()
    want = rt.SPDHG({"projection_data": sino_t, "data_axes_labels_order": list(LABELS)}, dict(algo), dict(TV))
    res = rt.SPDHG({"projection_data": cupy.ndarray(sino_t), "data_axes_labels_order": list(LABELS)}, dict(algo), dict(TV))
    assert isinstance(want, torch.Tensor)
    assert type(res) is cupy.ndarray and res.shape == (geo.nz, geo.n, geo.n) and res.dtype == np.float32
    assert np.array_equal(res.get(), host(want))
    assert torch.equal(sino_t, keep), "the caller's projection data must not be written"
