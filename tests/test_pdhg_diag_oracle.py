"""PDHG with the diagonal preconditioner, without a GPU: properties of the numpy restatement (tests/_pdhg_diag_oracle.py; the
algorithm is the specification, docs/kernels/pdhg.md) on the inputs of tests/_pdhg_cases.py, and the host surface of the
feature -- the key, its refusals, what the driver calls with and without it, the C-ABI's argument checks."""
import ctypes as C
import functools
import types

import numpy as np
import pytest

import _pdhg_call_log as CALLS
import _pdhg_cases as K
import _pdhg_diag_oracle as D
import _pdhg_oracle as P


# ------------------------------------------------------------------------------------------------ step validity
@pytest.mark.parametrize("tv", [True, False], ids=["TV", "no TV"])
@pytest.mark.parametrize("ratio", [1.0, 4.0])
def test_steps_satisfy_the_convergence_condition(ratio, tv):
    """|Sigma^(1/2) K T^(1/2)|^2 <= c^2 = 0.9025 for the dense K = [A; grad] of the 32 x 32 2D case: a condition (Pock and
    Chambolle 2011, lemma 2 with alpha = 1), not a measurement"""
    shape, sino_shape = (1, K.N, K.N), (1, K.NA, K.NU)
    sigma, tau, sigma_G = D.step_arrays(K.dense(), sino_shape, shape, 2, tv, ratio, np.float64)
    rows, steps = [K.dense().A], [sigma.ravel()]
    if tv:
        G = D.gradient_matrix(shape)
        assert G.shape == (2 * K.N * K.N, K.N * K.N) and np.abs(G).sum(axis=1).max() == 2 and np.abs(G).sum(axis=0).max() == 4
        rows.append(G)
        steps.append(np.full(G.shape[0], sigma_G))
    M = np.sqrt(np.concatenate(steps))[:, None] * np.vstack(rows) * np.sqrt(tau.ravel())[None, :]
    norm2 = float(np.linalg.norm(M, 2) ** 2)
    print(f"PDHG diagonal steps, ratio {ratio}, TV {tv}: |Sigma^1/2 K T^1/2|^2 = {norm2:.6f}")
    assert norm2 <= 0.9025 * (1 + 1e-9), norm2


def test_host_scalars_are_float32_and_follow_the_specification():
    f = np.float32
    a, t, sigma_G, w = D.host_scalars(3, True, 4.0)
    assert all(type(v) is np.float32 for v in (a, t, sigma_G, w))
    assert a == f(0.95) * f(4) and t == f(0.95) / f(4) and sigma_G == a / f(2) and w == f(6)
    assert D.host_scalars(2, True)[3] == f(4) and D.host_scalars(3, False)[3] == f(0)
    assert D.EPS == 2.0 ** -10
    sums = np.array([0.0, -0.0, 2.0 ** -11, 2.0 ** -10, 0.5, np.float32(3.0)], f)
    got = D.diag_steps(sums, a)
    assert got.dtype == np.float32 and np.array_equal(got, [a * f(1024), a * f(1024), a * f(1024), a * f(1024), a / f(0.5), a / f(3)])
    assert np.array_equal(D.diag_steps(sums, t, w), t / (sums + w))


# ------------------------------------------------------------------------------------------------ the guard
WIDE_NU, WIDE_NZ = 48, 2     # a detector of 48 pixels in front of a 32 x 32 volume: the diagonal is 45.3


class _Rows:
    """the dense operator with only the rows `keep` of every slice's matrix: sinograms are [nz, len(keep)] arrays"""

    def __init__(self, dense, keep):
        self.n, self.A = dense.n, dense.A[keep]

    def fp(self, vol):
        vol = np.asarray(vol, np.float64)
        return vol.reshape(vol.shape[0], -1) @ self.A.T

    def bp(self, sino):
        sino = np.asarray(sino, np.float64)
        return (sino @ self.A).reshape(sino.shape[0], self.n, self.n)


@functools.lru_cache(maxsize=None)
def _wide():
    dense = P.Dense64(K.N, WIDE_NU, K.ANGLES, 0.0)
    b = dense.fp(K.phantom(WIDE_NZ, floor=0.1)) + 0.3 * np.random.default_rng(24).standard_normal((WIDE_NZ, K.NA, WIDE_NU))
    return dense, np.maximum(b, 0.05)


@pytest.mark.parametrize("fidelity, lam, nonneg", [("LS", 0.5, False), ("L1", 0.5, False), ("KL", 0.05, True)], ids=lambda v: str(v))
def test_rays_that_miss_the_volume_take_the_guarded_step_and_change_nothing(fidelity, lam, nonneg):
    dense, b = _wide()
    missed = dense.A.sum(axis=1) == 0.0
    assert 0 < missed.sum() < missed.size // 2 and (dense.A >= 0.0).all()
    kw = dict(fidelity=fidelity, lam=lam, nonneg=nonneg, dtype=np.float64)
    state = {}
    full = list(D.pdhg_iterates(dense, b, iterations=10, state=state, **kw))
    a = D.host_scalars(3, dtype=np.float64)[0]
    assert np.array_equal(state["sigma"].reshape(WIDE_NZ, -1)[:, missed], np.full((WIDE_NZ, missed.sum()), a / D.EPS))
    assert (state["sigma"].reshape(WIDE_NZ, -1)[:, ~missed] <= a / D.EPS).all()   # (a grazing ray below eps is guarded too)
    assert all(np.isfinite(x).all() for x in full) and np.isfinite(state["y"]).all() and np.abs(full[-1]).max() > 0
    keep = np.flatnonzero(~missed)
    less = list(D.pdhg_iterates(_Rows(dense, keep), b.reshape(WIDE_NZ, -1)[:, keep], iterations=10,
                                vol_shape=(WIDE_NZ, K.N, K.N), **kw))
    worst = max(float(np.abs(x - z).max() / max(1.0, np.abs(z).max())) for x, z in zip(full, less))
    print(f"PDHG diagonal {fidelity}: {int(missed.sum())} of {missed.size} rays miss; iterates with and without them differ by {worst:.2e}")
    assert worst <= 1e-12, worst


# ------------------------------------------------------------------------------------------------ float32 against float64
@functools.lru_cache(maxsize=None)
def _run(name, dtype_name, counts):
    kw, positive = K.CASES[name]
    op = K.matched() if dtype_name == "float32" else K.dense()
    return D.pdhg_many(op, K.sinogram(positive=positive), counts, dtype=np.dtype(dtype_name).type, **kw)


@pytest.mark.parametrize("name", list(K.CASES))
def test_float32_against_float64(name):
    """the float32 arithmetic the kernels reproduce holds the project's parity bar against the same algorithm in double
    (the values seen are recorded in docs/kernels/pdhg.md)"""
    f32, f64 = _run(name, "float32", K.COUNTS), _run(name, "float64", K.COUNTS)
    for n in K.COUNTS:
        r = P.rel_l2(f32[n], f64[n])
        print(f"PDHG diagonal {name} after {n}: float32 vs float64 rel-L2 = {r:.2e}")
        assert f32[n].dtype == np.float32 and f64[n].dtype == np.float64 and f32[n].shape == (K.NZ, K.N, K.N)
        assert r <= 1e-5, (name, n, r)


# ------------------------------------------------------------------------------------------------ convergence
LONG = 3000


def _objective(x, b, kw):
    """F(Ax) + lambda TV(x) in float64; the KL term in its divergence form sum(Ax - b + b log(b / Ax)) -- the same objective
    up to a constant, but with its zero at a perfect fit, like the other two, so that "within 1 %" means something"""
    value = P.objective(K.dense(), x, b, kw["fidelity"], kw["lam"])
    if kw["fidelity"] == "KL":
        bp = np.maximum(np.asarray(b, np.float64), 0.0)
        value -= float((bp - np.where(bp > 0.0, bp * np.log(np.where(bp > 0.0, bp, 1.0)), 0.0)).sum())
    return value


@functools.lru_cache(maxsize=None)
def _objectives(name, diagonal):
    """the float64 objective after each of LONG iterations"""
    kw, positive = K.CASES[name]
    b = K.sinogram(positive=positive)
    its = (D.pdhg_iterates(K.dense(), b, iterations=LONG, dtype=np.float64, **kw) if diagonal else
           P.pdhg_iterates(K.dense(), b, K.lipschitz(), iterations=LONG, dtype=np.float64, **kw))
    return np.array([_objective(x, b, kw) for x in its])


def _count(obj, best, share):
    """the first iteration whose objective lies within `share` of the best one"""
    return int(np.flatnonzero(obj - best <= share * abs(best))[0]) + 1


@pytest.mark.parametrize("name", list(K.CASES))
def test_objective_falls_and_the_diagonal_steps_need_fewer_iterations(name):
    scalar, diag = _objectives(name, False), _objectives(name, True)
    at = [diag[n - 1] for n in K.CHECKPOINTS]
    print(f"PDHG diagonal {name}: objective at {K.CHECKPOINTS} = {['%.8g' % v for v in at]}")
    assert all(np.isfinite(at)) and all(later < earlier for earlier, later in zip(at, at[1:])), at
    best = min(scalar.min(), diag.min())
    counts = {share: (_count(scalar, best, share) if (scalar - best <= share * abs(best)).any() else None,
                      _count(diag, best, share) if (diag - best <= share * abs(best)).any() else None) for share in (0.01, 0.001)}
    print(f"PDHG {name}: best objective of {LONG} iterations {best:.8g}; iterations to come within 1 % / 0.1 % of it: "
          f"scalar steps {counts[0.01][0]} / {counts[0.001][0]}, diagonal steps {counts[0.01][1]} / {counts[0.001][1]}")
    s, d = counts[0.01]
    if name == "LS+TV":
        assert d is not None and s is not None and 3 * d <= s, (s, d)
    elif name == "KL+TV":
        assert d is not None and s is not None and d <= s, (s, d)
    # L1+TV and LS without TV: recorded, not asserted (docs/kernels/pdhg.md)


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


def test_the_key_defaults_to_none_and_takes_diagonal():
    assert _dicts()[1]["PDHG_preconditioner"] is None
    assert _dicts(algo={"PDHG_preconditioner": None})[1]["PDHG_preconditioner"] is None
    _, a, _ = _dicts(algo={"PDHG_preconditioner": "diagonal"}, reg={"method": "PD_TV"})
    assert a["PDHG_preconditioner"] == "diagonal" and "lipschitz_const" not in a
    assert _dicts(method_run="SPDHG", me=_self(OS_number=4))[1]["PDHG_preconditioner"] is None
    assert "PDHG_preconditioner" not in _dicts(method_run="FISTA")[1]


@pytest.mark.parametrize("value", ["Diagonal", "jacobi", "", 1, True, 0.5])
def test_other_values_are_refused(value):
    with pytest.raises(ValueError, match="PDHG_preconditioner"):
        _dicts(algo={"PDHG_preconditioner": value})


@pytest.mark.parametrize("value", ["diagonal", "jacobi"])
def test_spdhg_refuses_the_key(value):
    with pytest.raises(ValueError, match="PDHG_preconditioner.*PDHG only"):
        _dicts(algo={"PDHG_preconditioner": value}, method_run="SPDHG", me=_self(OS_number=4))


VOL, SINO = CALLS.VOL, CALLS.SINO


@pytest.fixture
def driver(monkeypatch):
    """a RecToolsIRCuPy whose projector and launches are recorders on CPU tensors: (the object, the log of calls)"""
    return CALLS.recording_driver(monkeypatch, more_ops=("pdhg_diag_steps",))


def _data():
    import torch
    return {"projection_data": torch.zeros(SINO, dtype=torch.float32)}


SET_UP = ["fill 0.0", "WORK", "fill 0.0", "fill 0.0", "fill 0.0", "fill 0.0", "A.invalidate", "A.set_residual_layout planar",
          "A.set_volume_layout planar"]
TEAR_DOWN = ["A.set_residual_layout planar", "A.set_volume_layout planar", "A.invalidate"]


def test_without_the_key_the_driver_makes_the_calls_it_always_made(driver):
    """x0, the work arrays, q = 0 three times, y = 0, the layouts; per iteration the five launches; the layouts again"""
    rt, log = driver
    for algo in ({}, {"PDHG_preconditioner": None}):
        del log[:]
        algo = dict(algo, iterations=2, lipschitz_const=50.0, recon_mask_radius=None)
        rt.PDHG(_data(), algo, {"method": "PD_TV"})
        loop = ["A.forward", "pdhg_sino_dual", "A.backward", "pdhg_tv_dual", "pdhg_primal"]
        assert log == [c.replace("WORK", "pdhg_work_arrays") for c in SET_UP] + 2 * loop + TEAR_DOWN
        assert rt.last_run["preconditioner"] is None and rt.last_run["method"] == "PDHG"


@pytest.mark.parametrize("tv", [True, False], ids=["TV", "no TV"])
def test_with_the_key_the_power_method_never_runs_and_the_diag_launches_do(driver, tv):
    rt, log = driver
    algo = {"iterations": 2, "PDHG_preconditioner": "diagonal", "recon_mask_radius": None}
    rt.PDHG(_data(), algo, {"method": "PD_TV"} if tv else None)
    assert "lipschitz_const" not in algo
    set_up = [c.replace("WORK", "pdhg_work_arrays tau") for c in SET_UP]
    if not tv:
        del set_up[2:5]
    steps = ["fill 1.0", "A.forward", "pdhg_diag_steps", "fill 1.0", "A.backward", "pdhg_diag_steps"]   # two projector calls
    loop = ["A.forward", "pdhg_sino_dual_diag", "A.backward"] + (["pdhg_tv_dual"] if tv else []) + ["pdhg_primal_diag"]
    assert log == set_up + steps + 2 * loop + TEAR_DOWN
    assert rt.last_run["preconditioner"] == "diagonal" and rt.last_run["iterations_done"] == 2


def test_the_layouts_are_restored_when_the_set_up_projection_raises(driver, monkeypatch):
    rt, log = driver

    def failing(vol, sub, out=None):
        raise RuntimeError("stop here")

    monkeypatch.setattr(rt.Atools, "forward", failing, raising=False)
    with pytest.raises(RuntimeError, match="stop here"):
        rt.PDHG(_data(), {"iterations": 2, "PDHG_preconditioner": "diagonal"}, {"method": "PD_TV"})
    assert log[-3:] == TEAR_DOWN


# ------------------------------------------------------------------------------------------------ C-ABI
def test_scratch_bytes_keep_their_value_and_tau_is_one_more_array():
    from tomobar_amd import _lib, ops
    lib = _lib.lib()
    for dx, dy, dz in [(37, 13, 7), (64, 64, 64), (1, 1, 1)]:
        arr3 = (dx * dy * dz * 4 + 255) // 256 * 256 + ops.ARRAY_SKEW
        arr2 = (dx * dy * 4 + 255) // 256 * 256 + ops.ARRAY_SKEW
        assert lib.tomo_pdhg_scratch_bytes(dx, dy, dz, 3) == 5 * arr3 and lib.tomo_pdhg_diag_scratch_bytes(dx, dy, dz, 3) == 6 * arr3
        assert lib.tomo_pdhg_scratch_bytes(dx, dy, dz, 2) == 4 * arr2 and lib.tomo_pdhg_diag_scratch_bytes(dx, dy, dz, 2) == 5 * arr2


def test_invalid_arguments_are_refused_before_the_device_is_touched():
    from tomobar_amd import _lib
    lib = _lib.lib()
    p = [C.c_void_p(0x1000 * k) for k in range(1, 9)]   # never dereferenced: every case fails validation
    nul = C.c_void_p(0)

    def steps(out=p[0], src=p[1], n=16, numer=0.95, add=0.0):
        return lib.tomo_pdhg_diag_steps(out, src, n, numer, add, None)

    def sino(y=p[0], r=p[1], b=p[2], s=p[3], n=16, fid=0):
        return lib.tomo_pdhg_sino_dual_diag(y, r, b, s, n, fid, None)

    def primal(x=p[0], xb=p[1], g=p[2], tau=p[3], q1=p[4], q2=p[5], q3=p[6], dx=4, dy=4, dz=4, nd=3):
        return lib.tomo_pdhg_primal_diag(0, x, xb, g, tau, q1, q2, q3, dx, dy, dz, nd, 0, None)

    bad = [(steps, dict(out=nul)), (steps, dict(src=nul)), (steps, dict(numer=0.0)), (steps, dict(numer=float("nan"))),
           (steps, dict(add=-1.0)), (steps, dict(add=float("inf"))),
           (sino, dict(fid=3)), (sino, dict(fid=-1)), (sino, dict(y=nul)), (sino, dict(s=nul)), (sino, dict(r=p[0])),
           (sino, dict(b=p[0])), (sino, dict(s=p[0])),
           (primal, dict(nd=5)), (primal, dict(dx=0)), (primal, dict(x=nul)), (primal, dict(tau=nul)), (primal, dict(xb=p[0])),
           (primal, dict(g=p[1])), (primal, dict(tau=p[0])), (primal, dict(tau=p[1])), (primal, dict(tau=p[2])),
           (primal, dict(q2=nul)), (primal, dict(q1=nul)), (primal, dict(q3=p[0])), (primal, dict(q3=nul))]
    for fn, kw in bad:
        assert fn(**kw) == _lib.E_INVALID, (fn.__name__, kw)
        with pytest.raises(ValueError):
            _lib.check(fn(**kw))
    assert steps(n=0) == _lib.OK and sino(n=0) == _lib.OK   # nothing to do, nothing launched
