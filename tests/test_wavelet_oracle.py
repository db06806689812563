"""The `_WAVELETS` suffix without a GPU: the numpy restatement tests/_wavelet_oracle.py of docs/kernels/wavelets.md held
against what the document states (taps, perfect reconstruction, Parseval, the offset convention and band order, the
threshold), and everything in Python that reads the suffix -- prox_regul's dispatch (recorders in the manner of
tests/test_regulariser_table.py), the refusals, dicts_check, ADMM's division by rho, FISTA end to end on the oracle
stand-ins of tests/_cpu_backend.py, and one z-slab case over gloo."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import _wavelet_oracle as W
import test_regulariser_table as TT   # the literal expectations of the table's dispatch tests (read, not collected from here)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (2, 3), (1, 37), (37, 1), (13, 37), (16, 24), (150, 200)]
_ids = lambda s: "x".join(map(str, s))   # noqa: E731


def field(shape, seed=5):
    return np.random.default_rng(seed).standard_normal(shape)


# ------------------------------------------------------------------------------------------------ taps
def test_committed_literals_are_the_derived_filter():
    h = W.derive_taps()
    lit = np.array(W.H_LITERALS)
    assert h.shape == (10,) and np.abs(h - lit).max() <= 1e-14
    assert abs(lit.sum() - np.sqrt(2.0)) <= 1e-14
    g = np.array([(-1) ** k * lit[9 - k] for k in range(10)])
    for m in range(-4, 5):
        ks = [k for k in range(10) if 0 <= k + 2 * m < 10]
        assert abs(sum(lit[k] * lit[k + 2 * m] for k in ks) - (m == 0)) <= 1e-14, m
        assert abs(sum(g[k] * g[k + 2 * m] for k in ks) - (m == 0)) <= 1e-14, m
        assert abs(sum(lit[k] * g[k + 2 * m] for k in ks)) <= 1e-14, m
    h64, g64 = W.taps(np.float64)
    assert np.array_equal(h64, lit) and np.array_equal(g64, g)
    h32, g32 = W.taps(np.float32)
    assert h32.dtype == g32.dtype == np.float32 and np.array_equal(h32, lit.astype(np.float32))
    assert np.array_equal(g32, g.astype(np.float32))


def test_the_kernel_source_holds_the_same_literals():
    import re
    src = open(os.path.join(ROOT, "tomobar_amd", "csrc", "wavelet_kernels.hip")).read()
    found = [float(v) for v in re.findall(r"#define WL_H\d (-?[0-9.]+)f", src)]
    assert found == list(W.H_LITERALS)


# ------------------------------------------------------------------------------------------------ the float64 oracle
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_perfect_reconstruction_and_parseval(shape):
    x = field(shape)
    back = W.shrink(x, 0.0, np.float64)
    assert back.shape == x.shape and np.abs(back - x).max() <= 1e-12 * np.abs(x).max()
    # Parseval, level by level: the four bands of a level carry the energy of the even-extended input of that level
    s = x
    for bands in W.forward(x, 0.0, np.float64):
        ext = W._extend(np.swapaxes(W._extend(s), -1, -2))
        assert abs(sum(float(np.sum(b * b)) for b in bands) - float(np.sum(ext * ext))) <= 1e-12 * float(np.sum(ext * ext))
        assert all(b.shape == ((s.shape[0] + 1) // 2, (s.shape[1] + 1) // 2) for b in bands)
        s = bands[0]


def test_parseval_of_the_whole_pyramid_when_no_level_is_extended():
    x = field((16, 24))
    levels = W.forward(x, 0.0, np.float64)
    energy = float(np.sum(levels[-1][0] ** 2)) + sum(float(np.sum(b * b)) for lev in levels for b in lev[1:])
    assert abs(energy - float(np.sum(x * x))) <= 1e-12 * float(np.sum(x * x))


def test_unit_impulse_pins_the_offsets_and_the_band_order():
    """an impulse at (y0, x0) = (13, 20) of a 32 x 40 slice: a[i] = h[n0 - 2 i], so level 1 holds f_y[13 - 2 i] f_x[20 - 2 j]
    at i = 2 .. 6, j = 6 .. 10 with (f_x, f_y) = (h, h), (h, g), (g, h), (g, g) for LL, LH, HL, HH -- first letter the x
    filter -- and zeros elsewhere"""
    h, g = W.taps(np.float64)
    x = np.zeros((32, 40))
    x[13, 20] = 1.0
    ll, lh, hl, hh = W.forward(x, 0.0, np.float64)[0]
    for band, fx, fy in ((ll, h, h), (lh, h, g), (hl, g, h), (hh, g, g)):
        want = np.zeros((16, 20))
        for i in range(2, 7):
            for j in range(6, 11):
                want[i, j] = fy[13 - 2 * i] * fx[20 - 2 * j]
        assert np.abs(band - want).max() <= 1e-15
    # wrap-around: an impulse at sample 1 reaches the last coefficients (2 i + k = 1 mod n)
    x = np.zeros((32, 40))
    x[0, 1] = 1.0
    ll = W.forward(x, 0.0, np.float64)[0][0]
    assert abs(ll[0, 0] - h[0] * h[1]) <= 1e-15 and abs(ll[0, 19] - h[0] * h[3]) <= 1e-15 and abs(ll[15, 16] - h[2] * h[9]) <= 1e-15


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_constant_slice_has_no_details_and_a_large_threshold_leaves_ll3(shape):
    c = -3.25
    for lev in W.forward(np.full(shape, c), 0.0, np.float64):
        assert all(np.abs(b).max() <= 1e-12 * abs(c) for b in lev[1:])
    x = field(shape)
    levels = W.forward(x, 0.0, np.float64)
    t = 2.0 * max(float(np.abs(b).max()) for lev in levels for b in lev[1:]) + 1.0
    bare = [[b if i == 0 else np.zeros_like(b) for i, b in enumerate(lev)] for lev in levels]
    assert np.array_equal(W.shrink(x, t, np.float64), W.inverse(bare, shape, np.float64))
    # the threshold itself: copysign(max(|d| - t, 0), d), LL untouched
    d = np.array([-2.0, -0.5, -0.0, 0.0, 0.5, 2.0])
    assert np.array_equal(W.soft(d, 0.5, np.float64), np.array([-1.5, -0.0, -0.0, 0.0, 0.0, 1.5]))
    assert np.array_equal(np.signbit(W.soft(d, 0.5, np.float64)), np.signbit(d))
    thr = W.forward(x, 0.3, np.float64)
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(thr, levels))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
def test_a_stack_is_the_stack_of_its_slices(dtype):
    vol = field((5, 13, 37)).astype(dtype)
    whole = W.shrink(vol, 0.05, dtype)
    assert whole.dtype == dtype
    for z in range(5):
        assert np.array_equal(whole[z], W.shrink(vol[z], 0.05, dtype))
    assert np.array_equal(W.shrink(vol[1:4], 0.05, dtype), whole[1:4])
    levels = W.forward(vol, 0.05, dtype)
    flat = W.pack(levels)
    assert flat.dtype == dtype and flat.size == 5 * 4 * (7 * 19 + 4 * 10 + 2 * 5)
    assert all(np.array_equal(a, b) for l1, l2 in zip(levels, W.unpack(flat, vol.shape)) for a, b in zip(l1, l2))
    assert np.array_equal(flat[:flat.size // 5], W.pack(W.forward(vol[0], 0.05, dtype)))
    m = field((5, 13, 37), 6).astype(dtype)
    assert np.array_equal(W.shrink(vol, 0.05, dtype, mix=m), (m + whole) * dtype(0.5))


def test_float32_mode_rounds_every_operation():
    """the float32 restatement against the same sums spelled out one operation at a time on one short line"""
    h, g = W.taps(np.float32)
    x = field((1, 6)).astype(np.float32)
    a, d = W.analysis(x, np.float32)
    for i in range(3):
        sa = sd = np.float32(0.0)
        for k in range(10):
            sa = np.float32(sa + np.float32(h[k] * x[0, (2 * i + k) % 6]))
            sd = np.float32(sd + np.float32(g[k] * x[0, (2 * i + k) % 6]))
        assert a[0, i] == sa and d[0, i] == sd
    back = W.synthesis(a, d, 6, np.float32)
    for j in range(6):
        s = np.float32(0.0)
        for k in range(j & 1, 10, 2):
            i = ((j - k) % 6) // 2
            s = np.float32(s + np.float32(h[k] * a[0, i]))
            s = np.float32(s + np.float32(g[k] * d[0, i]))
        assert back[0, j] == s


# ------------------------------------------------------------------------------------------------ the suffix in the table module
KINDS = [k for k in TT.ORDER if k != "LLT_ROF"]


def test_suffix_predicate():
    from tomobar_amd.supp import regularisers as T
    assert tuple(k.name for k in T.KINDS) == TT.ORDER            # the table itself is as it was
    assert T.WAVELETS == "WAVELETS" and callable(T.has_wavelets)
    for kind in TT.ORDER:
        assert T.has_wavelets(f"{kind}_WAVELETS") and T.has_wavelets(f"WAVELETS_{kind}") and not T.has_wavelets(kind)
        assert T.kind_of(f"{kind}_WAVELETS").name == kind
    for method in (None, 123, "WAVELETS", "FGP_TV_WAVELETS", "PD_TV_wavelets"):
        assert not T.has_wavelets(method)
    assert T.wavelet_threshold({}) == 0.001 and T.wavelet_threshold({"regul_param2": 0.5}) == 0.5
    from tomobar_amd import _lib
    assert T.WAVELETS_SCRATCH in _lib.SIGNATURES and len(_lib.SIGNATURES[T.WAVELETS_SCRATCH][1]) == 4


@pytest.fixture
def calls(monkeypatch):
    """every function prox_regul can end in, the wavelet function included, replaced by a recorder"""
    from tomobar_amd import regularisersCuPy as R
    from tomobar_amd import slab as S
    log = []

    def recorder(name, is_slab):
        def fn(*args, **kwargs):
            log.append((name, args, dict(kwargs)))
            if is_slab:
                kwargs["info"].update(iterations_done=5, rel_change=0.25)
            return name
        return fn

    for name, _, _ in TT.WHOLE.values():
        monkeypatch.setattr(R, name, recorder(name, False))
    for name, _, _ in TT.SLAB.values():
        monkeypatch.setattr(S, name, recorder(name, True))
    monkeypatch.setattr(R, "WAVELETS_cupy", recorder("WAVELETS_cupy", False))
    return log


def _check_wavelet_call(call, X, threshold, result):
    name, args, kwargs = call
    assert name == "WAVELETS_cupy" and args[0] is X and TT._same(args[1:], (threshold, 0)), args
    assert set(kwargs) == {"out", "mix"} and kwargs["out"] is result and kwargs["mix"] is result, kwargs


@pytest.mark.parametrize("optional", [False, True], ids=["defaults", "optional_keys"])
@pytest.mark.parametrize("shape, slab", [((4, 5, 6), False), ((1, 5, 6), True)], ids=["whole_volume", "singleton_axis_with_slab"])
def test_suffix_runs_the_kind_as_before_then_the_wavelet_function(calls, shape, slab, optional):
    from tomobar_amd import regularisersCuPy as R
    X, out = torch.zeros(shape), torch.zeros(shape)
    comm = object() if slab else None
    for kind in KINDS:
        for method in (f"{kind}_WAVELETS", f"WAVELETS_{kind}"):
            fn, plain, full = TT.WHOLE[kind]
            del calls[:]
            assert R.prox_regul(TT._self(comm), X, TT._reg(kind, optional, kind), out=out) == fn
            (before,) = calls
            del calls[:]
            R._record(-1, -1.0)
            assert R.prox_regul(TT._self(comm), X, TT._reg(method, optional, kind), out=out) == fn, method
            first, second = calls
            assert first[0] == before[0] == fn and first[1][0] is X and TT._same(first[1][1:], before[1][1:]), (method, first)
            assert TT._same(first[1][1:], full if optional else plain) and first[2] == before[2] and first[2]["out"] is out
            _check_wavelet_call(second, X, 0.44 if optional else 0.001, fn)
            assert R.last_prox() == (-1, -1.0)    # (the recorders record nothing: the wavelet step did not either)


@pytest.mark.parametrize("optional", [False, True], ids=["defaults", "optional_keys"])
def test_suffix_in_slab_mode_runs_the_slab_driver_then_the_wavelet_function(calls, optional):
    from tomobar_amd import regularisersCuPy as R
    X, out, comm = torch.zeros((4, 5, 6)), torch.zeros((4, 5, 6)), object()
    for kind in KINDS:
        method = f"{kind}_WAVELETS"
        reg = TT._reg(method, optional, kind)
        del calls[:]
        if kind == "TGV":
            for fn in (lambda: R.prox_regul(TT._self(comm), X, reg, out=out), lambda: R.check_prox_available(TT._self(comm), X.shape, reg)):
                with pytest.raises(ValueError) as e:
                    fn()
                assert str(e.value) == "TGV is not available in z-slab mode" and calls == []
            continue
        fn, plain, full = TT.SLAB[kind]
        R._record(-1, -1.0)
        assert R.prox_regul(TT._self(comm), X, reg, out=out) == fn
        first, second = calls
        assert first[0] == fn and first[1][0] is X and first[1][1] is comm and TT._same(first[1][2:], full if optional else plain)
        assert set(first[2]) == {"out", "tolerance", "info"} and first[2]["out"] is out and first[2]["tolerance"] == 0.001
        _check_wavelet_call(second, X, 0.44 if optional else 0.001, fn)
        assert R.last_prox() == (5, 0.25)   # the kind's iterations


@pytest.mark.parametrize("slab", [False, True], ids=["whole_volume", "slab"])
def test_suffix_refusals(calls, slab):
    from tomobar_amd import regularisersCuPy as R
    X, comm = torch.zeros((4, 5, 6)), object() if slab else None
    for method in ("LLT_ROF_WAVELETS", "WAVELETS_LLT_ROF"):
        for fn in (lambda: R.prox_regul(TT._self(comm), X, dict(TT.REG, method=method)),
                   lambda: R.check_prox_available(TT._self(comm), X.shape, {"method": method}),
                   lambda: R.reserve_prox_scratch(TT._self(comm), X.shape, {"method": method})):
            with pytest.raises(ValueError) as e:
                fn()
            assert str(e.value) == "LLT_ROF does not combine with WAVELETS: regul_param2 is already its second weight"
    # a method that also names an earlier kind runs that kind
    R.check_prox_available(TT._self(comm), X.shape, {"method": "LLT_ROF_PD_TV_WAVELETS"})
    for method in ("WAVELETS", "FGP_TV_WAVELETS"):
        with pytest.raises(ValueError) as e:
            R.prox_regul(TT._self(comm), X, dict(TT.REG, method=method))
        assert str(e.value) == TT.UNKNOWN.replace("'FGP_TV'", repr(method))
    for kind in ("TGV", "NDF", "Diff4th"):
        with pytest.raises(ValueError) as e:
            R.prox_regul(TT._self(comm), X, dict(TT.REG, method=f"{kind}_WAVELETS", half_precision=True))
        assert str(e.value) == f"{kind} does not support half_precision=True"
    assert calls == []


def test_reserve_prox_scratch_reserves_the_pyramid_by_a_call_of_its_own(monkeypatch):
    import types
    from tomobar_amd import regularisersCuPy as R
    log = []
    monkeypatch.setattr(R, "ops", types.SimpleNamespace(reserve_tv_scratch=lambda *a: log.append(("tv",) + a),
                                                        reserve_wavelet_scratch=lambda *a: log.append(("wavelet",) + a)))
    for shape, passed in (((8, 9, 10), (8, 9, 10)), ((1, 9, 10), (9, 10)), ((9, 10), (9, 10))):
        for kind in KINDS:
            del log[:]
            R.reserve_prox_scratch(TT._self(), shape, {"method": f"{kind}_WAVELETS"})
            assert log == [("tv", passed, "cuda:0", kind, False), ("wavelet", passed, "cuda:0")], (shape, kind, log)
            del log[:]
            R.reserve_prox_scratch(TT._self(), shape, {"method": kind})
            assert log == [("tv", passed, "cuda:0", kind, False)]
    del log[:]
    R.reserve_prox_scratch(TT._self(object()), (8, 9, 10), {"method": "PD_TV_WAVELETS"})   # a slab rank reserves nothing
    R.reserve_prox_scratch(TT._self(), (8, 9, 10), {"method": "WAVELETS"})
    assert log == []


# ------------------------------------------------------------------------------------------------ dictionaries, ADMM
def test_dicts_check_adds_exactly_regul_param2(monkeypatch):
    import types
    from tomobar_amd import ops
    from tomobar_amd.supp.dicts import dicts_check
    monkeypatch.setattr(ops, "to_device", lambda x, index: x)
    me = types.SimpleNamespace(Atools=types.SimpleNamespace(device_index=0), OS_number=1)

    def run(reg):
        return dicts_check(me, {"projection_data": torch.zeros((2, 3, 4))}, {}, reg, method_run="FISTA")[2]

    for kind in TT.ORDER:
        plain = run({"method": kind})
        got = run({"method": f"{kind}_WAVELETS"})
        assert set(got) - set(plain) == ({"regul_param2"} if kind != "LLT_ROF" else set()), kind
        assert got["regul_param2"] == 0.001 and {k: got[k] for k in plain if k != "method"} == {k: plain[k] for k in plain if k != "method"}
        assert run({"method": f"{kind}_WAVELETS", "regul_param2": 0.25})["regul_param2"] == 0.25
        for bad in (0.0, -1.0):
            with pytest.raises(ValueError) as e:
                run({"method": f"{kind}_WAVELETS", "regul_param2": bad})
            assert str(e.value) == "_regularisation_['regul_param2'] must be positive"
    assert "regul_param2" not in run({"method": "WAVELETS"}) and "regul_param2" not in run({"method": "PD_TV"})


NZ, NN, NA = 4, 16, 12
ANGLES = np.linspace(0, np.pi, NA, endpoint=False)
T_W = 0.004


def _sino():
    return np.random.default_rng(11).random((NZ, NA, NN)).astype(np.float32)


def _data():
    return {"projection_data": _sino(), "data_axes_labels_order": ["detY", "angles", "detX"]}


@pytest.fixture
def cpu_ops(monkeypatch):
    """the drivers on the oracle stand-ins (tests/_cpu_backend.py, with the whole-volume TV of tests/_cpu_backend_tol.py),
    plus the one function this suffix adds to the ops seam: the float32 restatement"""
    import _cpu_backend as B
    import _cpu_backend_tol as BT
    ops = BT.install(monkeypatch)
    ops.wavelet_calls = []

    def wavelet_shrink(data, threshold, out=None, mix=None):
        assert type(threshold) is np.float32
        ops.wavelet_calls.append((tuple(data.shape), float(threshold), mix is not None and mix.data_ptr() == out.data_ptr()))
        res = W.shrink(B._np(data), threshold, np.float32, mix=None if mix is None else B._np(mix).copy())
        return torch.from_numpy(res) if out is None else B._put(out, res)

    ops.wavelet_shrink = wavelet_shrink
    ops.reserve_wavelet_scratch = lambda *args: None
    return ops


def test_admm_divides_the_threshold_by_rho(cpu_ops, monkeypatch):
    import tomobar_amd.methodsIR_CuPy as IR
    seen = []

    def prox(self, X, r, out=None):
        seen.append((r["method"], r["regul_param"], r["regul_param2"]))
        out.copy_(X)
        return out

    monkeypatch.setattr(IR, "prox_regul", prox)
    reg = {"method": "PD_TV_WAVELETS", "regul_param": 0.002, "regul_param2": T_W, "iterations": 3}
    IR.RecToolsIRCuPy(NN, 0, NZ, 0.0, ANGLES, NN, 0, None).ADMM(_data(), {"iterations": 1, "lipschitz_const": 3000.0, "ADMM_rho_const": 4.0}, reg)
    assert seen == [("PD_TV_WAVELETS", 0.002 / 4.0, T_W / 4.0)]
    assert reg["regul_param"] == 0.002 and reg["regul_param2"] == T_W, "the caller's values were rewritten"
    del seen[:]
    reg = {"method": "PD_TV", "regul_param": 0.002, "regul_param2": T_W, "iterations": 3}     # without the suffix: untouched
    IR.RecToolsIRCuPy(NN, 0, NZ, 0.0, ANGLES, NN, 0, None).ADMM(_data(), {"iterations": 1, "lipschitz_const": 3000.0, "ADMM_rho_const": 4.0}, reg)
    assert seen == [("PD_TV", 0.002 / 4.0, T_W)]


def test_fista_with_pd_tv_wavelets_equals_the_loop_composed_by_hand(cpu_ops):
    """two FISTA iterations against the same loop written out here on the oracle's projector, with the prox put together
    from the oracle's PD_TV and the float32 restatement of the shrinkage: (PD_TV(X) + W_t(X)) * 0.5.  (On the commit before
    the suffix existed the method string ran plain PD_TV: this test fails there.)"""
    import _cpu_backend as B
    import _cpu_backend_tol as BT
    import tomobar_amd.methodsIR_CuPy as IR
    f32 = np.float32
    lam, inner, lip, L = 0.002, 5, 8.0, 3000.0
    reg = {"method": "PD_TV_WAVELETS", "regul_param": lam, "regul_param2": T_W, "iterations": inner, "PD_LipschitzConstant": lip}
    algo = {"iterations": 2, "lipschitz_const": L, "nonnegativity": True, "recon_mask_radius": None}
    got = IR.RecToolsIRCuPy(NN, 0, NZ, 0.0, ANGLES, NN, 0, None).FISTA(_data(), dict(algo), dict(reg)).numpy()
    assert cpu_ops.wavelet_calls == [((NZ, NN, NN), float(f32(T_W)), True)] * 2

    A = B.OracleTools3D(NN, 0, NZ, ANGLES, 0.0, NN)
    b = torch.from_numpy(_sino())
    tau = f32(lam * 0.1)
    sigma, lt = f32(1.0 / (lip * tau)), f32(tau / lam)
    X, X_t, t = torch.zeros(A.vol_shape()), torch.zeros(A.vol_shape()), f32(1.0)
    res, grad = A.residual_buffer(None), torch.zeros(A.vol_shape())
    for it in range(2):
        A.residual(X_t, b, None, "LS", None, res)
        t_old = t
        t = f32((f32(1.0) + np.sqrt(f32(1.0) + f32(4.0) * t * t)) * f32(0.5))
        beta = f32((t_old - f32(1.0)) / t)
        A.grad_step(res, X_t, grad, f32(1.0 / L), True, None)
        tv = BT._orc_pdtv(grad, sigma, tau, lt, f32(1.0), inner, 0, 1, False)
        prox = torch.from_numpy((tv + W.shrink(grad.numpy(), f32(T_W), np.float32)) * f32(0.5))
        if it == 0:
            A.momentum(prox, X, X_t, beta)
        X = prox
    assert np.array_equal(got.view(np.uint32), X.numpy().view(np.uint32)), float(np.abs(got - X.numpy()).max())
    plain = IR.RecToolsIRCuPy(NN, 0, NZ, 0.0, ANGLES, NN, 0, None).FISTA(_data(), dict(algo), dict(reg, method="PD_TV")).numpy()
    assert len(cpu_ops.wavelet_calls) == 2 and not np.array_equal(got, plain)


# ------------------------------------------------------------------------------------------------ z-slabs over gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _slab_worker(rank, world, port, shape, reg, want):
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import types
        import _cpu_backend as B
        import _ndf_oracle
        import _wavelet_oracle as W
        from _tgv_oracle import phantom
        import tomobar_amd.regularisersCuPy as R
        import tomobar_amd.slab as SL
        ops = B.make_ops()
        shrunk = []

        def wavelet_shrink(data, threshold, out=None, mix=None):
            shrunk.append(tuple(data.shape))
            return B._put(out, W.shrink(B._np(data), threshold, np.float32, mix=B._np(mix).copy()))

        ops.wavelet_shrink = wavelet_shrink
        R.ops = ops
        SL._hip_ndf_step = _ndf_oracle.ORACLE.step_slab
        comm = SL.SlabComm(rank, world)
        z0, z1 = SL.slab_bounds(shape[0], world, rank)
        vol = phantom(shape)
        mine = torch.from_numpy(vol[z0:z1].copy())
        me = types.SimpleNamespace(nonneg_regul=0, Atools=types.SimpleNamespace(device_index=0), slab=comm)
        before = comm.timing_summary()["messages"]
        got = R.prox_regul(me, mine, dict(reg))
        assert shrunk == [(z1 - z0,) + tuple(shape[1:])], (rank, shrunk)
        assert np.array_equal(got.numpy().view(np.uint32), want[z0:z1].view(np.uint32)), (rank, np.abs(got.numpy() - want[z0:z1]).max())
        assert np.array_equal(mine.numpy(), vol[z0:z1]), "the input was written"
        assert R.last_prox()[0] == reg["iterations"]
        # every message belongs to the kind's halo exchange: one each way per neighbour and iteration
        sent = comm.timing_summary()["messages"] - before
        assert sent == 2 * reg["iterations"] * (int(comm.has_lo) + int(comm.has_hi)), (rank, sent)
    finally:
        dist.destroy_process_group()


def test_slab_ranks_shrink_their_own_planes_and_match_the_whole_volume(shape=(9, 7, 11), world=2):
    import _ndf_oracle
    from _tgv_oracle import phantom
    p = _ndf_oracle.PARAMS["A"]
    reg = dict(method="NDF_WAVELETS", regul_param=p["lam"], edge_threshold=p["sigma"], time_marching_step=p["tau"],
               NDF_penalty=p["penalty"], iterations=6, regul_param2=0.05)
    vol = phantom(shape)
    kind = np.array(_ndf_oracle.ORACLE.cached(shape, "A", (6,))[6])
    want = (kind + W.shrink(vol, np.float32(0.05), np.float32)) * np.float32(0.5)
    assert not np.array_equal(want, kind)
    mp.start_processes(_slab_worker, args=(world, _free_port(), shape, reg, want), nprocs=world, join=True, start_method="spawn")
