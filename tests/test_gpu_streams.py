"""MI355X: every entry point held to the stream it is given ("every entry point takes the stream explicitly",
"asynchronous on the stream passed in", the classes "order ALL their work on torch's current stream", "two streams of one
device never share scratch").  What tests/test_gpu_guards.py does for space this file does for time, with tests/_on_stream.py:
a case keeps a side stream busy for DELAY_MS, lets its inputs arrive on that stream behind the delay, makes the library call
with that stream and reads back on that stream.  Whatever the library does outside that stream runs while the delay is
pending: it reads NaN, or writes before the output's NaN fill lands.  Values are held to the oracle values of each operator's
own suite, at that suite's strictness, imported from there.

1. the harness on a stand-in that breaks the rule: it must fail it;
2. one case per prototype of include/tomo_mi355x.h with a `void *stream` (tests/_stream_table.py is the table;
   tests/test_stream_coverage.py holds it to the header without a GPU): first warm on the side stream -- arenas and plans are
   keyed by stream --, then behind the delay; an entry point documented as asynchronous must leave the stream busy;
3. two streams at once, interleaved: scratch is per stream;
4. scratch that changes under pending work: arena growth, FBP plan eviction, tomo_release_scratch;
5. the Python classes on the caller's stream.

One projector context is used by one stream at a time (the transposed-volume scratch and the token of
tomo_momentum_transposed belong to the context): sharing a context between concurrent streams is not part of the contract."""
import ctypes as C
import math
import os
import sys
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _on_stream as S  # noqa: E402
import _stream_table as ST  # noqa: E402

F32 = np.float32
REGISTERED = []


def case(name):
    """marks the test of a case of tests/_stream_table.CASES"""
    assert name in ST.CASES and name not in REGISTERED, name
    REGISTERED.append(name)
    return lambda fn: fn


@pytest.fixture(scope="module", autouse=True)
def calibrated():
    """the cycles of torch.cuda._sleep per millisecond, once for this file; afterwards the host times of the cases"""
    t0 = time.perf_counter()
    S.calibrate()
    yield
    late = [(ms, label) for label, delayed, ms in S.ENQUEUE_LOG if delayed]
    if late:
        worst = max(late)
        print(f"\nstreams: {len(late)} delayed calls, largest host time from the delay's enqueue to the return {worst[0]:.3f} ms "
              f"({worst[1]}), DELAY_MS {S.DELAY_MS}, file wall time {time.perf_counter() - t0:.1f} s")
        by_label = {}
        for ms, label in late:
            by_label[label] = max(ms, by_label.get(label, 0.0))
        for label, ms in sorted(by_label.items(), key=lambda kv: -kv[1]):
            print(f"streams:   {ms:8.3f} ms  {label}")


@pytest.fixture(scope="module")
def streams(calibrated):
    """two side streams for the whole file: arenas, plans and placed blocks are keyed by stream"""
    a, b = S.side_stream(), S.side_stream()
    assert a.cuda_stream != b.cuda_stream and 0 not in (a.cuda_stream, b.cuda_stream)
    yield a, b
    a.synchronize()
    b.synchronize()


@pytest.fixture
def side(streams):
    return streams[0]


def run_late(body, side, name, label=None):
    """`body(provider)` warm on the side stream, then behind the delay on arrays that arrive late"""
    kind = ST.CASES[name][0]
    with torch.cuda.stream(side):
        W = S.Late(side, delayed=False, label=label or name)
        body(W)
        side.synchronize()
        W.close()
        A = S.Late(side, delayed=True, asynchronous=kind != ST.SYNC, label=label or name)
        body(A)
    assert kind == ST.SYNC or A.asserted > 0, "the case never looked at the stream after a call"
    return A


def lib():
    from tomobar_amd import _lib as L
    return L.lib()


def ok(rc):
    from tomobar_amd import _lib as L
    L.check(rc)


def vp(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def cur():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def same_bits(got, want, what):
    from _march_gpu import same_bits as sb
    sb(got, np.ascontiguousarray(want), what)


# ================================================================================================ 1. the harness can fail
def test_the_harness_fails_work_that_is_not_on_the_stream(streams):
    """x * 2 under the null stream while the delay is pending on the side stream: the product is formed from the pattern, not
    from the data.  The same operation under the side stream is right.  (Poisoned memory the test owns: nothing faults.)"""
    side = streams[0]
    x = np.random.default_rng(1).standard_normal(4099).astype(np.float32)
    for s in (side, torch.cuda.default_stream()):          # warm, like every case: the product's first launch loads its kernel
        with torch.cuda.stream(s):
            W = S.Late(side, delayed=False)
            W.read(W.ro(x).view * 2.0)
    torch.cuda.synchronize()
    for on_side in (False, True):
        A = S.Late(side, label="stand-in")
        xd = A.ro(x)
        with torch.cuda.stream(side if on_side else torch.cuda.default_stream()):
            y = xd.view * 2.0
        got = A.read(y)           # (asserts that the delay is still pending)
        if on_side:
            same_bits(got, x * F32(2), "on the side stream")
        else:
            assert np.isnan(got).all(), "work on the null stream saw the data: the delay orders nothing"
        same_bits(xd.host(), x, "the input arrived")
        torch.cuda.synchronize()


def test_an_output_written_off_the_stream_is_overwritten_by_its_fill(streams):
    """the other half: a store that is not ordered on the side stream lands before late_out's NaN fill"""
    side = streams[0]
    torch.empty(4099, device="cuda").fill_(1.0)        # warm: the fill's first launch loads its kernel
    torch.cuda.synchronize()
    A = S.Late(side, label="stand-in")
    out = A.out((4099,))
    t = out.view
    with torch.cuda.stream(torch.cuda.default_stream()):
        t.fill_(1.0)
    assert np.isnan(out.host()).all()


# ================================================================================================ 2. every entry point
def G():
    import test_gpu_guards as mod
    return mod


@case("projector_pair")
def test_projector_pair(oracle, side):
    run_late(lambda A: G().case_projector_pair_and_matched_adjoint(A, oracle, G().GEOMS[0]), side, "projector_pair")


@case("fused_residuals")
def test_fused_residuals(oracle, side):
    run_late(lambda A: G().case_fused_residuals(A, oracle, G().GEOMS[0], "planar"), side, "fused_residuals")


@case("fused_epilogues")
@pytest.mark.parametrize("adjoint", ["unmatched", "matched"])
def test_fused_epilogues(oracle, side, adjoint):
    run_late(lambda A: G().case_fused_epilogues_of_both_adjoints(A, oracle, G().GEOMS[0], adjoint, 0), side, "fused_epilogues",
             f"fused_epilogues {adjoint}")


@case("volume_zquad")
def test_volume_zquad(oracle, side):
    pair = G()._pair(oracle, G().GEOMS[2])      # one context, warm and late: its scratch has grown to the quad layout's size
    run_late(lambda A: G().case_volume_zquad_producers(A, oracle, pair), side, "volume_zquad")


@case("slicewise_tv")
def test_slicewise_tv(oracle, pd_arith, side):
    run_late(lambda A: G().case_slicewise_tv(A, oracle, pd_arith), side, "slicewise_tv")


@case("wavelets")
def test_wavelets(side):
    run_late(lambda A: G().case_wavelets(A, (7, 13, 37)), side, "wavelets")


@case("patch_select_nltv")
def test_patch_select_nltv(side):
    run_late(lambda A: G().case_patch_select_and_nltv(A, (13, 37), (7, 2, 15)), side, "patch_select_nltv")


@case("fbp_filter")
def test_fbp_filter(oracle, side):
    run_late(lambda A: G().case_fbp_filter_in_place(A, oracle, 45), side, "fbp_filter")


@case("fourier_inv")
def test_fourier_inv(monkeypatch, side):
    def body(A):
        with monkeypatch.context() as m:
            G().case_fourier_inv(A, m)
    run_late(body, side, "fourier_inv")


@case("elementwise")
@pytest.mark.parametrize("name", ["momentum", "admm_dual", "axpby", "scale", "clamp_min", "mul", "recip_safe", "fill",
                                  "pwls_weights_scaled"])
def test_elementwise(oracle, side, name):
    assert "tomo_" + name in ST.CASES["elementwise"][1] and name in G().EW
    run_late(lambda A: G()._ew_case(oracle, name, 4099, 0, 0, mk=A), side, "elementwise", "tomo_" + name)


@case("pwls_weights")
def test_pwls_weights(oracle, side):
    """tomo_pwls_weights reduces max(b, 1e-6) to the host before it scales: it waits for its stream"""
    run_late(lambda A: G()._ew_case(oracle, "pwls_weights", 4099, 0, 0, mk=A), side, "pwls_weights")


def test_elementwise_runs_every_entry_of_its_table():
    assert sorted("tomo_" + n for n in G().EW) == sorted(ST.CASES["elementwise"][1] + ST.CASES["pwls_weights"][1])


@case("reductions")
def test_reductions(side):
    run_late(lambda A: G()._reductions(4099, 0, "late", mk=A), side, "reductions")


@case("rel_change")
def test_rel_change(side):
    x_h, r_h, want = G()._rel_change_inputs(4099)
    run_late(lambda A: [G()._rel_change(4099, (0, 0, 0), mode, x_h, r_h, want, mk=A) for mode in ("absent", "aliasing", "separate")],
             side, "rel_change")


@case("pad_crop_mask_permute")
def test_pad_crop_mask_permute(oracle, side):
    run_late(lambda A: G().case_pad_crop_mask_permute(A, oracle), side, "pad_crop_mask_permute")


@case("sino_terms")
def test_sino_terms(oracle, side):
    run_late(lambda A: G().case_shift_rows_residual_ring_robust(A, oracle), side, "sino_terms")


@case("ring_terms")
def test_ring_terms(side):
    run_late(lambda A: G().case_ring_terms(A), side, "ring_terms")


@case("halo_staging")
def test_halo_staging(side):
    run_late(lambda A: G().case_halo_staging(A), side, "halo_staging")


@case("stream_kernels")
def test_stream_kernels(side):
    run_late(lambda A: G().case_stream_kernels(A, 4099, 0), side, "stream_kernels")


@case("diag_stream")
def test_diag_stream(side):
    """tomo_diag_stream has no suite: it is a measuring kernel.  What its source states -- every output k receives the sum of the
    inputs, accumulated in their order from 0, plus k (the float4 form adds k to the first lane of a quad only) -- is held bit
    for bit, dword and float4 form."""
    rng = np.random.default_rng(12)
    n = 4100
    ins = [rng.standard_normal(n).astype(np.float32) for _ in range(3)]
    acc = np.zeros(n, np.float32)
    for a in ins:
        acc = acc + a

    def body(A):
        for vec in (1, 4):
            ind = [A.ro(a) for a in ins]
            outs = [A.out((n,)) for _ in range(2)]
            pi = (C.c_void_p * 3)(*[g.view.data_ptr() for g in ind])
            po = (C.c_void_p * 2)(*[g.view.data_ptr() for g in outs])
            ok(lib().tomo_diag_stream(pi, 3, po, 2, n, vec, 3, cur()))
            for k, g in enumerate(outs):
                want = acc + F32(k)
                if vec == 4:       # the float4 form adds k to the first lane of each quad only
                    want = acc.copy()
                    want[0::4] += F32(k)
                same_bits(g.host(), want, ("diag_stream", vec, k))
    run_late(body, side, "diag_stream")


# ---- the funnelled operators, through the functions their suites use
TV_SHAPES = [(6, 9, 13), (24, 19)]       # of tests/test_gpu_parity.py::TV_SHAPES: the smallest 3D and the 2D one


def _tv_input(shape, shifted):
    """as tests/test_gpu_parity.py::test_pdtv_default_arithmetic_vs_oracle forms it"""
    rng = np.random.default_rng(5)
    x = (rng.random(shape) * 0.3 + (np.indices(shape)[-1] > shape[-1] // 2)).astype(np.float32)
    return (x - 0.6).astype(np.float32) if shifted else x


def _pdtv_cases(oracle):
    for shape in TV_SHAPES:
        for half in (False, True):
            x = _tv_input(shape, True)
            yield shape, half, x, oracle.pd_tv(x, 0.04, 11, 0, 1, 8.0, half).reshape(shape)


def _pdtv_body(oracle, pd_arith, call, what):
    from test_gpu_parity import TV_SHAPES as theirs
    assert all(s in theirs for s in TV_SHAPES)
    cases = list(_pdtv_cases(oracle))

    def body(A):
        for shape, half, x, want in cases:
            xd, out = A.ro(x), A.out(shape)
            call(xd.view, out.view, half)
            pd_arith.check(out.host(), want, half=half, what=f"{what} {shape} on a side stream")
        A.check(what)
    return body


@case("pdtv")
def test_pdtv(oracle, pd_arith, side):
    from tomobar_amd import ops
    s = oracle.pd_scalars(0.04, 8.0)
    run_late(_pdtv_body(oracle, pd_arith, lambda x, out, half: ops.pdtv(x, out, *s, 11, 0, 1, half), "pdtv"), side, "pdtv")


def _roftv_body(oracle, call):
    cases = [(shape, half, _tv_input(shape, False)) for shape in TV_SHAPES for half in (False, True)]
    cases = [(shape, half, x, oracle.rof_tv(x, 0.05, 11, 0.005, half).reshape(shape)) for shape, half, x in cases]

    def body(A):
        for shape, half, x, want in cases:
            xd, out = A.ro(x), A.out(shape)
            call(xd.view, out.view, half)
            assert np.array_equal(out.host(), want), (shape, half)
        A.check("roftv")
    return body


@case("roftv")
def test_roftv(oracle, side):
    from tomobar_amd import ops
    run_late(_roftv_body(oracle, lambda x, out, half: ops.roftv(x, out, F32(0.05), F32(0.005), 11, half)), side, "roftv")


def _tol_stopped(A, name, pd_arith):
    """a *_tol entry with tol > 0 on a case of tests/_tolerance_cases.py, as tests/test_gpu_tolerance.py::_inner_case holds it:
    stops where the oracle's sequence stops, returns that iterate"""
    import _tolerance_cases as T
    from tomobar_amd import ops
    method, _, kw, _ = T.INNER_CASES[name]
    half = bool(kw.get("half_precision", False))
    tol, stop, d_stop, _ = T.inner_plan(name)
    x = T.inner_input(name)
    want = T.inner_oracle(name, stop).reshape(x.shape)
    xd, out = A.ro(x), A.out(x.shape)
    if method == "PD_TV":
        _, done, d = ops.pdtv_tol(xd.view, out.view, *T.O.pd_scalars(kw["regularisation_parameter"], 8.0), T.INNER_ITERATIONS,
                                  kw.get("methodTV", 0), kw.get("nonneg", 0), half, tol)
    else:
        _, done, d = ops.roftv_tol(xd.view, out.view, F32(kw["regularisation_parameter"]), F32(kw["time_marching_parameter"]),
                                   T.INNER_ITERATIONS, half, tol)
    assert done == stop, (name, done, stop)
    got = out.host()
    if pd_arith is not None:
        pd_arith.check(got, want, half=half, what=f"{name} stopped after {stop} on a side stream")
    else:
        assert np.array_equal(got, want), name
    if method == "ROF_TV" or half or pd_arith.exact:
        assert abs(d - d_stop) <= got.size * T.EPS53 * d_stop, (d, d_stop)


@case("pdtv_tol")
def test_pdtv_tol(oracle, pd_arith, side):
    """tol == 0 is tomo_pdtv and asynchronous; tol > 0 reads the change back at every check"""
    from tomobar_amd import ops
    s = oracle.pd_scalars(0.04, 8.0)

    def zero(x, out, half):
        _, done, d = ops.pdtv_tol(x, out, *s, 11, 0, 1, half, 0.0)
        assert done == 11 and math.isnan(d)
    run_late(_pdtv_body(oracle, pd_arith, zero, "pdtv_tol, tol 0"), side, "pdtv_tol", "pdtv_tol, tol 0")
    with torch.cuda.stream(side):
        for delayed in (False, True):
            _tol_stopped(S.Late(side, delayed=delayed, asynchronous=False, label="pdtv_tol, tol > 0"), "pd_2d", pd_arith)


@case("roftv_tol")
def test_roftv_tol(oracle, side):
    from tomobar_amd import ops

    def zero(x, out, half):
        _, done, d = ops.roftv_tol(x, out, F32(0.05), F32(0.005), 11, half, 0.0)
        assert done == 11 and math.isnan(d)
    run_late(_roftv_body(oracle, zero), side, "roftv_tol", "roftv_tol, tol 0")
    with torch.cuda.stream(side):
        for delayed in (False, True):
            _tol_stopped(S.Late(side, delayed=delayed, asynchronous=False, label="roftv_tol, tol > 0"), "rof_2d_half", None)


MARCH_SHAPES = [(7, 13, 37), (13, 37)]      # the first 3D and the first 2D shape of the marching suites


@case("tgv")
def test_tgv(side):
    import test_gpu_tgv as TG
    from tomobar_amd import ops
    T = TG.T
    assert MARCH_SHAPES[0] in TG.SHAPES_3D and MARCH_SHAPES[1] in TG.SHAPES_2D
    wants = [(shape, T.phantom(shape), T.cached(shape, "A", TG.COUNTS)[7]) for shape in MARCH_SHAPES]

    def body(A):
        for shape, f, want in wants:
            xd, out = A.ro(f), A.out(shape)
            _, done, d = ops.tgv(xd.view, out.view, *TG._scalars(T.PARAMS_A), 7, 0.0)
            assert done == 7 and math.isnan(d)
            same_bits(out.host(), want, ("tgv", shape))
        A.check("tgv")
    run_late(body, side, "tgv")


def _march_case(name, side):
    import _march_gpu as MG
    import _march_gpu_suite as MS
    from _tgv_oracle import phantom
    D = MG.OPS[name].oracle
    p = D.PARAMS["A"]
    assert all(s in MS.SHAPES[name] for s in MARCH_SHAPES)
    wants = [(shape, phantom(shape), D.cached(shape, "A", MS.COUNTS)[7]) for shape in MARCH_SHAPES]

    def body(A):
        for shape, f, want in wants:
            xd, out = A.ro(f), A.out(shape)
            _, done, d = MG.ops_fn(name)(xd.view, out.view, *MG.f32(D, p), *(p[k] for k in D.extra), 7, 0.0)
            assert done == 7 and math.isnan(d)
            same_bits(out.host(), want, (name, shape))
        A.check(name)
    run_late(body, side, name.lower())


@case("ndf")
def test_ndf(side):
    _march_case("NDF", side)


@case("diff4th")
def test_diff4th(side):
    _march_case("Diff4th", side)


@case("llt_rof")
def test_llt_rof(side):
    _march_case("LLT_ROF", side)


# ---- the PDHG / SPDHG step kernels on one shape of tests/_pdhg_cases.MARCH_SHAPES, one step
STEP_SHAPE, STEP_KIND = (3, 5, 63), "noise"


def _zeros(A, shape, nd):
    return [A.rw(np.zeros(shape, np.float32)) for _ in range(nd)]


@case("pdhg_marches")
def test_pdhg_marches(side):
    import _pdhg_cases as K
    from tomobar_amd import ops
    shape = STEP_SHAPE
    assert shape in K.MARCH_SHAPES and 1 in K.MARCH_COUNTS
    x0, g_host, lam = K.march_input(STEP_KIND, shape), K.march_g(shape), K.MARCH_LAMBDA[STEP_KIND]
    wants = {(mtv, nn): K.march_oracle(STEP_KIND, shape, mtv, nn)[0][1] for mtv in (0, 1) for nn in (0, 1)}

    def body(A):
        for (mtv, nn), (wx, wb, wq) in wants.items():
            x, xbar, g, q = A.rw(x0), A.rw(x0), A.ro(g_host), _zeros(A, shape, 3)
            ops.pdhg_tv_dual(xbar.view, [t.view for t in q], K.MARCH_SIGMA, lam, mtv)
            ops.pdhg_primal(x.view, xbar.view, g.view, [t.view for t in q], K.MARCH_TAU, nn)
            same_bits(x.host(), wx, ("pdhg x", mtv, nn))
            same_bits(xbar.host(), wb, ("pdhg x-bar", mtv, nn))
            for d in range(3):
                same_bits(q[d].host(), wq[d], ("pdhg q", d, mtv, nn))
        A.check("pdhg marches")
    run_late(body, side, "pdhg_marches")


@case("pdhg_diag")
def test_pdhg_diag(side):
    import _pdhg_cases as K
    import _pdhg_diag_oracle as D
    import test_gpu_pdhg_diag as TD
    from tomobar_amd import ops
    shape, sino_shape = STEP_SHAPE, (5, 23, 48)
    assert sino_shape in TD.SINO_EXTENTS
    sums = TD._row_sums(sino_shape)
    steps_want = D.diag_steps(sums, TD.NUMER, F32(0))
    y, r, b = TD._sino_inputs(sino_shape)
    duals = {fid: D.sino_dual(y, r, b, fid, steps_want) for fid in TD.P.FIDELITIES}
    x0, g_host, lam = K.march_input(STEP_KIND, shape), K.march_g(shape), K.MARCH_LAMBDA[STEP_KIND]
    tau = TD._tau_field(shape, True)
    primal = {nn: D.march_steps(x0, g_host, K.MARCH_SIGMA, tau, lam, 0, nn, K.MARCH_COUNTS)[1] for nn in (0, 1)}

    def body(A):
        sg, og = A.ro(sums), A.out(sino_shape)
        ops.pdhg_diag_steps(og.view, sg.view, TD.NUMER, F32(0))
        same_bits(og.host(), steps_want, "diag_steps")
        for fid, want in duals.items():
            yd, rd, bd, sd = A.rw(y), A.ro(r), A.ro(b), A.ro(steps_want)
            ops.pdhg_sino_dual_diag(yd.view, rd.view, bd.view, sd.view, fid)
            same_bits(yd.host(), want, ("sino_dual_diag", fid))
        for nn, (wx, wb, wq) in primal.items():
            x, xbar, g, t, q = A.rw(x0), A.rw(x0), A.ro(g_host), A.ro(tau), _zeros(A, shape, 3)
            ops.pdhg_tv_dual(xbar.view, [a.view for a in q], K.MARCH_SIGMA, lam, 0)
            ops.pdhg_primal_diag(x.view, xbar.view, g.view, [a.view for a in q], t.view, nn)
            same_bits(x.host(), wx, ("primal_diag x", nn))
            same_bits(xbar.host(), wb, ("primal_diag x-bar", nn))
            for d in range(3):
                same_bits(q[d].host(), wq[d], ("primal_diag q", d, nn))
        A.check("pdhg diag")
    run_late(body, side, "pdhg_diag")


@case("pdhg_tgv")
def test_pdhg_tgv(side):
    import _pdhg_cases as K
    import _pdhg_tgv_cases as T
    import test_gpu_pdhg_tgv as TT
    from tomobar_amd import ops
    shape = STEP_SHAPE
    x0, g_host = K.march_input(STEP_KIND, shape), K.march_g(shape)
    r1, r0 = T.MARCH_RADII[STEP_KIND]
    wants = {pv: T.march_oracle(STEP_KIND, shape, 1, pv)[0][1] for pv in (False, True)}
    start = T.march_state(shape)

    def body(A):
        for per_voxel, want in wants.items():
            x, xbar, g = A.rw(x0), A.rw(x0), A.ro(g_host)
            tau = A.ro(T.march_tau(shape)) if per_voxel else None
            bands = {name: [A.rw(a) for a in start[name]] for name in TT.GROUPS}
            f = {name: [t.view for t in bands[name]] for name in TT.GROUPS}
            ops.pdhg_tgv_dual(xbar.view, f["vbar"], f["p"], f["q"], T.MARCH_SIGMA_P, T.MARCH_SIGMA_Q, r1, r0)
            ops.pdhg_tgv_primal(x.view, xbar.view, g.view, f["v"], f["vbar"], f["p"], f["q"],
                                tau.view if per_voxel else T.MARCH_TAU_X, T.MARCH_TAU_V, 1)
            same_bits(x.host(), want["x"], ("pdhg_tgv x", per_voxel))
            same_bits(xbar.host(), want["xbar"], ("pdhg_tgv x-bar", per_voxel))
            for name in TT.GROUPS:
                for k, t in enumerate(bands[name]):
                    same_bits(t.host(), want[name][k], ("pdhg_tgv", name, k, per_voxel))
        A.check("pdhg tgv")
    run_late(body, side, "pdhg_tgv")


@case("pdhg_stripe")
def test_pdhg_stripe(side):
    """3 planes, 130 angles (three segments, the last one of 2 rows), 260 columns (one full 256-column block and a tail)"""
    import _pdhg_stripe_cases as SC
    import _pdhg_stripe_oracle as SO
    from tomobar_amd import ops
    y0, r, b, sig, sbar = SC.kernel_inputs(3, 130, 260)
    s0, part0 = SC.update_inputs(3, 130, 260)
    want_s, want_sbar = SO.stripe_update(s0, part0, SC.KERNEL_TAU_S, SC.KERNEL_THETA)

    for per_sample in (False, True):
        want_y, want_part = SO.sino_dual_stripe(y0, r, b, sbar, "KL", sig if per_sample else SC.KERNEL_SIGMA)

        def dual(A):
            y, rd, bd, sb, part = A.rw(y0), A.ro(r), A.ro(b), A.ro(sbar), A.out(want_part.shape)
            sg = A.ro(sig) if per_sample else None
            ops.pdhg_sino_dual_stripe(y.view, rd.view, bd.view, sb.view, part.view, "KL", sg.view if per_sample else SC.KERNEL_SIGMA)
            same_bits(y.host(), want_y, "y")          # (the first read-back asserts `still_busy`)
            same_bits(part.host(), want_part, "part")
            A.check("fused dual")
        run_late(dual, side, "pdhg_stripe", "pdhg_sino_dual_stripe, " + ("per sample" if per_sample else "scalar"))

    def update(A):
        s, part, sb = A.rw(s0), A.ro(part0), A.out(s0.shape)
        ops.pdhg_stripe_update(s.view, sb.view, part.view, 130, SC.KERNEL_TAU_S, SC.KERNEL_THETA)
        same_bits(s.host(), want_s, "s")
        same_bits(sb.host(), want_sbar, "s-bar")
        A.check("stripe update")
    run_late(update, side, "pdhg_stripe", "pdhg_stripe_update")


@case("spdhg_tv")
def test_spdhg_tv(side):
    import _pdhg_cases as K
    import _spdhg_cases as SK
    from tomobar_amd import ops
    shape = STEP_SHAPE
    x0, z0, lam = K.march_input(STEP_KIND, shape), SK.tv_z0(shape), K.MARCH_LAMBDA[STEP_KIND]
    wants = {(mtv, nn): SK.tv_oracle(STEP_KIND, shape, mtv, nn)[0][1] for mtv in (0, 1) for nn in (0, 1)}

    def body(A):
        for (mtv, nn), (wx, wz, wq, we) in wants.items():
            x, z, q = A.rw(x0), A.rw(z0), _zeros(A, shape, 3)
            e = [A.out(shape) for _ in range(3)]          # e is written, never read first
            ops.spdhg_tv_dual(x.view, [t.view for t in q], [t.view for t in e], K.MARCH_SIGMA, lam, mtv)
            ops.spdhg_tv_primal(x.view, z.view, [t.view for t in e], K.MARCH_TAU, SK.TV_W, nn)
            same_bits(x.host(), wx, ("spdhg x", mtv, nn))
            same_bits(z.host(), wz, ("spdhg z", mtv, nn))
            for d in range(3):
                same_bits(q[d].host(), wq[d], ("spdhg q", d, mtv, nn))
                same_bits(e[d].host(), we[d], ("spdhg e", d, mtv, nn))
        A.check("spdhg tv")
    run_late(body, side, "spdhg_tv")


# ---- scratch entry points
@case("reserve_scratch")
def test_reserve_scratch(oracle, pd_arith, side):
    """tomo_reserve_scratch for an arena that is large enough already (the warm pass grew it) is asynchronous, and the
    operator that follows finds its scratch on the same stream"""
    from tomobar_amd import ops
    shape = TV_SHAPES[0]
    x = _tv_input(shape, True)
    want = oracle.pd_tv(x, 0.04, 11, 0, 1, 8.0, False)
    s = oracle.pd_scalars(0.04, 8.0)

    def body(A):
        xd, out = A.ro(x), A.out(shape)
        xd.view
        ops.reserve_tv_scratch(shape, "cuda:0", "PD_TV", False)
        ops.pdtv(xd.view, out.view, *s, 11, 0, 1, False)
        pd_arith.check(out.host(), want, what="pdtv after reserve_scratch on a side stream")
    run_late(body, side, "reserve_scratch")


@case("placed_scratch")
def test_placed_scratch(side):
    """tomo_placed_scratch (ops.pdhg_work_arrays, the PDHG driver's allocator): the block of the stream the call names, taken
    while the delay is pending; the PDHG step runs in it"""
    import _pdhg_cases as K
    from tomobar_amd import ops
    shape = STEP_SHAPE
    x0, g_host, lam = K.march_input(STEP_KIND, shape), K.march_g(shape), K.MARCH_LAMBDA[STEP_KIND]
    wx, wb, wq = K.march_oracle(STEP_KIND, shape, 0, 1)[0][1]
    seen = []

    def body(A):
        x, start, gd = A.rw(x0), A.ro(x0), A.ro(g_host)
        x.view
        xbar, g, q, lease = ops.pdhg_work_arrays(shape, "cuda:0", True)
        seen.append(xbar.data_ptr())
        xbar.copy_(start.view)
        g.copy_(gd.view)
        for t in q:
            t.zero_()
        ops.pdhg_tv_dual(xbar, q, K.MARCH_SIGMA, lam, 0)
        ops.pdhg_primal(x.view, xbar, g, q, K.MARCH_TAU, 1)
        same_bits(x.host(), wx, "x")
        assert ops.lease_is_current(lease)
        same_bits(A.read(xbar), wb, "x-bar in the placed block")
        for d in range(3):
            same_bits(A.read(q[d]), wq[d], ("q in the placed block", d))
    run_late(body, side, "placed_scratch")
    assert seen[0] == seen[1], "the same request on the same stream returns the same block"


# ---- the z-slab entries through the single-GPU slab runners
@case("pdtv_slabs")
@pytest.mark.parametrize("half", [False, True])
def test_pdtv_slabs(side, half):
    """7 iterations in the overlapped schedule: launches of 3, 3 (tomo_pdtv_multi_slab_range; binary16: 2, 2, 2) and a
    trailing single iteration (tomo_pdtv_iter_slab)"""
    from test_gpu_slab import run_pdtv_slabs
    run_late(lambda A: run_pdtv_slabs(2, half, "ranges", iters_list=(7,), to_device=lambda v: A.ro(v).view, to_host=A.read),
             side, "pdtv_slabs", f"pdtv_slabs half={half}")


@case("roftv_slabs")
def test_roftv_slabs(side):
    from test_gpu_slab import run_roftv_slabs
    run_late(lambda A: run_roftv_slabs(2, False, to_device=lambda v: A.ro(v).view, to_host=A.read), side, "roftv_slabs")


@case("march_slabs")
@pytest.mark.parametrize("name", ["NDF", "Diff4th", "LLT_ROF"])
def test_march_slabs(monkeypatch, side, name):
    """tests/_march_gpu.run_slabs, its read-back replaced by one on the side stream, against the oracle as
    check_slabs_equal_whole_volume holds the whole volume"""
    import _march_gpu as MG
    from _tgv_oracle import phantom
    from tomobar_amd.slab import slab_bounds
    shape, iters = (19, 21, 90), 6
    want = MG.OPS[name].oracle.cached(shape, "A", (iters,))[iters]
    f = phantom(shape)

    def body(A):
        with monkeypatch.context() as m:
            m.setattr(MG, "host", A.read)
            got = MG.run_slabs(name, A.ro(f).view, [slab_bounds(shape[0], 2, r) for r in range(2)], "ranges", "A", iters)
        same_bits(got, want, (name, "slabs on a side stream"))
    assert "tomo_" + name.lower() + "_iter_slab_range" in ST.CASES["march_slabs"][1]
    run_late(body, side, "march_slabs", f"march_slabs {name}")


def test_every_case_of_the_table_has_its_test():
    assert sorted(REGISTERED) == sorted(ST.CASES)


# ================================================================================================ 3. two streams at once
def interleave(streams, job, label, rounds=4, asynchronous=True):
    """`job` = (make, run): `make(k, provider)` the late arrays of one call on stream k, `run(k, arrays)` the operator on them,
    returning [(array, check)].  Warm on each stream, then `rounds` times on each stream in turn, each stream behind its own
    delay: the pattern of tests/test_gpu_parity.py::test_back_projection_relay_scratch_is_per_stream.  Every array is made
    before the first delay is enqueued (tests/_on_stream.py: staging waits), every result is read on its own stream."""
    make, run = job
    for k, s in enumerate(streams):
        with torch.cuda.stream(s):
            W = S.Late(s, delayed=False, label=label)
            run(k, [make(k, W) for _ in range(rounds)][0])
            s.synchronize()
            W.close()
    provs = [S.Late(s, asynchronous=asynchronous, label=f"{label}, {rounds} rounds on two streams") for s in streams]
    made = [[make(k, provs[k]) for _ in range(rounds)] for k in range(len(streams))]
    pending = [[] for _ in streams]
    for r in range(rounds):
        for k, s in enumerate(streams):
            with torch.cuda.stream(s):
                pending[k] += run(k, made[k][r])
    for p in provs:
        p.returned()              # both streams still hold their delay: everything above is in flight
    for k, p in enumerate(provs):
        assert len(pending[k]) >= rounds
        for arr, check in pending[k]:
            check(arr.host() if hasattr(arr, "host") else p.read(arr), k)
    assert not asynchronous or all(p.asserted == 1 for p in provs)


def _other(x):
    """the second stream's input where a suite has one input per shape: mirrored along x and scaled"""
    return np.ascontiguousarray(np.flip(x, axis=-1) * F32(0.75))


def _simple_job(inputs, wants, call, check):
    """one read-only input, one output of its shape"""
    def make(k, A):
        return A.ro(inputs[k]), A.out(inputs[k].shape)

    def run(k, arrays):
        xd, out = arrays
        call(xd.view, out.view)
        return [(out, lambda got, k: check(got, wants[k], k))]
    return make, run


@pytest.mark.parametrize("iters", [11, 4])
@pytest.mark.parametrize("half", [False, True], ids=["float32", "binary16"])
@pytest.mark.parametrize("shape", TV_SHAPES, ids=["3d", "2d"])
def test_two_streams_pdtv(oracle, pd_arith, streams, shape, half, iters):
    """11 iterations begin with a launch that takes "the duals are zero" as a flag; 4 = 2 + 2 begin, in 3D, with one that reads
    duals the host zeroes with hipMemsetAsync (pd_plan of tv_kernels.hip): with four calls in flight that memset has to be
    ordered behind the call before it"""
    from tomobar_amd import ops
    s = oracle.pd_scalars(0.04, 8.0)
    inputs = [_tv_input(shape, True), _other(_tv_input(shape, True))]
    wants = [oracle.pd_tv(x, 0.04, iters, 0, 1, 8.0, half).reshape(shape) for x in inputs]
    interleave(streams, _simple_job(inputs, wants, lambda x, out: ops.pdtv(x, out, *s, iters, 0, 1, half),
                                    lambda got, want, k: pd_arith.check(got, want, half=half, what=f"pdtv {shape} stream {k}")),
               f"pdtv {shape} half={half} iterations={iters}")


def test_two_streams_roftv(oracle, streams):
    from tomobar_amd import ops
    shape = TV_SHAPES[0]
    inputs = [_tv_input(shape, False), _other(_tv_input(shape, False))]
    wants = [oracle.rof_tv(x, 0.05, 11, 0.005, False) for x in inputs]

    def check(got, want, k):
        assert np.array_equal(got, want), ("roftv", k)
    interleave(streams, _simple_job(inputs, wants, lambda x, out: ops.roftv(x, out, F32(0.05), F32(0.005), 11, False), check), "roftv")


def test_two_streams_slicewise(oracle, pd_arith, streams):
    import _slicewise_cases as SC
    from test_gpu_slicewise import pd, rof
    shape, iters = (3, 9, 59), 7
    assert (shape, iters) in SC.PD_CASES and (shape, iters) in SC.ROF_CASES
    inputs = [SC.volume(shape), SC.volume(shape, seed=1)]
    assert not np.array_equal(*inputs)
    kw_pd, kw_rof = SC.pd_kwargs(iters), SC.rof_kwargs(iters)
    want_pd = [SC.oracle_slices("PD_TV", v, **kw_pd) for v in inputs]
    want_rof = [SC.oracle_slices("ROF_TV", v, **kw_rof) for v in inputs]

    def rof_check(got, want, k):
        assert np.array_equal(got, want), ("slice-wise ROF_TV", k)
    interleave(streams, _simple_job(inputs, want_pd, lambda x, out: pd(x, slicewise=True, out=out, **kw_pd),
                                    lambda got, want, k: pd_arith.check(got, want, what=f"slice-wise PD_TV stream {k}")),
               "slice-wise PD_TV")
    interleave(streams, _simple_job(inputs, want_rof, lambda x, out: rof(x, slicewise=True, out=out, **kw_rof), rof_check),
               "slice-wise ROF_TV")


def _bits_check(what):
    return lambda got, want, k: same_bits(got, want, (what, "stream", k))


def test_two_streams_tgv(streams):
    import test_gpu_tgv as TG
    from tomobar_amd import ops
    T = TG.T
    shape = MARCH_SHAPES[0]
    inputs = [T.phantom(shape), _other(T.phantom(shape))]
    wants = [T.tgv(f, iterations=7, **T.PARAMS_A) for f in inputs]
    same_bits(wants[0], T.cached(shape, "A", TG.COUNTS)[7], "the oracle run is the cached one")
    interleave(streams, _simple_job(inputs, wants, lambda x, out: ops.tgv(x, out, *TG._scalars(T.PARAMS_A), 7, 0.0), _bits_check("tgv")),
               "tgv")


@pytest.mark.parametrize("name", ["NDF", "Diff4th", "LLT_ROF"])
def test_two_streams_marching(streams, name):
    import _march_gpu as MG
    from _tgv_oracle import phantom
    D = MG.OPS[name].oracle
    p = D.PARAMS["A"]
    shape = MARCH_SHAPES[0]
    inputs = [phantom(shape), _other(phantom(shape))]
    wants = [D.run(f, 7, **p) for f in inputs]
    same_bits(wants[0], D.cached(shape, "A", (1, 2, 7, 40))[7], "the oracle run is the cached one")
    interleave(streams, _simple_job(inputs, wants,
                                    lambda x, out: MG.ops_fn(name)(x, out, *MG.f32(D, p), *(p[k] for k in D.extra), 7, 0.0),
                                    _bits_check(name)), name)


def test_two_streams_nltv(streams):
    import _nltv_oracle as N
    import test_gpu_nltv as TN
    from tomobar_amd import ops
    shape, params, lam, n = (13, 37), (7, 2, 15), 0.02, 2
    h = TN.INPUTS["noisy"][1]
    imgs = [np.array(TN.oracle_tables("noisy", shape, params)[0]), _other(np.array(TN.oracle_tables("noisy", shape, params)[0]))]
    tables = [TN.oracle_tables("noisy", shape, params)[1], N.patch_select(imgs[1], *params, h)]
    wants = [N.nltv(img, *t, lam, n) for img, t in zip(imgs, tables)]

    def make(k, A):
        return A.ro(imgs[k]), A.out(shape), [A.ro(np.array(a)) for a in tables[k]]

    def run(k, arrays):
        xd, out, t = arrays
        ops.nltv(xd.view, out.view, *(g.view for g in t), F32(lam), n, 0.0)
        return [(out, lambda got, k: same_bits(got, wants[k], ("nltv, stream", k)))]
    interleave(streams, (make, run), "nltv")


def test_two_streams_wavelet_shrink(streams):
    import _wavelet_oracle as W
    from test_gpu_wavelets import want
    from _tgv_oracle import phantom
    from tomobar_amd import ops
    shape, t = (7, 13, 37), 0.02
    inputs = [phantom(shape), _other(phantom(shape))]
    wants = [want(shape, t)[1], None]
    wants[1] = _wavelet_shrink_oracle(W, inputs[1], t)
    same_bits(_wavelet_shrink_oracle(W, inputs[0], t), wants[0], "the oracle run is the suite's")
    interleave(streams, _simple_job(inputs, wants, lambda x, out: ops.wavelet_shrink(x, F32(t), out=out), _bits_check("wavelet_shrink")),
               "wavelet_shrink")


def _wavelet_shrink_oracle(W, f, t):
    """W_t(f) as tests/test_gpu_wavelets.py::want forms it"""
    return W.inverse(W.forward(f, t, np.float32), f.shape, np.float32)


def test_two_streams_fbp_filter_same_rows_and_nu(oracle, streams):
    """the same (rows, nu) on both streams: the plan pair, with its one work area, is per stream"""
    from test_fbp import rel
    rows, nu, cutoff = 7, 45, 0.6
    inputs = [np.random.default_rng(3 + k).random((rows, 1, nu)).astype(np.float32) for k in range(2)]
    wants = [oracle.fbp_filter(x, cutoff) for x in inputs]

    def run(k, d):
        ok(lib().tomo_fbp_filter(0, vp(d.view), rows, nu, cutoff, 1.0 / rows / nu, cur()))

        def check(got, k):
            assert np.isfinite(got).all() and rel(got, wants[k]) < 1e-5, (k, rel(got, wants[k]))
        return [(d, check)]
    interleave(streams, (lambda k, A: A.rw(inputs[k]), run), "fbp_filter")


def test_two_streams_pdhg_and_spdhg_tv_in_their_placed_blocks(streams):
    """the PDHG and SPDHG TV kernels on work arrays from tomo_placed_scratch: the block is per (device, stream, slot)"""
    import _pdhg_cases as K
    import _pdhg_oracle as P
    import _spdhg_cases as SK
    import _spdhg_oracle as SO
    from tomobar_amd import ops
    shape = STEP_SHAPE
    lam, g_host, z0 = K.MARCH_LAMBDA[STEP_KIND], K.march_g(shape), SK.tv_z0(shape)
    inputs = [K.march_input(STEP_KIND, shape), _other(K.march_input(STEP_KIND, shape))]
    pd_want = [P.march_steps(x, g_host, K.MARCH_SIGMA, K.MARCH_TAU, lam, 0, 1, (1,))[1] for x in inputs]
    sp_want = [SO.tv_steps(x, z0, K.MARCH_SIGMA, K.MARCH_TAU, lam, 0, 1, (1,), SK.TV_W, {})[1] for x in inputs]
    same_bits(pd_want[0][0], K.march_oracle(STEP_KIND, shape, 0, 1)[0][1][0], "the oracle run is the cached one")
    same_bits(sp_want[0][0], SK.tv_oracle(STEP_KIND, shape, 0, 1)[0][1][0], "the oracle run is the cached one")
    blocks = [set(), set()]

    def pdhg_make(k, A):
        return A.rw(inputs[k]), A.ro(inputs[k]), A.ro(g_host), A.out(shape)

    def pdhg_job(k, arrays):
        x, start, gd, xbar_out = arrays
        x.view
        xbar, g, q, _ = ops.pdhg_work_arrays(shape, "cuda:0", True)
        blocks[k].add(xbar.data_ptr())
        xbar.copy_(start.view)
        g.copy_(gd.view)
        for t in q:
            t.zero_()
        ops.pdhg_tv_dual(xbar, q, K.MARCH_SIGMA, lam, 0)
        ops.pdhg_primal(x.view, xbar, g, q, K.MARCH_TAU, 1)
        xbar_out.view.copy_(xbar)
        return [(x, lambda got, k: same_bits(got, pd_want[k][0], ("pdhg x, stream", k))),
                (xbar_out, lambda got, k: same_bits(got, pd_want[k][1], ("pdhg x-bar, stream", k)))]

    def spdhg_make(k, A):
        return A.rw(inputs[k]), A.ro(z0), A.out(shape)

    def spdhg_job(k, arrays):
        x, zs, z_out = arrays
        x.view
        z, _, q, e, _ = ops.spdhg_work_arrays(shape, "cuda:0", True)
        z.copy_(zs.view)
        for t in q:
            t.zero_()
        ops.spdhg_tv_dual(x.view, q, e, K.MARCH_SIGMA, lam, 0)
        ops.spdhg_tv_primal(x.view, z, e, K.MARCH_TAU, SK.TV_W, 1)
        z_out.view.copy_(z)
        return [(x, lambda got, k: same_bits(got, sp_want[k][0], ("spdhg x, stream", k))),
                (z_out, lambda got, k: same_bits(got, sp_want[k][1], ("spdhg z, stream", k)))]
    interleave(streams, (pdhg_make, pdhg_job), "pdhg tv in a placed block")
    assert len(blocks[0]) == len(blocks[1]) == 1 and blocks[0] != blocks[1], "one block per stream"
    interleave(streams, (spdhg_make, spdhg_job), "spdhg tv in a placed block")


def test_two_streams_projector_and_fused_residual_one_context_each(oracle, streams):
    """the forward projector and the fused residual with one context per stream (a context owns its transposed-volume scratch)"""
    import types
    from _cpu_backend import OracleTools3D
    g = G().GEOMS[0]
    pairs = [G()._pair(oracle, g) for _ in streams]
    P = pairs[0][0]
    rng = np.random.default_rng(4)
    vols = [rng.random((P.nz, P.n, P.n)).astype(np.float32) for _ in streams]
    b = (rng.random((P.nz, P.na, P.nu)) * 30).astype(np.float32)
    fp_want = [P.fp(v, None) for v in vols]
    res_want = []
    for k, v in enumerate(vols):
        ns = types.SimpleNamespace(_fp=lambda vol, sub, k=k: fp_want[k], _sub=lambda i: i, _idx=lambda i: slice(None))
        t = torch.empty(pairs[k][2].sino_shape(None), dtype=torch.float32)
        OracleTools3D.residual(ns, v, b, None, "LS", None, t)
        res_want.append(t.numpy())

    def make(k, A):
        shape = pairs[k][2].sino_shape(None)
        return A.ro(vols[k]), A.ro(b), A.out(shape), A.out(shape)

    def run(k, arrays):
        H = pairs[k][2]
        vd, bd, sino, res = arrays
        H.forward(vd.view, None, out=sino.view)
        H.residual(vd.view, bd.view, None, "LS", None, res.view)
        return [(sino, lambda got, k: same_bits(got, fp_want[k], ("fp, stream", k))),
                (res, lambda got, k: same_bits(got, res_want[k], ("residual, stream", k)))]
    interleave(streams, (make, run), "fp and fused residual")


# ================================================================================================ 4. scratch that changes
def _release_all():
    ok(lib().tomo_release_scratch(0))


def test_arena_growth_under_pending_work(oracle, pd_arith, side):
    """PD_TV at (6, 9, 13), then at a shape that needs a larger arena, on one stream behind a delay with no synchronisation by
    the test in between: the library has to wait for the stream before it frees the block it grew out of.  The same for the
    NDF arena and for the ARENA_MAIN of tomo_fbp_filter."""
    import _march_gpu as MG
    import _march_gpu_suite as MS
    from _tgv_oracle import phantom
    from test_fbp import rel
    from tomobar_amd import ops
    s = oracle.pd_scalars(0.04, 8.0)
    small, large = (6, 9, 13), (20, 70, 150)
    L = lib()
    assert L.tomo_pdtv_scratch_bytes(150, 70, 20, 3, 0) > L.tomo_pdtv_scratch_bytes(13, 9, 6, 3, 0)
    xs = [_tv_input(sh, True) for sh in (small, large)]
    pd_want = [oracle.pd_tv(x, 0.04, 11, 0, 1, 8.0, False) for x in xs]
    D = MG.OPS["NDF"].oracle
    p = D.PARAMS["A"]
    nshapes = [(7, 13, 37), (3, 70, 131)]
    assert all(sh in MS.SHAPES["NDF"] for sh in nshapes)
    assert L.tomo_ndf_scratch_bytes(131, 70, 3, 3) > L.tomo_ndf_scratch_bytes(37, 13, 7, 3)
    fs = [phantom(sh) for sh in nshapes]
    ndf_want = [D.cached(sh, "A", MS.COUNTS)[7] for sh in nshapes]
    nu, cutoff = 45, 0.6
    sinos = [np.random.default_rng(3).random((rows, 1, nu)).astype(np.float32) for rows in (7, 64)]
    fbp_want = [oracle.fbp_filter(x, cutoff) for x in sinos]
    with open(os.path.join(ROOT, "tomobar_amd", "csrc", "fbp_filter.hip")) as fh:
        assert "const size_t spec_bytes = rows * (size_t)nh * sizeof(float2);" in fh.read()      # the ARENA_MAIN need of a call
    assert 64 * (nu // 2 + 1) * 8 > 7 * (nu // 2 + 1) * 8

    def pdtv(xd, out):
        ops.pdtv(xd.view, out.view, *s, 11, 0, 1, False)

    def ndf(xd, out):
        ops.ndf(xd.view, out.view, *MG.f32(D, p), *(p[k] for k in D.extra), 7, 0.0)

    def fbp(d, _):
        rows = d.view.shape[0]
        ok(L.tomo_fbp_filter(0, vp(d.view), rows, nu, cutoff, 1.0 / rows / nu, cur()))

    def fbp_check(got, want, what):
        assert np.isfinite(got).all() and rel(got, want) < 1e-5, (what, rel(got, want))

    parts = [("pdtv", pdtv, xs, pd_want, False, lambda got, want, what: pd_arith.check(got, want, what=what)),
             ("ndf", ndf, fs, ndf_want, False, same_bits),
             ("fbp_filter", fbp, sinos, fbp_want, True, fbp_check)]
    with torch.cuda.stream(side):
        for name, call, inputs, wants, in_place, check in parts:
            def make(A, x):
                return (A.rw(x), None) if in_place else (A.ro(x), A.out(x.shape))
            # the arena of this stream at the small size, and nothing pending: release, the small case warm, synchronise
            _release_all()
            W = S.Late(side, delayed=False, label="arena growth")
            call(*make(W, inputs[0]))
            side.synchronize()
            W.close()
            # small, then large, behind one delay: the arena grows while the delay and the small call are pending
            A = S.Late(side, asynchronous=False, label="arena growth")
            made = [make(A, x) for x in inputs]
            for arrays in made:
                call(*arrays)
            for (xd, out), want, x in zip(made, wants, inputs):
                check((xd if in_place else out).host(), want.reshape(x.shape), f"{name} {x.shape} across the growth of its arena")


def test_fbp_plan_eviction_under_pending_work(oracle, side):
    """ten distinct `rows` at nu = 45, then the first again, behind one delay: ten exceeds the FBP_MAX_PLANS pairs the cache
    keeps, so plans whose last execution is still pending are evicted.  Every result stays within the bound of
    tests/test_fbp.py."""
    from test_fbp import rel
    with open(os.path.join(ROOT, "tomobar_amd", "csrc", "fbp_filter.hip")) as fh:
        assert "constexpr size_t FBP_MAX_PLANS = 8;" in fh.read()
    nu, cutoff = 45, 0.6
    rows_list = list(range(3, 13)) + [3]
    assert len(set(rows_list)) == 10
    sinos = [np.random.default_rng(40 + k).random((rows, 1, nu)).astype(np.float32) for k, rows in enumerate(rows_list)]
    wants = [oracle.fbp_filter(x, cutoff) for x in sinos]
    with torch.cuda.stream(side):
        A = S.Late(side, asynchronous=False, label="fbp plan eviction")
        ds = [A.rw(x) for x in sinos]
        for d, x in zip(ds, sinos):
            ok(lib().tomo_fbp_filter(0, vp(d.view), x.shape[0], nu, cutoff, 1.0 / x.shape[0] / nu, cur()))
        for k, (d, want) in enumerate(zip(ds, wants)):
            got = d.host()
            assert np.isfinite(got).all() and rel(got, want) < 1e-5, (k, rows_list[k], rel(got, want))


def test_release_scratch_under_pending_work(oracle, pd_arith, side):
    """tomo_release_scratch(0) with work pending on the side stream, then one more PD_TV and one more FBP filter on that stream:
    both right, and so are the outputs from before the release, read back afterwards"""
    from test_fbp import rel
    from tomobar_amd import ops
    s = oracle.pd_scalars(0.04, 8.0)
    shape, rows, nu, cutoff = (6, 9, 13), 7, 45, 0.6
    xs = [_tv_input(shape, True), _other(_tv_input(shape, True))]
    pd_want = [oracle.pd_tv(x, 0.04, 11, 0, 1, 8.0, False) for x in xs]
    sinos = [np.random.default_rng(50 + k).random((rows, 1, nu)).astype(np.float32) for k in range(2)]
    fbp_want = [oracle.fbp_filter(x, cutoff) for x in sinos]
    with torch.cuda.stream(side):
        for delayed in (False, True):
            A = S.Late(side, delayed=delayed, asynchronous=False, label="release_scratch")
            ins, outs, ds = [A.ro(x) for x in xs], [A.out(shape) for _ in xs], [A.rw(x) for x in sinos]
            for k in range(2):
                ops.pdtv(ins[k].view, outs[k].view, *s, 11, 0, 1, False)
                ok(lib().tomo_fbp_filter(0, vp(ds[k].view), rows, nu, cutoff, 1.0 / rows / nu, cur()))
                if k == 0:
                    _release_all()
            for k in range(2):
                pd_arith.check(outs[k].host(), pd_want[k], what=f"pdtv {'before' if k == 0 else 'after'} release_scratch")
                got = ds[k].host()
                assert np.isfinite(got).all() and rel(got, fbp_want[k]) < 1e-5, (k, rel(got, fbp_want[k]))


# ================================================================================================ 5. the Python classes
# INTEGRATION.md, stream rule: the classes order ALL their work on torch's current stream.  One small case of each driver's own
# suite under torch.cuda.stream(side), the projection data late behind a delay, at that suite's expected value and bound.  The
# drivers read scalars back, so nothing is asserted about the stream afterwards.
def on_side(side, host_array, call):
    """call(late device tensor) under the side stream, warm and then behind the delay; the late result on the host"""
    got = None
    with torch.cuda.stream(side):
        for delayed in (False, True):
            A = S.Late(side, delayed=delayed, asynchronous=False, label="driver")
            x = A.ro(host_array)
            res = call(x.view)
            got = A.read(res if isinstance(res, torch.Tensor) else torch.from_dlpack(res))
            same_bits_any(x.host(), host_array, "the caller's array was written")
            A.close()
    return got


def same_bits_any(got, want, what):
    assert got.shape == want.shape and np.array_equal(got.view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), what


@pytest.fixture(scope="module")
def outer(golden_dir):
    return np.load(os.path.join(golden_dir, "outer_golden.npz"))


@pytest.mark.parametrize("name", ["fista_os4_pdtv", "fista_plain", "admm_pdtv"])
def test_fista_and_admm_on_the_callers_stream(outer, side, name):
    """FISTA with PD_TV over ordered subsets, plain FISTA and ADMM: cases of tests/test_gpu_recon.py against the reference's own
    Python loops (tests/golden/outer_golden.npz), its bound"""
    import test_gpu_recon as TR
    method, mk, dk, ak, reg = TR.CASES[name]
    sino = np.ascontiguousarray(outer["sino"], np.float32)
    geom = dict(sino=sino, angles=outer["angles"], nz=sino.shape[0], n=sino.shape[2], na=sino.shape[1])
    alg = dict(ak, lipschitz_const=float(outer[ak["lipschitz_const"]]))

    def call(x):
        rt = TR.make(geom, **mk)
        d = dict({"projection_data": x, "data_axes_labels_order": ["detY", "angles", "detX"]}, **dk)
        return getattr(rt, method)(d, dict(alg), None if reg is None else dict(reg))
    got = on_side(side, sino, call)
    assert got.dtype == np.float32 and got.shape == (geom["nz"], geom["n"], geom["n"])
    assert TR.rel(got, outer[name]) < TR.TOL, TR.rel(got, outer[name])


def test_osem_on_the_callers_stream(oracle, golden_dir, side):
    """tests/test_gpu_recon.py::test_osem_against_reference_python_loop, case osem_os4: the reference's loop within its bound,
    the oracle's restatement bit for bit"""
    import test_gpu_recon as TR
    from tomobar_amd.methodsIR_CuPy import RecToolsIRCuPy
    g = np.load(os.path.join(golden_dir, "osem_golden.npz"))
    os_n, alg, reg = TR.OSEM_CASES["osem_os4"]
    assert reg is None
    sino, angles = np.ascontiguousarray(g["sino"], np.float32), g["angles"]
    nz, _, n = sino.shape
    want = oracle.circular_mask(oracle.osem(oracle.Projector(nz, n, n, angles, 0.0, os_n), sino, alg["iterations"], False, None),
                                alg.get("recon_mask_radius", 1.0))

    def call(x):
        rt = RecToolsIRCuPy(n, 0, nz, 0.0, angles, n, 0, os_n)
        return rt.OSEM({"projection_data": x, "data_axes_labels_order": ["detY", "angles", "detX"]}, dict(alg), None)
    got = on_side(side, sino, call)
    assert TR.rel(got, g["osem_os4"]) < TR.TOL
    assert np.array_equal(got, want), np.abs(got - want).max()


def test_sirt_on_the_callers_stream(oracle, outer, side):
    """tests/test_gpu_recon.py::test_simple_iterative_methods_vs_oracle, the SIRT loop with the oracle's operators, its bound"""
    import test_gpu_recon as TR
    sino = np.ascontiguousarray(outer["sino"], np.float32)
    geom = dict(sino=sino, angles=outer["angles"], nz=sino.shape[0], n=sino.shape[2], na=sino.shape[1])
    want = TR.sirt_with_the_oracle(oracle, geom, 4)

    def call(x):
        return TR.make(geom).SIRT({"projection_data": x, "data_axes_labels_order": ["detY", "angles", "detX"]},
                                  {"iterations": 4, "recon_mask_radius": None})
    assert TR.rel(on_side(side, sino, call), want) < TR.TOL


def _golden_geometry(mod, outer):
    """the `golden` geometry of tests/test_gpu_pdhg.py and tests/test_gpu_spdhg.py"""
    gsino = np.ascontiguousarray(outer["sino"], np.float32)
    return mod.Geometry(4, 24, outer["angles"], gsino, outer["L_full"])


def test_pdhg_on_the_callers_stream(oracle, outer, side):
    """tests/test_gpu_pdhg.py::test_driver_equals_the_oracle_loop, case "LS+TV nonneg": bit for bit"""
    import test_gpu_pdhg as TP
    gname, d, a, r = TP.DRIVER_CASES["LS+TV nonneg"]
    assert gname == "golden"
    geo = _golden_geometry(TP, outer)
    want = TP._oracle_run(oracle, geo, d, a, r)

    def call(x):
        return geo.tools().PDHG(dict({"projection_data": x, "data_axes_labels_order": list(TP.LABELS)}, **d), TP._algorithm(geo, a), dict(r))
    same_bits(on_side(side, geo.sino, call), want, "PDHG on a side stream")


def test_spdhg_on_the_callers_stream(oracle, outer, side):
    """tests/test_gpu_spdhg.py::test_driver_equals_the_oracle_loop, case "LS+TV nonneg OS4": bit for bit"""
    import test_gpu_spdhg as TS
    gname, os_number, d, a, r = TS.DRIVER_CASES["LS+TV nonneg OS4"]
    assert gname == "golden"
    geo = _golden_geometry(TS, outer)
    want = TS._oracle_run(oracle, geo, os_number, d, a, r)

    def call(x):
        return geo.tools(os_number).SPDHG(dict({"projection_data": x, "data_axes_labels_order": list(TS.LABELS)}, **d),
                                          TS._algorithm(geo, a), dict(r))
    same_bits(on_side(side, geo.sino, call), want, "SPDHG on a side stream")


def test_fbp_on_the_callers_stream(oracle, side):
    """tests/test_fbp.py::test_FBP_end_to_end_vs_oracle, its first case and bound"""
    from test_fbp import rel
    from tomobar_amd.methodsDIR_CuPy import RecToolsDIRCuPy
    nz, n, na = 6, 48, 40
    angles = np.linspace(0, np.pi, na, endpoint=False)
    data = np.ascontiguousarray(np.swapaxes(oracle.shepp_logan_sino(n, nz, n, angles), 0, 1))        # [angles, detY, detX]
    want = oracle.fbp(oracle.Projector(nz, n, n, angles), data, 0.35)
    got = on_side(side, data, lambda x: RecToolsDIRCuPy(n, 0, nz, 0.0, angles, n, device_projector=0).FBP(x))
    assert got.shape == (nz, n, n) and rel(got, want) < 1e-5


def test_fourier_inv_on_the_callers_stream(side):
    """tests/test_fourier.py::test_FOURIER_INV_vs_oracle_and_fixture at its smallest case, its bounds"""
    import test_fourier as TF
    from oracle import fourier_oracle as FO
    golden = np.load(os.path.join(TF.HERE, "golden", "fourier_golden.npz"))
    case = min(TF.CASES, key=lambda c: golden[c[0] + "_sino"].size)
    name, kw = case[0], case[7]
    assert "data_axes_labels_order" not in kw
    sino = np.ascontiguousarray(golden[name + "_sino"], np.float32)
    got = on_side(side, sino, lambda x: TF._tools(case, golden).FOURIER_INV(x, **kw))
    want = golden[name + "_rec"]
    assert got.shape == want.shape and TF.rel(got, want) < TF.TOL and TF.worst_slice(got, want) < 5 * TF.TOL
    assert TF.rel(got, TF._oracle_run(FO, golden, case)) < TF.TOL


def test_regularisers_on_the_callers_stream(oracle, pd_arith, side):
    """the *_cupy functions on a late array: PD_TV and ROF_TV against the oracle as tests/test_gpu_parity.py holds them, TGV, NDF,
    Diff4th and LLT_ROF against the restatements as their suites' *_cupy tests do"""
    import _march_gpu as MG
    import _march_gpu_suite as MS
    import test_gpu_tgv as TG
    from tomobar_amd.regularisersCuPy import PD_TV_cupy, ROF_TV_cupy
    shape = TV_SHAPES[0]
    x = _tv_input(shape, True)
    got = on_side(side, x, lambda t: PD_TV_cupy(t, 0.04, 11, 0, 1, 8.0, 0, False))
    pd_arith.check(got, oracle.pd_tv(x, 0.04, 11, 0, 1, 8.0, False), what="PD_TV_cupy on a side stream")
    x = _tv_input(shape, False)
    got = on_side(side, x, lambda t: ROF_TV_cupy(t, 0.05, 11, 0.005, 0, False))
    assert np.array_equal(got, oracle.rof_tv(x, 0.05, 11, 0.005, False))
    vol = TG.T.phantom((7, 13, 37))
    same_bits(on_side(side, vol, lambda t: TG._tgv_cupy(t)), TG.T.cached((7, 13, 37), "A", TG.COUNTS)[7], "TGV_cupy")
    for name in ("NDF", "Diff4th", "LLT_ROF"):
        want = MG.OPS[name].oracle.cached((7, 13, 37), "B", MS.COUNTS)[7]
        same_bits(on_side(side, vol, lambda t: MG.cupy(name, t, pname="B")), want, name + "_cupy")


def test_wavelets_and_nltv_cupy_on_the_callers_stream(side):
    """WAVELETS_cupy as tests/test_gpu_wavelets.py::test_wavelets_cupy_surface holds it, PatchSelect_cupy then NLTV_cupy as
    tests/test_gpu_nltv.py::test_patch_select_cupy_then_nltv_cupy_equals_the_oracle_chain does"""
    import test_gpu_nltv as TN
    from _tgv_oracle import phantom
    from test_gpu_wavelets import want
    from tomobar_amd.regularisersCuPy import NLTV_cupy, PatchSelect_cupy, WAVELETS_cupy
    shape = (7, 13, 37)
    same_bits(on_side(side, phantom(shape), lambda t: WAVELETS_cupy(t, 0.02, 0)), want(shape, 0.02)[1], "WAVELETS_cupy")
    params = (3, 1, 8)
    img, _ = TN.oracle_tables("noisy", shape, params)
    got = on_side(side, np.array(img), lambda t: NLTV_cupy(t, *PatchSelect_cupy(t, *params, 0.3), 0.5, 5))
    same_bits(got, TN.oracle_iterates(shape, params, 0.5, TN.COUNTS)[5], "PatchSelect_cupy, then NLTV_cupy")
