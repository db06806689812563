"""MI355X: the operators that have no funnel, with every array a call reads or writes inside guard bands
(tests/_guarded.py).  A store outside an array damages a band; a load from outside an array returns the band's NaN and shows
in the values.  Each case is held to the oracle of the operator's own suite, at that suite's strictness -- the expected
values are imported from those suites, not restated --, every band must be intact and every read-only input bit-identical
afterwards.  Buffers whose size the API fixes (tomo_ctx_residual_elems, tomo_ctx_volume_elems, wavelet_pyramid_floats,
tomo_halo_staging_bytes) hold exactly that many elements, so the band begins where the contract ends.

The last section takes the streaming kernels past one grid of threads, where their grid-stride loops start a second trip."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from _guarded import guarded  # noqa: E402
from _march_gpu import same_bits  # noqa: E402

F32 = np.float32


def vp(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def lib():
    from tomobar_amd import _lib as L
    return L.lib()


def ok(rc):
    from tomobar_amd import _lib as L
    L.check(rc)


class Arrays:
    """the guarded arrays of one case: `ro` read-only inputs, `rw` arrays the call writes (given contents) and `out` NaN-filled
    outputs; `check` requires every band intact and every read-only input unchanged"""

    def __init__(self, shift=0):
        self.shift, self.all, self.read_only = shift, [], []

    def ro(self, a, shift=None, **kw):
        g = guarded(a, shift=self.shift if shift is None else shift, **kw)
        self.all.append(g)
        self.read_only.append(g)
        return g

    def rw(self, a, shift=None, **kw):
        g = guarded(a, shift=self.shift if shift is None else shift, **kw)
        self.all.append(g)
        return g

    def out(self, shape, shift=None, **kw):
        return self.rw(tuple(shape), shift, **kw)

    def done(self):
        """a call that returns its result to the host has returned (the late provider of tests/_on_stream.py starts the
        next call behind a new delay; here there is nothing to do)"""

    def check(self, what):
        for k, g in enumerate(self.all):
            g.check((what, "array", k), read_only=any(g is r for r in self.read_only))


def test_the_helper_on_the_device():
    """what tests/test_guarded.py proves on the CPU holds for a device allocation: the view starts where `shift` says, a stray
    element either side is found at its offset (written here through the allocation itself), the view's own elements are
    not the band"""
    for dtype, shape in ((np.float32, (3, 9, 11)), (np.uint16, (2, 5, 7)), (np.uint8, (1001,))):
        for k in (0, 1, 2, 3):
            g = guarded(shape, dtype=dtype, shift=k)
            assert g.view.is_cuda and g.view.data_ptr() % 16 == 4 * k and g.intact() == (True, None)
            first = (g.view.data_ptr() - g.buf.data_ptr()) // g.dtype.itemsize
            n = g.view.numel()
            g.view.copy_(torch.from_numpy(np.ones(shape, dtype)).cuda())
            assert g.intact()
            one = torch.from_numpy(np.ones(1, dtype)).cuda()
            g.buf[first + n:first + n + 1].copy_(one)
            assert g.intact() == (False, n)
            g.buf[first - 1:first].copy_(one)
            assert g.intact() == (False, -1)


# ================================================================================================ projector family
# make_pair order (nz, n, nu, na, cor, os): every extent odd; nz % 4 != 0 with subsets of 8 / 7 / 7 angles; one whole
# 16-plane brick plus one ragged plane with n % 32 == 0; a single slice
GEOMS = [(5, 37, 45, 19, 1.25, 1), (6, 36, 40, 22, 0.5, 3), (17, 64, 71, 13, 0.0, 1), (1, 33, 33, 9, "vec", 2)]
_gid = lambda g: "-".join(map(str, g))  # noqa: E731


def _pair(oracle, g):
    """(the oracle's projector, the matched oracle, the HIP object) of a geometry, as tests/test_gpu_parity.py builds them"""
    import _matched_bp_oracle as M
    from test_gpu_parity import make_pair
    P, H = make_pair(oracle, g)
    nz, n, nu, na, cor, os_n = g
    # the angles and the per-angle CoR vector of make_pair
    PM = M.MatchedProjector(nz, n, nu, np.linspace(0.1, np.pi + 0.1, na, endpoint=False),
                            np.linspace(-1.5, 2.0, na) if isinstance(cor, str) else cor, os_n)
    return P, PM, H


def _subsets(P):
    return [None] if P.os_number == 1 else list(range(P.os_number))


def _idx(P, s):
    return slice(None) if s is None else P.subsets[s]


def _nsel(P, s):
    return P.na if s is None else len(P.subsets[s])


@pytest.mark.parametrize("g", GEOMS, ids=_gid)
def test_projector_pair_and_matched_adjoint(oracle, g):
    """tomo_fp3d, tomo_bp3d, tomo_bp3d_matched: bit for bit against the oracles of tests/test_gpu_parity.py and
    tests/test_gpu_matched_bp.py, every subset"""
    case_projector_pair_and_matched_adjoint(Arrays, oracle, g)


def case_projector_pair_and_matched_adjoint(mk, oracle, g):
    P, PM, H = _pair(oracle, g)
    rng = np.random.default_rng(2)
    vol = rng.standard_normal((P.nz, P.n, P.n)).astype(np.float32)
    for s in _subsets(P):
        A = (mk or Arrays)()
        v, sino_out = A.ro(vol), A.out(H.sino_shape(s))
        assert H.forward(v.view, s, out=sino_out.view) is sino_out.view
        same_bits(sino_out.host(), P.fp(vol, s), (g, s, "fp"))
        sino = rng.standard_normal((P.nz, _nsel(P, s), P.nu)).astype(np.float32)
        sd, vol_out, vol_m = A.ro(sino), A.out(H.vol_shape()), A.out(H.vol_shape())
        H.backward(sd.view, s, out=vol_out.view)
        assert not H.kernel_path("bp").startswith("matched")
        same_bits(vol_out.host(), P.bp(sino, s), (g, s, "bp"))
        H.backward(sd.view, s, out=vol_m.view, adjoint="matched")
        assert H.kernel_path("bp").startswith("matched")
        same_bits(vol_m.host(), PM.bp(sino, s), (g, s, "matched bp"))
        A.check((g, s))


def _planar_of_quad(q, nz):
    """[ceil(nz/4)][na][nu][4] -> ([nz][na][nu], the slices past nz)"""
    nq, na, nu, _ = q.shape
    flat = q.transpose(0, 3, 1, 2).reshape(4 * nq, na, nu)
    return np.ascontiguousarray(flat[:nz]), flat[nz:]


@pytest.mark.parametrize("layout", ["planar", "zquad"])
@pytest.mark.parametrize("g", GEOMS, ids=_gid)
def test_fused_residuals(oracle, g, layout):
    """tomo_fp3d_residual (LS / PWLS / KL) and tomo_fp3d_residual_robust in both residual layouts, the residual buffer of
    exactly tomo_ctx_residual_elems floats; tomo_fp3d_residual_ring (planar only: it refuses the quad layout).  Expected values
    as tests/test_gpu_parity.py::test_fused_residual_and_gradient_steps and tests/test_robust_terms.py form them."""
    case_fused_residuals(Arrays, oracle, g, layout)


def case_fused_residuals(mk, oracle, g, layout):
    from _cpu_backend import OracleTools3D
    P, _, H = _pair(oracle, g)
    rng = np.random.default_rng(3)
    b = (rng.random((P.nz, P.na, P.nu)) * 30).astype(np.float32)
    w = oracle.pwls_weights(b)
    x = rng.random((P.nz, P.n, P.n)).astype(np.float32)
    rx = rng.standard_normal((P.nz, P.nu)).astype(np.float32)
    H.set_residual_layout(layout)
    try:
        assert H.residual_layout() == layout
        for s in _subsets(P):
            idx, na_s = _idx(P, s), _nsel(P, s)
            ax = P.fp(x, s)
            elems = int(lib().tomo_ctx_residual_elems(H._ctx, H._sub(s)))
            shape = H.sino_shape(s) if layout == "planar" else (-(-P.nz // 4), na_s, P.nu, 4)
            assert int(np.prod(shape)) == elems
            ns = types.SimpleNamespace(_fp=lambda v, sub: ax, _sub=lambda os_index: os_index, _idx=lambda os_index: idx)

            def stated(fid):      # the residual as tests/_cpu_backend.py states it
                t = torch.empty(H.sino_shape(s), dtype=torch.float32)
                OracleTools3D.residual(ns, x, b, w if fid == "PWLS" else None, fid, s, t)
                return t.numpy()

            raw = stated("PWLS")
            wants = [("LS", None, stated("LS")), ("PWLS", None, raw), ("KL", None, stated("KL")),
                     ("PWLS", ("huber", 3.0), oracle.robust_weight(raw, huber=3.0)),
                     ("PWLS", ("studentst", 2.0), oracle.robust_weight(raw, studentst=2.0))]
            A = (mk or Arrays)()
            xd, bd, wd = A.ro(x), A.ro(b), A.ro(w)
            for fid, robust, want in wants:
                res = A.out(shape, planes=4 * na_s * P.nu)
                H.residual(xd.view, bd.view, wd.view if fid == "PWLS" else None, fid, s, res.view, robust=robust)
                got = res.host()
                if layout == "zquad":
                    got, tail = _planar_of_quad(got, P.nz)
                    assert not np.any(tail) and not np.isnan(tail).any(), "slices past the end of the volume must be written as zeros"
                same_bits(got, want.astype(np.float32), (g, s, layout, fid, robust))
            if layout == "planar":
                want = torch.empty(H.sino_shape(s), dtype=torch.float32)
                OracleTools3D.residual_ring(ns, x, b, rx, 4.0, s, want)
                res, rd = A.out(shape), A.ro(rx)
                H.residual_ring(xd.view, bd.view, rd.view, 4.0, s, res.view)
                same_bits(res.host(), want.numpy(), (g, s, "ring"))
            A.check((g, s, layout))
    finally:
        H.set_residual_layout("planar")


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "shift1"])
@pytest.mark.parametrize("adjoint", ["unmatched", "matched"])
@pytest.mark.parametrize("g", GEOMS, ids=_gid)
def test_fused_epilogues_of_both_adjoints(oracle, g, adjoint, shift):
    """tomo_bp3d[_matched]_fista / _fista_momentum / _admm with every volume array at `shift`: the oracle's gradient pushed
    through the one restatement of tests/test_gpu_bp_epilogues.py, array_equal"""
    case_fused_epilogues_of_both_adjoints(Arrays, oracle, g, adjoint, shift)


def case_fused_epilogues_of_both_adjoints(mk, oracle, g, adjoint, shift):
    import test_gpu_bp_epilogues as EP
    P, PM, H = _pair(oracle, g)
    H.adjoint = adjoint
    rng = np.random.default_rng(21)
    vshape = (P.nz, P.n, P.n)
    x, xo, u = (rng.standard_normal(vshape).astype(np.float32) * F32(k) for k in (0.05, 0.05, 0.01))
    for s in _subsets(P):
        r = rng.standard_normal((P.nz, _nsel(P, s), P.nu)).astype(np.float32)
        grad = (PM if adjoint == "matched" else P).bp(r, s)
        A = (mk or Arrays)(shift)
        rd = A.ro(r, shift=0)
        for nonneg in (False, True):
            (X,) = EP.restate("fista", grad, x, nonneg=nonneg)
            xt, out = A.ro(x), A.out(vshape)
            H.grad_step(rd.view, xt.view, out.view, EP.LINV, nonneg, s)
            assert H.kernel_path("bp").startswith("matched") == (adjoint == "matched")
            assert np.array_equal(out.host(), X), (g, s, "fista", nonneg)
            X, Xt = EP.restate("fista_mom", grad, x, xo, nonneg=nonneg)
            xt, xold = A.rw(x), A.rw(xo)
            H.grad_step_momentum(rd.view, xt.view, xold.view, EP.LINV, EP.BETA, nonneg, s)
            assert np.array_equal(xold.host(), X) and np.array_equal(xt.host(), Xt), (g, s, "fista_momentum", nonneg)
            relax_on = nonneg
            Z, ZU = EP.restate("admm", grad, x, u, xo, nonneg=nonneg, relax_on=relax_on)
            z, xd, ud, zu = A.rw(x), A.ro(xo), A.ro(u), A.out(vshape)
            H.admm_z_update(rd.view, z.view, xd.view, ud.view, zu.view, EP.TAU, EP.RHO, relax_on, EP.OMA, EP.ALPHA, nonneg, s)
            assert np.array_equal(z.host(), Z) and np.array_equal(zu.host(), ZU), (g, s, "admm", nonneg)
        A.check((g, adjoint, shift, s))


def test_volume_zquad_producers(oracle):
    """tomo_volume_to_zquad and tomo_momentum_transposed (both layouts) on the 64-wide geometry, X_t of exactly
    tomo_ctx_volume_elems floats; expected as tests/test_gpu_volume_zquad.py forms it"""
    case_volume_zquad_producers(Arrays, oracle)


def case_volume_zquad_producers(mk, oracle, pair=None):
    from test_gpu_volume_zquad import _relay
    g = GEOMS[2]
    P, _, H = pair or _pair(oracle, g)      # (a context's transposed-volume scratch grows, once, with the first quad-interleaved call)
    rng = np.random.default_rng(22)
    vshape = (P.nz, P.n, P.n)
    x, xold = (rng.standard_normal(vshape).astype(np.float32) for _ in range(2))
    beta = F32(0.7391357421875)
    want = x + beta * (x - xold)
    A = (mk or Arrays)()
    xd, xo = A.ro(x), A.ro(xold)
    try:
        assert int(lib().tomo_ctx_volume_elems(H._ctx)) == int(np.prod(vshape))
        xt = A.out(vshape)
        H.momentum(xd.view, xo.view, xt.view, beta)
        same_bits(xt.host(), want, "momentum, planar")
        H.invalidate()
        H.set_volume_layout("zquad", require_ok=False)
        qshape = (-(-P.nz // 4), P.n, P.n, 4)
        assert int(lib().tomo_ctx_volume_elems(H._ctx)) == int(np.prod(qshape))
        xq = A.out(qshape, planes=4 * P.n * P.n)
        H.momentum(xd.view, xo.view, xq.view, beta)
        same_bits(xq.host(), _relay(torch.from_numpy(want)).numpy(), "momentum, zquad")
        H.invalidate()
        conv = A.out(qshape, planes=4 * P.n * P.n)
        assert H.volume_to_zquad(xd.view, out=conv.view) is conv.view
        same_bits(conv.host(), _relay(torch.from_numpy(x)).numpy(), "volume_to_zquad")
        H.invalidate()
        A.check(g)
    finally:
        H.set_volume_layout("planar")


# ================================================================================================ other volume operators
def test_slicewise_tv(oracle, pd_arith):
    """tomo_pdtv_slices / tomo_roftv_slices on an all-odd stack and the smallest stack of tests/_slicewise_cases.py (a slice-wise
    operator has no 2D input), against the oracle per slice as tests/test_gpu_slicewise.py compares them"""
    case_slicewise_tv(Arrays, oracle, pd_arith)


def case_slicewise_tv(mk, oracle, pd_arith):
    import _slicewise_cases as S
    from test_gpu_slicewise import pd, rof
    for shape, iters in (((3, 9, 59), 7), ((2, 2, 2), 7)):
        assert (shape, iters) in S.PD_CASES and (shape, iters) in S.ROF_CASES
        vol = S.volume(shape)
        for half in (False, True):
            A = (mk or Arrays)()
            x, out = A.ro(vol), A.out(shape)
            kw = S.rof_kwargs(iters, half)
            rof(x.view, slicewise=True, out=out.view, **kw)
            got = out.host()
            assert got.shape == shape and np.array_equal(got, S.oracle_slices("ROF_TV", vol, **kw)), (shape, half, "ROF_TV")
            out = A.out(shape)
            kw = S.pd_kwargs(iters, half=half)
            pd(x.view, slicewise=True, out=out.view, **kw)
            pd_arith.check(out.host(), S.oracle_slices("PD_TV", vol, **kw), half=half, what=f"guarded slicewise PD_TV {shape}")
            A.check((shape, half))


@pytest.mark.parametrize("shape", [(13, 37), (7, 13, 37)], ids=lambda s: "x".join(map(str, s)))
def test_wavelets(shape):
    """tomo_wavelet_shrink / _forward / _inverse, the pyramid of exactly wavelet_pyramid_floats floats (tomo_wavelet_forward and
    tomo_wavelet_inverse through the C entry: the wrapper of the first allocates its own pyramid)"""
    case_wavelets(Arrays, shape)


def case_wavelets(mk, shape):
    from test_gpu_wavelets import mix_of, want
    from _tgv_oracle import phantom
    from tomobar_amd import ops
    f, t = phantom(shape), 0.02
    pyr_want, w = want(shape, t)
    m_host = mix_of(shape)
    dz, dy, dx = (1, *shape) if len(shape) == 2 else shape
    nd, plane = len(shape), shape[-1] * shape[-2]
    A = (mk or Arrays)()
    x, m, out, mixed = A.ro(f), A.ro(m_host), A.out(shape), A.out(shape)
    ops.wavelet_shrink(x.view, F32(t), out=out.view)
    same_bits(out.host(), w, (shape, "shrink"))
    ops.wavelet_shrink(x.view, F32(t), out=mixed.view, mix=m.view)
    same_bits(mixed.host(), (m_host + w) * F32(0.5), (shape, "shrink, mix"))
    nfl = ops.wavelet_pyramid_floats(shape)
    assert nfl == pyr_want.size
    pyr = A.out((nfl,), planes=plane)
    ok(lib().tomo_wavelet_forward(0, vp(x.view), vp(pyr.view), dx, dy, dz, nd, float(F32(t)), stream()))
    same_bits(pyr.host(), pyr_want, (shape, "pyramid"))
    given = A.rw(pyr_want, planes=plane)          # the inverse overwrites LL_1 and LL_2 of the pyramid it reads
    inv = A.out(shape)
    ops.wavelet_inverse(given.view, shape, out=inv.view)
    same_bits(inv.host(), w, (shape, "inverse"))
    A.check(shape)


@pytest.mark.parametrize("shape, params", [((13, 37), (7, 2, 15)), ((7, 13, 37), (3, 1, 8))], ids=lambda v: "x".join(map(str, v)))
def test_patch_select_and_nltv(shape, params):
    """tomo_patch_select (C entry: the wrapper allocates its tables) and tomo_nltv with the uint16 tables and the weights
    guarded, against tests/_nltv_oracle.py as tests/test_gpu_nltv.py compares them"""
    case_patch_select_and_nltv(Arrays, shape, params)


def case_patch_select_and_nltv(mk, shape, params):
    import test_gpu_nltv as TN
    from tomobar_amd import ops
    img, tables = TN.oracle_tables("noisy", shape, params)
    S_, P_, K = params
    dz, dy, dx = (1, *shape) if len(shape) == 2 else shape
    A = (mk or Arrays)()
    x = A.ro(np.array(img))
    hi, hj = (A.out((K, *shape), dtype=np.uint16, fill=0xFFFF) for _ in range(2))
    wt = A.out((K, *shape))
    ok(lib().tomo_patch_select(0, vp(x.view), vp(hi.view), vp(hj.view), vp(wt.view), dx, dy, dz, len(shape), S_, P_, K,
                               float(F32(TN.INPUTS["noisy"][1])), stream()))
    for name, got, want in (("H_i", hi, tables[0]), ("H_j", hj, tables[1])):
        assert got.host().dtype == np.uint16 and np.array_equal(got.host(), want), (shape, params, name)
    same_bits(wt.host(), tables[2], (shape, params, "Weights"))
    lam, n = 0.02, 2
    t = [A.ro(np.array(a)) for a in tables]
    out = A.out(shape)
    ops.nltv(x.view, out.view, *(g.view for g in t), F32(lam), n, 0.0)
    same_bits(out.host(), TN.oracle_iterates(shape, params, lam, TN.COUNTS)[n], (shape, params, "nltv"))
    A.check((shape, params))


# ================================================================================================ direct methods
@pytest.mark.parametrize("nu", [45, 64])
def test_fbp_filter_in_place(oracle, nu):
    """tomo_fbp_filter in place on 7 rows, at the bound of tests/test_fbp.py"""
    case_fbp_filter_in_place(Arrays, oracle, nu)


def case_fbp_filter_in_place(mk, oracle, nu):
    from test_fbp import rel
    rows, cutoff = 7, 0.6
    x = np.random.default_rng(3).random((rows, 1, nu)).astype(np.float32)
    A = (mk or Arrays)()
    d = A.rw(x)
    ok(lib().tomo_fbp_filter(0, vp(d.view), rows, nu, cutoff, 1.0 / rows / nu, stream()))
    want = oracle.fbp_filter(x, cutoff)
    assert np.isfinite(d.host()).all() and rel(d.host(), want) < 1e-5, (nu, rel(d.host(), want))
    A.check(nu)


def test_fourier_inv(monkeypatch):
    """tomo_fourier_inv at the smallest case of tests/test_fourier.py (even sizes: the driver hands its input straight to
    the entry point).  The driver prepares the arguments; the entry point runs first on the guarded input with a guarded
    output in place of the driver's own, and that output is held to the bounds of test_FOURIER_INV_vs_oracle_and_fixture."""
    case_fourier_inv(Arrays, monkeypatch)


def case_fourier_inv(mk, monkeypatch):
    import test_fourier as TF
    from oracle import fourier_oracle as FO
    golden = np.load(os.path.join(TF.HERE, "golden", "fourier_golden.npz"))
    case = min(TF.CASES, key=lambda c: golden[c[0] + "_sino"].size)
    name, nz, nproj, dn, rs, cor, span, kw = case
    assert nz % 2 == 0 and dn % 2 == 0 and "data_axes_labels_order" not in kw and "recon_mask_radius" not in kw
    A = (mk or Arrays)()
    src = A.ro(np.ascontiguousarray(golden[name + "_sino"], np.float32))
    real, outs = lib().tomo_fourier_inv, []

    def on_guarded(device, data_p, out_p, nz_even, out_z, nproj_, raw_n, n, ne, unpad_m, out_size, *rest):
        assert data_p.value == src.view.data_ptr() and (nz_even, nproj_, raw_n) == tuple(src.view.shape)
        dst = A.out((out_z, out_size, out_size))
        ok(real(device, data_p, vp(dst.view), nz_even, out_z, nproj_, raw_n, n, ne, unpad_m, out_size, *rest))
        outs.append(dst)
        return real(device, data_p, out_p, nz_even, out_z, nproj_, raw_n, n, ne, unpad_m, out_size, *rest)

    monkeypatch.setattr(lib(), "tomo_fourier_inv", on_guarded)
    rec = TF._tools(case, golden).FOURIER_INV(src.view, **kw).cpu().numpy()
    assert len(outs) == 1
    got, want = outs[0].host(), golden[name + "_rec"]
    assert got.shape == want.shape == rec.shape and np.isfinite(got).all()
    assert TF.rel(got, want) < TF.TOL, "vs the reference's own output"
    assert TF.rel(got, TF._oracle_run(FO, golden, case)) < TF.TOL, "vs the oracle"
    assert TF.rel(rec, want) < TF.TOL
    A.check(name)


# ================================================================================================ glue: element-wise
EW_N = (1, 3, 4, 5, 255, 1024, 1025, 4099)
BETA, AX, BY, LO, VALUE, WMAX = F32(0.731), F32(0.3), F32(-1.1), F32(-0.25), F32(2.75), F32(1.625)


def _recip_want(x):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = F32(1) / x
    return np.where(np.isnan(r) | np.isinf(r), F32(1), r).astype(np.float32)


def _special(x):
    """x with 0, inf and NaN in its first elements (recip_safe's branches)"""
    x = x.copy()
    x[:3] = np.array([0.0, np.inf, np.nan], np.float32)[:x.size]
    return x


# name -> (read-only inputs, the written array's initial content or None (pure output), call(lib, inputs, out, n), want);
# x, y, z are the three random arrays of a case.  Expected values: numpy float32 in the order of operations the functors
# of glue_kernels.hip state, bit for bit, as tests/test_gpu_parity.py::test_glue_kernels forms them
EW = {
    "momentum": (lambda x, y, z: (x, y), None, lambda L, i, o, n: L.tomo_momentum(vp(i[0]), vp(i[1]), vp(o), float(BETA), n, stream()),
                 lambda x, y, z: x + BETA * (x - y)),
    "admm_dual": (lambda x, y, z: (y, z), "x", lambda L, i, o, n: L.tomo_admm_dual(vp(o), vp(i[0]), vp(i[1]), n, stream()),
                  lambda x, y, z: x + (y - z)),
    "axpby": (lambda x, y, z: (x,), "y", lambda L, i, o, n: L.tomo_axpby(float(AX), vp(i[0]), float(BY), vp(o), n, stream()),
              lambda x, y, z: AX * x + BY * y),
    "scale": (lambda x, y, z: (x,), None, lambda L, i, o, n: L.tomo_scale(float(AX), vp(i[0]), vp(o), n, stream()),
              lambda x, y, z: AX * x),
    "clamp_min": (lambda x, y, z: (), "x", lambda L, i, o, n: L.tomo_clamp_min(vp(o), float(LO), n, stream()),
                  lambda x, y, z: np.where(x < LO, LO, x)),
    "mul": (lambda x, y, z: (x,), "y", lambda L, i, o, n: L.tomo_mul(vp(i[0]), vp(o), n, stream()),
            lambda x, y, z: x * y),
    "recip_safe": (lambda x, y, z: (_special(x),), None, lambda L, i, o, n: L.tomo_recip_safe(vp(i[0]), vp(o), n, stream()),
                   lambda x, y, z: _recip_want(_special(x))),
    "fill": (lambda x, y, z: (), None, lambda L, i, o, n: L.tomo_fill(vp(o), float(VALUE), n, stream()),
             lambda x, y, z: np.full(x.shape, VALUE, np.float32)),
    "pwls_weights": (lambda x, y, z: (x,), None, lambda L, i, o, n: L.tomo_pwls_weights(vp(i[0]), vp(o), n, stream()),
                     None),     # the oracle's pwls_weights, below
    "pwls_weights_scaled": (lambda x, y, z: (x,), None,
                            lambda L, i, o, n: L.tomo_pwls_weights_scaled(vp(i[0]), vp(o), n, float(WMAX), stream()),
                            lambda x, y, z: np.maximum(x, F32(1e-6)) / WMAX),
}


def _ew_case(oracle, name, n, in_shift, out_shift, seed=7, mk=None):
    ins_of, initial, call, want_of = EW[name]
    rng = np.random.default_rng(seed + n)
    x, y, z = (rng.standard_normal(n).astype(np.float32) for _ in range(3))
    want = oracle.pwls_weights(x) if want_of is None else want_of(x, y, z)
    assert want.dtype == np.float32
    A = (mk or Arrays)()
    ins = [A.ro(a, shift=in_shift) for a in ins_of(x, y, z)]
    out = A.out((n,), shift=out_shift) if initial is None else A.rw({"x": x, "y": y}[initial], shift=out_shift)
    ok(call(lib(), [g.view for g in ins], out.view, n))
    same_bits(out.host(), want, (name, n, in_shift, out_shift))
    A.check((name, n, in_shift, out_shift))


@pytest.mark.parametrize("name", list(EW))
def test_elementwise_entries(oracle, name):
    """every element-wise entry of glue_kernels.hip: all arrays aligned (float4 kernel with its scalar tail), all arrays one
    float off (scalar kernel), and at 4099 elements only the written array off (scalar kernel chosen by the output alone)"""
    for n in EW_N:
        _ew_case(oracle, name, n, 0, 0)
        _ew_case(oracle, name, n, 1, 1)
    _ew_case(oracle, name, 4099, 0, 1)


def _reductions(n, shift, what, mk=None):
    """tomo_norm2 / tomo_dot at the tolerances of test_glue_kernels; tomo_max / tomo_pwls_max exactly (the maximum of float32
    values is one of them: no rounding takes part)"""
    rng = np.random.default_rng(70 + n)
    x, y = (rng.standard_normal(n).astype(np.float32) for _ in range(2))
    A = (mk or Arrays)(shift)
    xd, yd = A.ro(x), A.ro(y)
    out, outf = C.c_double(0.0), C.c_float(0.0)
    ok(lib().tomo_norm2(vp(xd.view), n, C.byref(out), stream()))
    A.done()
    np.testing.assert_allclose(out.value, np.linalg.norm(x.astype(np.float64)), rtol=1e-12)
    ok(lib().tomo_dot(vp(xd.view), vp(yd.view), n, C.byref(out), stream()))
    A.done()
    np.testing.assert_allclose(out.value, np.dot(x.astype(np.float64), y.astype(np.float64)), rtol=1e-9, atol=1e-12)
    ok(lib().tomo_max(vp(xd.view), n, C.byref(outf), stream()))
    A.done()
    assert outf.value == float(x.max()), (what, n, shift, "max")
    ok(lib().tomo_pwls_max(vp(xd.view), n, C.byref(outf), stream()))
    A.done()
    assert outf.value == float(np.maximum(x, F32(1e-6)).max()), (what, n, shift, "pwls_max")
    small = A.ro(-np.abs(x))       # nothing above the clamp: the clamp itself is the maximum
    ok(lib().tomo_pwls_max(vp(small.view), n, C.byref(outf), stream()))
    A.done()
    assert outf.value == float(F32(1e-6))
    A.check((what, n, shift))


def test_reductions():
    for n in EW_N:
        for shift in (0, 1):
            _reductions(n, shift, "reductions")


def _rel_change(n, shifts, mode, x_h, r_h, want, mk=None):
    """one tomo_rel_change call at the bound of tests/test_gpu_tolerance.py::test_rel_change_kernel"""
    import _tolerance_cases as T
    from tomobar_amd import ops
    sx, sr, sk = shifts
    A = (mk or Arrays)()
    x, ref = A.ro(x_h, shift=sx), A.rw(r_h, shift=sr)
    keep = A.out((n,), shift=sk) if mode == "separate" else None
    got = ops.rel_change(x.view, ref.view, None if mode == "absent" else (ref.view if mode == "aliasing" else keep.view))
    for g, w in zip(got, want):
        assert abs(g - w) <= n * T.EPS53 * w, (n, shifts, mode, g, w)
    same_bits(ref.host(), x_h if mode == "aliasing" else r_h, (n, shifts, mode, "ref"))
    if keep is not None:
        same_bits(keep.host(), x_h, (n, shifts, mode, "keep"))
    A.check((n, shifts, mode))


def _rel_change_inputs(n):
    from test_gpu_tolerance import _exact_sums
    rng = np.random.default_rng(n)
    x_h = rng.standard_normal(n).astype(np.float32)
    r_h = (x_h + 0.1 * rng.standard_normal(n)).astype(np.float32)
    return x_h, r_h, _exact_sums(x_h, r_h)


def test_rel_change():
    """keep absent / aliasing ref / separate; the float4 kernel with 0..3 leading elements (all pointers shifted alike) and
    the scalar kernel (pointers shifted differently)"""
    for n in EW_N:
        x_h, r_h, want = _rel_change_inputs(n)
        for mode in ("absent", "aliasing", "separate"):
            for k in (0, 1, 2, 3):
                _rel_change(n, (k, k, k), mode, x_h, r_h, want)
            _rel_change(n, (0, 1, 2), mode, x_h, r_h, want)


# ================================================================================================ glue: pre / post
def test_pad_crop_mask_permute(oracle):
    """the four pre / post kernels at the shapes of tests/test_gpu_parity.py::test_pad_crop_mask_permute, outputs passed in"""
    case_pad_crop_mask_permute(Arrays, oracle)


def case_pad_crop_mask_permute(mk, oracle):
    rng = np.random.default_rng(8)
    A = (mk or Arrays)()
    b = rng.random((3, 7, 10)).astype(np.float32)
    bd, out = A.ro(b), A.out((3, 7, 18))
    ok(lib().tomo_pad_edge(vp(bd.view), vp(out.view), 3 * 7, 10, 4, stream()))
    same_bits(out.host(), oracle.pad_detector(b, 4), "pad_edge")
    v = rng.standard_normal((3, 21, 21)).astype(np.float32)
    vd, out = A.ro(v), A.out((3, 12, 12))
    ok(lib().tomo_crop_center(vp(vd.view), vp(out.view), 3, 21, 12, stream()))
    same_bits(out.host(), oracle.crop_recon(v, 12), "crop_center")
    for n in (20, 21):
        v = rng.standard_normal((2, n, n)).astype(np.float32)
        for radius in (0.85, 1.0, 0.5, 2.0):
            m = A.rw(v)
            ok(lib().tomo_circ_mask(vp(m.view), 2, n, float(radius), stream()))
            same_bits(m.host(), oracle.circular_mask(v, radius).astype(np.float32), ("circ_mask", n, radius))
    t = rng.random((4, 5, 6)).astype(np.float32)
    td = A.ro(t)
    for perm in ((1, 0, 2), (2, 1, 0), (0, 2, 1), (2, 0, 1)):
        p = td.view.permute(*perm)
        out = A.out(tuple(p.shape))
        ok(lib().tomo_permute3(vp(td.view), vp(out.view), *p.shape, *p.stride(), stream()))
        same_bits(out.host(), np.ascontiguousarray(t.transpose(perm)), ("permute3", perm))
    A.check("pad / crop / mask / permute")


# ================================================================================================ glue: sinogram terms
NZ, NA_S, NU, NA_FULL = 3, 7, 45, 19
SRC = np.array([0, 3, 6, 9, 12, 15, 18], np.int32)      # the subset's rows of the full angle axis; the last one is the last


def _sino_terms_inputs():
    rng = np.random.default_rng(31)
    res = rng.standard_normal((NZ, NA_S, NU)).astype(np.float32)
    full = (rng.random((NZ, NA_FULL, NU)) * 30).astype(np.float32)
    wfull = rng.random((NZ, NA_FULL, NU)).astype(np.float32)
    ring = rng.standard_normal((NZ, NU)).astype(np.float32)
    return res, full, wfull, ring


def _seam(**kw):
    """the attributes tests/_cpu_backend.OracleTools3D's methods read, for a residual that is already projected"""
    return types.SimpleNamespace(nz=NZ, nu=NU, _fp=lambda v, sub: v, _sub=lambda os_index: os_index, _idx=lambda os_index: SRC, **kw)


def test_shift_rows_residual_ring_robust(oracle):
    """tomo_shift_rows, tomo_sino_residual, tomo_sino_add_ring, tomo_sino_robust against the formulas the oracle and the CPU
    stand-in of the projector (tests/_cpu_backend.py) state, bit for bit as the driver tests hold them"""
    case_shift_rows_residual_ring_robust(Arrays, oracle)


def case_shift_rows_residual_ring_robust(mk, oracle):
    from _cpu_backend import OracleTools3D
    from tomobar_amd import _lib as L
    res, full, wfull, ring = _sino_terms_inputs()
    A = (mk or Arrays)()
    src = A.ro(SRC)
    # shift_rows, both signs: integer, fractional, negative shifts and one that leaves the detector
    shift = np.array([0.0, 1.0, 0.25, -0.75, 2.5, -3.5, 0.999], np.float32)
    ns = types.SimpleNamespace(nz=NZ, na=NA_S, vshift=shift, subsets=None)
    rd, sd = A.ro(res), A.ro(shift)
    for sign in (1.0, -1.0):
        out = A.out(res.shape)
        ok(lib().tomo_shift_rows(vp(rd.view), vp(out.view), NZ, NA_S, NU, vp(sd.view), sign, stream()))
        same_bits(out.host(), oracle.Projector.shift_rows(ns, res, None, sign), ("shift_rows", sign))
    # sino_residual on an already projected subset
    ax = np.abs(res) * F32(20)
    axd, bd, wd = A.ro(ax), A.ro(full), A.ro(wfull)
    for fid in ("LS", "PWLS", "KL"):
        want = torch.empty(res.shape, dtype=torch.float32)
        OracleTools3D.residual(_seam(), ax, full, wfull if fid == "PWLS" else None, fid, 0, want)
        out = A.out(res.shape)
        ok(lib().tomo_sino_residual(vp(axd.view), vp(bd.view), vp(wd.view) if fid == "PWLS" else None, vp(src.view), NZ, NA_S,
                                    NA_FULL, NU, 0, L.FID[fid], vp(out.view), stream()))
        same_bits(out.host(), want.numpy(), ("sino_residual", fid))
    # ... and with b and w already gathered
    want = torch.empty(res.shape, dtype=torch.float32)
    OracleTools3D.residual(_seam(), ax, full, wfull, "PWLS", 0, want)
    gb, gw, out = A.ro(full[:, SRC]), A.ro(wfull[:, SRC]), A.out(res.shape)
    ok(lib().tomo_sino_residual(vp(axd.view), vp(gb.view), vp(gw.view), vp(src.view), NZ, NA_S, NA_FULL, NU, 3, L.FID["PWLS"],
                                vp(out.view), stream()))
    same_bits(out.host(), want.numpy(), "sino_residual, gathered")
    # sino_add_ring: the ring residual with nothing subtracted
    want = torch.empty(res.shape, dtype=torch.float32)
    OracleTools3D.residual_ring(_seam(), res, np.zeros_like(full), ring, 4.0, 0, want)
    io, gd = A.rw(res), A.ro(ring)
    ok(lib().tomo_sino_add_ring(vp(io.view), vp(gd.view), 4.0, NZ, NA_S, NU, stream()))
    same_bits(io.host(), want.numpy(), "sino_add_ring")
    # sino_robust in place
    raw = res * F32(4)
    for mode, delta in (("huber", 3.0), ("studentst", 2.0)):
        io = A.rw(raw)
        ok(lib().tomo_sino_robust(vp(io.view), raw.size, L.ROBUST[mode], delta, stream()))
        same_bits(io.host(), oracle.robust_weight(raw, **{mode: delta}), ("sino_robust", mode))
    assert src.view.dtype == torch.int32
    A.check("sinogram terms")


def test_ring_terms():
    """tomo_ring_gh_reduce (with and without PWLS weights), tomo_ring_gh_update, tomo_swls_apply at (nz, na_s, nu) = (3, 7, 45)
    with an index table into 19 angles, against the formulas of tests/_cpu_backend.py"""
    case_ring_terms(Arrays)


def case_ring_terms(mk):
    from _cpu_backend import OracleTools3D
    res, full, wfull, ring = _sino_terms_inputs()
    l_inv, lam, beta = F32(1 / 300.0), F32(0.3), F32(0.37)
    A = (mk or Arrays)()
    src, wd, rx = A.ro(SRC), A.ro(wfull), A.ro(ring)
    for weights in (None, wfull):
        want_res, want_r = torch.from_numpy(res.copy()), torch.empty((NZ, NU), dtype=torch.float32)
        OracleTools3D.ring_reduce(_seam(), want_res, weights, ring, l_inv, 0, want_r)
        io, r_out = A.rw(res), A.out((NZ, NU))
        ok(lib().tomo_ring_gh_reduce(vp(io.view), None if weights is None else vp(wd.view), vp(src.view), NZ, NA_S, NA_FULL, NU,
                                     vp(rx.view), float(l_inv), vp(r_out.view), stream()))
        same_bits(r_out.host(), want_r.numpy(), ("ring_gh_reduce", weights is not None, "r"))
        same_bits(io.host(), want_res.numpy(), ("ring_gh_reduce", weights is not None, "res"))
    r_old = np.random.default_rng(32).standard_normal((NZ, NU)).astype(np.float32)
    w_r, w_old, w_x = torch.from_numpy(ring.copy()), torch.from_numpy(r_old.copy()), torch.empty((NZ, NU), dtype=torch.float32)
    OracleTools3D.ring_update(None, w_r, w_old, w_x, lam, beta)
    r, ro, x = A.rw(ring), A.rw(r_old), A.out((NZ, NU))
    ok(lib().tomo_ring_gh_update(vp(r.view), vp(ro.view), vp(x.view), float(lam), float(beta), NZ * NU, stream()))
    for name, got, want in (("r", r, w_r), ("r_old", ro, w_old), ("r_x", x, w_x)):
        same_bits(got.host(), want.numpy(), ("ring_gh_update", name))
    want_res = torch.from_numpy(res.copy())
    OracleTools3D.swls_apply(_seam(), want_res, wfull, 0.1, 0)
    io = A.rw(res)
    ok(lib().tomo_swls_apply(vp(io.view), vp(wd.view), vp(src.view), NZ, NA_S, NA_FULL, NU, 0.1, stream()))
    same_bits(io.host(), want_res.numpy(), "swls_apply")
    A.check("ring terms")


# ================================================================================================ glue: halo staging
def _ptr_table(tensors):
    return (C.c_void_p * max(len(tensors), 1))(*[t.data_ptr() for t in tensors])


def _size_table(nbytes):
    return (C.c_size_t * max(len(nbytes), 1))(*nbytes)


def test_halo_staging():
    """tomo_halo_pack / _unpack / _pack2 / _pull2 with the blocks of tests/test_gpu_slab.py::test_halo_pack_unpack_round_trip
    (odd byte counts, starts that are not 4-byte aligned), every block a slice of a guarded byte buffer and the staging
    buffer of exactly tomo_halo_staging_bytes bytes"""
    case_halo_staging(Arrays)


def case_halo_staging(mk):
    from tomobar_amd.slab import _halo_staging_bytes
    rng = np.random.default_rng(3)
    u = rng.random((7, 13, 37)).astype(np.float32).view(np.uint8).ravel()                  # 1924 B per plane
    p = rng.random((7, 13, 37)).astype(np.float16).view(np.uint8).ravel()                  # 962 B per plane
    b = rng.integers(0, 255, 1001).astype(np.uint8)
    cuts = [(u, 4 * 1924, 7 * 1924), (p, 4 * 962, 7 * 962), (p, 962, 2 * 962), (b, 3, 1000), (u, 0, 1924)]
    nbytes = [hi - lo for _, lo, hi in cuts]
    total = _halo_staging_bytes(nbytes)
    assert lib().tomo_halo_staging_bytes(_size_table(nbytes), len(nbytes)) == total
    image = np.full(total, 0xAB, np.uint8)          # what the staging buffer must hold: the padding between blocks untouched
    off = 0
    for (a, lo, hi), nb in zip(cuts, nbytes):
        image[off:off + nb] = a[lo:hi]
        off += (nb + 15) // 16 * 16
    A = (mk or Arrays)()
    srcs = {id(a): A.ro(a) for a in (u, p, b)}
    blocks = [srcs[id(a)].view[lo:hi] for a, lo, hi in cuts]
    assert any(t.data_ptr() % 4 for t in blocks) and any(nb % 2 for nb in nbytes)
    stage = A.out((total,), dtype=np.uint8, fill=0xAB)
    ok(lib().tomo_halo_pack(_ptr_table(blocks), _size_table(nbytes), len(blocks), vp(stage.view), stream()))
    assert np.array_equal(stage.host(), image)
    # unpack into NaN-free byte buffers of the sources' sizes: only the blocks' bytes change
    dsts = {id(a): A.out((a.size,), dtype=np.uint8, fill=0x11) for a in (u, p, b)}
    outs = [dsts[id(a)].view[lo:hi] for a, lo, hi in cuts]
    ok(lib().tomo_halo_unpack(vp(stage.view), _ptr_table(outs), _size_table(nbytes), len(outs), stream()))
    for a in (u, p, b):
        want = np.full(a.size, 0x11, np.uint8)
        for c, lo, hi in cuts:
            if c is a:
                want[lo:hi] = a[lo:hi]
        assert np.array_equal(dsts[id(a)].host(), want)
    # both directions in one launch: blocks 0..2 down, 3..4 up; then an empty direction
    down, up = slice(0, 3), slice(3, 5)
    tot_d, tot_u = _halo_staging_bytes(nbytes[down]), _halo_staging_bytes(nbytes[up])
    msg_d, msg_u = A.out((tot_d,), dtype=np.uint8, fill=0xAB), A.out((tot_u,), dtype=np.uint8, fill=0xAB)
    ok(lib().tomo_halo_pack2(_ptr_table(blocks[down]), _size_table(nbytes[down]), 3, vp(msg_d.view),
                             _ptr_table(blocks[up]), _size_table(nbytes[up]), 2, vp(msg_u.view), stream()))
    assert np.array_equal(msg_d.host(), image[:tot_d])
    img_u, off = np.full(tot_u, 0xAB, np.uint8), 0
    for (a, lo, hi), nb in zip(cuts[up], nbytes[up]):
        img_u[off:off + nb] = a[lo:hi]
        off += (nb + 15) // 16 * 16
    assert np.array_equal(msg_u.host(), img_u)
    dsts2 = {id(a): A.out((a.size,), dtype=np.uint8, fill=0x11) for a in (u, p, b)}
    outs2 = [dsts2[id(a)].view[lo:hi] for a, lo, hi in cuts]
    ok(lib().tomo_halo_pull2(vp(msg_d.view), _ptr_table(outs2[down]), _size_table(nbytes[down]), 3,
                             vp(msg_u.view), _ptr_table(outs2[up]), _size_table(nbytes[up]), 2, stream()))
    for a in (u, p, b):
        assert np.array_equal(dsts2[id(a)].host(), dsts[id(a)].host())
    ok(lib().tomo_halo_pack2(_ptr_table([]), _size_table([]), 0, None,
                             _ptr_table(blocks[up]), _size_table(nbytes[up]), 2, vp(msg_u.view), stream()))
    assert np.array_equal(msg_u.host(), img_u)
    A.check("halo staging")


# ================================================================================================ past one grid of threads
# glue_kernels.hip (EW_MAX_GRID) and pdhg_kernels.hip (STREAM_MAX_GRID) cap a launch at 256 * 8 blocks of 256 threads; a
# thread of the float4 kernels takes 4 elements per trip, a thread of the scalar kernels 1.  One element more than a whole grid
# covers starts the second trip of the grid-stride loop
MAX_GRID, BLOCK = 256 * 8, 256
N_VEC4 = MAX_GRID * BLOCK * 4 + 5        # second trip of one float4 and a 1-element scalar tail
N_SCALAR = MAX_GRID * BLOCK + 1          # second trip of one element
GRID_STRIDE = [pytest.param(N_VEC4, 0, id="vec4"), pytest.param(N_SCALAR, 1, id="scalar")]


def test_grid_sizes_are_what_the_sources_say():
    assert (N_VEC4, N_SCALAR) == (2097157, 524289)
    for fname, text in (("glue_kernels.hip", "constexpr int EW_MAX_GRID = 256 * 8;"), ("glue_kernels.hip", "constexpr int EW_BLOCK = 256;"),
                        ("pdhg_kernels.hip", "constexpr int STREAM_MAX_GRID = 256 * 8;"), ("pdhg_kernels.hip", "constexpr int STREAM_BLOCK = 256;")):
        with open(os.path.join(ROOT, "tomobar_amd", "csrc", fname)) as fh:
            assert text in fh.read(), (fname, text)


@pytest.mark.parametrize("n, shift", GRID_STRIDE)
def test_grid_stride_elementwise_and_rel_change(oracle, n, shift):
    for name in ("momentum", "axpby"):
        _ew_case(oracle, name, n, shift, shift)
    # rel_change takes 16-byte accesses whenever its pointers are shifted alike (three leading elements at shift 1): its
    # scalar kernel needs pointers shifted differently
    x_h, r_h, want = _rel_change_inputs(n)
    for shifts in [(shift, shift, shift)] + ([(1, 2, 3)] if shift else []):
        _rel_change(n, shifts, "separate", x_h, r_h, want)
        _rel_change(n, shifts, "aliasing", x_h, r_h, want)


@pytest.mark.parametrize("n, shift", GRID_STRIDE)
def test_grid_stride_stream_kernels(n, shift):
    """pdhg_sino_dual, spdhg_sino_dual, spdhg_primal (stream3_kernel) against tests/_pdhg_oracle.py / tests/_spdhg_oracle.py,
    bit for bit as tests/test_gpu_pdhg.py and tests/test_gpu_spdhg.py hold them"""
    case_stream_kernels(Arrays, n, shift)


def case_stream_kernels(mk, n, shift):
    import _pdhg_oracle as P
    import _spdhg_oracle as S
    from test_gpu_pdhg import _sino_inputs
    from test_gpu_spdhg import _primal_inputs
    from tomobar_amd import ops
    y, r, b = _sino_inputs((n,))
    sigma = F32(0.4)
    for fidelity in P.FIDELITIES:
        A = mk(shift)
        yd, rd, bd = A.rw(y), A.ro(r), A.ro(b)
        ops.pdhg_sino_dual(yd.view, rd.view, bd.view, fidelity, sigma)
        same_bits(yd.host(), P.sino_dual(y, r, b, fidelity, sigma), ("pdhg_sino_dual", n, fidelity))
        yd, rd = A.rw(y), A.rw(r)
        ops.spdhg_sino_dual(yd.view, rd.view, bd.view, fidelity, sigma)
        want_y, want_d = S.sino_step(y, r, b, fidelity, sigma)
        same_bits(yd.host(), want_y, ("spdhg_sino_dual", n, fidelity, "y"))
        same_bits(rd.host(), want_d, ("spdhg_sino_dual", n, fidelity, "d"))
        A.check((n, fidelity))
    x, z, delta = _primal_inputs((n,))
    tau, w = F32(0.05), F32(4.0)
    for nonneg in (0, 1):
        A = mk(shift)
        xd, zd, dd = A.rw(x), A.rw(z), A.ro(delta)
        ops.spdhg_primal(xd.view, zd.view, dd.view, tau, w, nonneg)
        want_x, want_z = S.primal_step(x, z, delta, tau, w, nonneg)
        same_bits(xd.host(), want_x, ("spdhg_primal", n, nonneg, "x"))
        same_bits(zd.host(), want_z, ("spdhg_primal", n, nonneg, "z"))
        A.check((n, "primal", nonneg))


def test_grid_stride_reductions():
    """reduce_kernel is scalar whatever the alignment: its second trip starts at N_SCALAR"""
    _reductions(N_SCALAR, 1, "grid-stride")
