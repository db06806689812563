"""Every kernel on an array that crosses 2^29, 2^30, 2^31 (or 2^32) elements, held to its oracle plane by plane through the
periodic-volume check of tests/_large_index.py, whose premises tests/test_large_index.py proves on the CPU.  One operator
per test id; every id frees its arrays and the library's scratch, and skips only when the device has less free memory than
its footprint plus 10 %."""
import ctypes as C
import gc
import math

import numpy as np
import pytest

import _large_index as LI

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _empty_device():
    """every id starts from an empty device: the caching allocator's blocks and the library's scratch arenas are released
    afterwards; one allocation per arena (the placement search holds several candidates at once and takes seconds)"""
    from tomobar_amd import _lib, ops
    tries = ops.placement_tries()
    ops.set_placement_tries(1)
    try:
        yield
    finally:
        torch.cuda.synchronize()
        gc.collect()
        torch.cuda.empty_cache()
        _lib.check(_lib.lib().tomo_release_scratch(0))
        ops.set_placement_tries(tries)


def need(footprint):
    free, _ = torch.cuda.mem_get_info()
    if free < 1.1 * footprint:
        pytest.skip(f"{free} bytes are free on the device, the footprint of {footprint} bytes plus 10 % is needed")


def run_volume_op(op, nd, pd_arith=None):
    shape = LI.op_shape(op, nd)
    need(LI.footprint(op.foot[0], shape, op.foot[1]))
    compare = LI.same_bits
    if op.pd:
        def compare(got, want, what):
            pd_arith.check(got, want, half=op.half, what=str(what))
    LI.periodic(op.gpu, op.oracle, op.bases((LI.PERIOD,) + shape[1:]), shape[0], op.reach, outputs=op.outputs, compare=compare,
                what=(op.id, shape))


_id = lambda op: op.id   # noqa: E731


# ------------------------------------------------------------------------------------------------ 1. 3-D, z-periodic
@pytest.mark.parametrize("op", [o for o in LI.volume_ops(3) if not o.pd], ids=_id)
def test_volume_past_2_to_the_31(op):
    run_volume_op(op, 3)


@pytest.mark.parametrize("op", [o for o in LI.volume_ops(3) if o.pd], ids=_id)
def test_pd_tv_volume_past_2_to_the_31(op, pd_arith):
    run_volume_op(op, 3, pd_arith)


# ------------------------------------------------------------------------------------------------ 2. 2-D, y-periodic
@pytest.mark.parametrize("op", [o for o in LI.volume_ops(2) if not o.pd], ids=_id)
def test_image_at_the_descriptor_limit(op):
    run_volume_op(op, 2)


@pytest.mark.parametrize("op", [o for o in LI.volume_ops(2) if o.pd], ids=_id)
def test_pd_tv_image_at_the_descriptor_limit(op, pd_arith):
    run_volume_op(op, 2, pd_arith)


# ------------------------------------------------------------------------------------------------ 3. vectors past 2^32
A, B, LO, VALUE, BETA = np.float32(0.75), np.float32(-1.5), np.float32(0.25), np.float32(0.375), np.float32(0.5)
SIGMA, TAU, W = np.float32(0.25), np.float32(0.125), np.float32(2.0)
F32 = np.float32


def _recip(x):
    with np.errstate(divide="ignore"):
        r = (F32(1) / x).astype(np.float32)
    return np.where(np.isnan(r) | np.isinf(r), F32(1), r).astype(np.float32)


def _vector_cases():
    """name -> (signs of the inputs' periods ("s": signed dyadic, "p": positive dyadic), NaN-filled outputs,
    call(ops, ins, outs) -> the tensors that hold the results, want(*periods) -> their expected periods)"""
    import _pdhg_diag_oracle as PD
    import _pdhg_oracle as PO
    import _spdhg_oracle as SO
    c = {
        "axpby": ("ss", 0, lambda ops, i, o: (ops.axpby(A, i[0], B, i[1]), [i[1]])[1], lambda x, y: [A * x + B * y]),
        "scale": ("s", 1, lambda ops, i, o: (ops.scale(A, i[0], o[0]), o)[1], lambda x: [A * x]),
        "mul": ("ss", 0, lambda ops, i, o: (ops.mul(i[0], i[1]), [i[1]])[1], lambda x, y: [x * y]),
        "fill": ("", 1, lambda ops, i, o: (ops.fill(o[0], VALUE), o)[1], lambda: [np.full(LI.DYADIC_PERIOD, VALUE, np.float32)]),
        "clamp_min": ("s", 0, lambda ops, i, o: (ops.clamp_min(i[0], LO), [i[0]])[1], lambda x: [np.where(x < LO, LO, x)]),
        "recip_safe": ("s", 1, lambda ops, i, o: (ops.recip_safe(i[0], o[0]), o)[1], lambda x: [_recip(x)]),
        "momentum": ("ss", 1, lambda ops, i, o: (ops.momentum(i[0], i[1], o[0], BETA), o)[1], lambda x, y: [x + BETA * (x - y)]),
        "admm_dual": ("sss", 0, lambda ops, i, o: (ops.admm_dual(i[0], i[1], i[2]), [i[0]])[1], lambda u, z, x: [u + (z - x)]),
        "pwls_weights": ("p", 0, lambda ops, i, o: [ops.pwls_weights(i[0])], lambda b: [np.maximum(b, F32(1e-6)) / b.max()]),
        "spdhg_primal": ("sss", 0, lambda ops, i, o: (ops.spdhg_primal(i[0], i[1], i[2], TAU, W, True), [i[0], i[1]])[1],
                         lambda x, z, d: list(SO.primal_step(x, z, d, TAU, W, True))),
        "pdhg_diag_steps": ("p", 1, lambda ops, i, o: (ops.pdhg_diag_steps(o[0], i[0], A, LO), o)[1], lambda s: [PD.diag_steps(s, A, LO)]),
    }
    for fid in ("LS", "L1", "KL"):
        c[f"pdhg_sino_dual-{fid}"] = ("ssp", 0, lambda ops, i, o, fid=fid: [ops.pdhg_sino_dual(i[0], i[1], i[2], fid, SIGMA)],
                                      lambda y, r, b, fid=fid: [PO.sino_dual(y, r, b, fid, SIGMA)])
        c[f"pdhg_sino_dual_diag-{fid}"] = ("sspp", 0, lambda ops, i, o, fid=fid: [ops.pdhg_sino_dual_diag(i[0], i[1], i[2], i[3], fid)],
                                           lambda y, r, b, s, fid=fid: [PD.sino_dual(y, r, b, fid, s)])
    c["spdhg_sino_dual-KL"] = ("ssp", 0, lambda ops, i, o: list(ops.spdhg_sino_dual(i[0], i[1], i[2], "KL", SIGMA)),
                               lambda y, r, b: list(SO.sino_step(y, r, b, "KL", SIGMA)))
    return c


VECTOR_CASES = _vector_cases()


def shifted(n, shift, fill=None):
    """`n` floats that start 4 * shift bytes past a 16-byte boundary (shift 0: the float4 body and its tail; 1: the scalar
    path), as tests/_guarded.guarded(shift=) places them"""
    raw = torch.empty(n + 4, dtype=torch.float32, device="cuda")
    off = (-(raw.data_ptr() // 4)) % 4 + shift
    v = raw[off:off + n]
    assert v.data_ptr() % 16 == 4 * shift
    if fill is not None:
        v.fill_(fill)
    return v


def vector_inputs(signs, shift, n=LI.VECTOR):
    periods = [LI.dyadic(10 + k, positive=(s == "p")) for k, s in enumerate(signs)]
    devs = [torch.from_numpy(p).cuda() for p in periods]
    return periods, devs, [LI.tiled(d, n, out=shifted(n, shift)) for d in devs]


def assert_tiled(x, period_dev, what):
    z = LI.first_unequal_plane(x, period_dev, 0, x.shape[0], 0)
    assert z is None, (what, "differs from the expected period at " + LI._where(z, LI.plane_elems(x.shape)))


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("name", list(VECTOR_CASES))
def test_vector_past_2_to_the_32(name, shift):
    from tomobar_amd import ops
    signs, n_out, call, want = VECTOR_CASES[name]
    need(4 * (LI.VECTOR + 4) * (len(signs) + max(n_out, 1)))
    periods, devs, ins = vector_inputs(signs, shift)
    outs = [shifted(LI.VECTOR, shift, float("nan")) for _ in range(n_out)]
    res = call(ops, ins, outs)
    torch.cuda.synchronize()
    wants = want(*periods)
    assert len(res) == len(wants)
    for k, (r, w) in enumerate(zip(res, wants)):
        assert r.numel() == LI.VECTOR and w.dtype == np.float32
        assert_tiled(r, torch.from_numpy(np.ascontiguousarray(w)).cuda(), (name, shift, "result", k))
    for k, (x, d) in enumerate(zip(ins, devs)):
        if not any(x is r for r in res):
            assert_tiled(x, d, (name, shift, "input", k, "was written"))


@pytest.mark.parametrize("shift", [0, 1])
def test_reductions_past_2_to_the_32(shift):
    """exact sums: with dyadic data the expected value does not depend on the order, so equality, not a tolerance"""
    from tomobar_amd import _lib, ops
    need(4 * (LI.VECTOR + 4) * 3)
    n = LI.VECTOR
    (x, y), _, (xd, yd) = vector_inputs("ss", shift)
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    assert ops.norm2(xd) == math.sqrt(LI.tiled_sum(x64 * x64, n))
    assert ops.dot(xd, yd) == LI.tiled_sum(x64 * y64, n)
    want = (LI.tiled_sum((x64 - y64) ** 2, n), LI.tiled_sum(x64 * x64, n))
    assert ops.rel_change(xd, yd) == want
    keep = shifted(n, shift, float("nan"))
    assert ops.rel_change(xd, yd, keep) == want
    assert_tiled(keep, torch.from_numpy(x).cuda(), ("rel_change", shift, "keep"))
    del keep
    assert ops.rel_change(xd, yd, yd) == want          # keep may be the reference itself
    assert_tiled(yd, torch.from_numpy(x).cuda(), ("rel_change", shift, "keep = ref"))
    m = C.c_float(0.0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib().tomo_max(C.c_void_p(xd.data_ptr()), n, C.byref(m), stream))
    assert m.value == float(x.max())
    xd[-1] = 3.0                                         # the one largest value is the last element
    _lib.check(_lib.lib().tomo_max(C.c_void_p(xd.data_ptr()), n, C.byref(m), stream))
    assert m.value == 3.0


# ------------------------------------------------------------------------------------------------ 4. slice-periodic
def _slices_base():
    import _slicewise_cases as S
    return S.volume((LI.PERIOD,) + LI.PLANE)


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_pdtv_slices_past_2_to_the_31(half, pd_arith):
    import _slicewise_cases as S
    from tomobar_amd.regularisersCuPy import PD_TV_cupy
    need(LI.footprint("PD_TV_slices", LI.TALL))

    def gpu(ins, outs):
        PD_TV_cupy(ins[0], S.LAM, 7, 0, 0, S.LIPSCHITZ, 0, half, out=outs[0], slicewise=True)

    LI.periodic(gpu, lambda w: [S.oracle_slices("PD_TV", w, **S.pd_kwargs(7, half=half))], _slices_base(), LI.TALL[0], 0,
                compare=lambda got, want, what: pd_arith.check(got, want, half=half, what=str(what)), what="pdtv_slices")


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_roftv_slices_past_2_to_the_31(half):
    import _slicewise_cases as S
    from tomobar_amd.regularisersCuPy import ROF_TV_cupy
    need(LI.footprint("ROF_TV_slices", LI.TALL))

    def gpu(ins, outs):
        ROF_TV_cupy(ins[0], S.LAM, 3, S.ROF_TAU, 0, half, out=outs[0], slicewise=True)

    LI.periodic(gpu, lambda w: [S.oracle_slices("ROF_TV", w, **S.rof_kwargs(3, half=half))], _slices_base(), LI.TALL[0], 0,
                what="roftv_slices")


WL_T = np.float32(0.5)


def test_wavelet_shrink_past_2_to_the_31():
    import _wavelet_oracle as W
    from tomobar_amd import ops
    need(LI.footprint("WAVELETS", LI.TALL))

    def gpu(ins, outs):
        ops.wavelet_shrink(ins[0], WL_T, out=outs[0])

    LI.periodic(gpu, lambda w: [W.shrink(w, WL_T)], _slices_base(), LI.TALL[0], 0, what="wavelet_shrink")


def test_wavelet_forward_past_2_to_the_31():
    import _wavelet_oracle as W
    from tomobar_amd import ops
    need(LI.footprint("wavelet pyramid", LI.TALL, 1) + 4 * ops.wavelet_pyramid_floats(LI.TALL))
    LI.periodic(lambda ins, outs: [ops.wavelet_forward(ins[0], WL_T).view(LI.TALL[0], -1)],
                lambda w: [W.pack(W.forward(w, WL_T)).reshape(w.shape[0], -1)], _slices_base(), LI.TALL[0], 0, outputs=0,
                what="wavelet_forward")


def test_wavelet_inverse_past_2_to_the_31():
    import _wavelet_oracle as W
    from tomobar_amd import ops
    need(LI.footprint("wavelet pyramid", LI.TALL, 1) + 4 * ops.wavelet_pyramid_floats(LI.TALL))
    base = _slices_base()
    pyr = W.pack(W.forward(base, WL_T)).reshape(LI.PERIOD, -1)

    def gpu(ins, outs):   # LL of levels 1 and 2 of the pyramid are overwritten on the way
        out = torch.full(LI.TALL, float("nan"), dtype=torch.float32, device="cuda")
        ops.wavelet_inverse(ins[0].view(-1), LI.TALL, out=out)
        return [out]

    def oracle(w):
        shape = (w.shape[0],) + LI.PLANE
        return [W.inverse(W.unpack(w.reshape(-1), shape), shape)]

    LI.periodic(gpu, oracle, pyr, LI.TALL[0], 0, outputs=0, scratch=(0,), what="wavelet_inverse")


def test_patch_select_and_nltv_with_tables_past_2_to_the_31():
    """K = 8 neighbours on a stack whose K * nvox passes 2^31: the tables' index k * nvox + at.  Both operators act slice by
    slice, so every slice of every table and of the result is the oracle's for that slice of the period."""
    import _nltv_oracle as N
    from tomobar_amd import ops
    shape, params, h, lam = LI.NLTV_STACK, (3, 1, 8), F32(0.3), F32(0.02)
    assert 8 * LI.numel(shape) > 2 ** 31
    need(LI.footprint("NLTV", shape, 2 + 16))
    base = N.noisy_phantom((LI.PERIOD,) + shape[1:])
    want_tables = N.patch_select(base, *params, h)
    base_dev = torch.from_numpy(base).cuda()
    x = LI.tiled(base_dev, shape[0])
    tables = ops.patch_select(x, *params, h)

    def check_tables(when):
        for name, t, w in zip(("H_i", "H_j", "Weights"), tables, want_tables):
            assert tuple(t.shape) == (8,) + shape
            for k in range(8):
                assert_tiled(t[k], torch.from_numpy(np.ascontiguousarray(w[k])).cuda(), (name, "neighbour", k, when))

    check_tables("after patch_select")
    out = torch.full_like(x, float("nan"))
    _, done, _ = ops.nltv(x, out, *tables, lam, 2)      # two iterations: through the work array and back
    assert done == 2
    assert_tiled(out, torch.from_numpy(N.nltv(base, *want_tables, lam, 2)).cuda(), "nltv")
    assert_tiled(x, base_dev, "the input was written")
    check_tables("after nltv")


# ------------------------------------------------------------------------------------------------ 5. projectors
@pytest.mark.parametrize("geom", ["volume", "sinogram"])
def test_projector_pair_past_2_to_the_31(oracle, geom):
    """forward, backward, the matched backward, the LS residual and the FISTA epilogue of both back projectors on
    vol[z] = base[z % 5]: A and A^T act slice by slice, so every slice is the oracle's for that slice of the period"""
    import _matched_bp_oracle as M
    import test_gpu_bp_epilogues as EP
    from tomobar_amd.projector import HipTools3D
    g = LI.PROJ_VOLUME if geom == "volume" else LI.PROJ_SINO
    nz, n, nu, na, p = g["nz"], g["n"], g["nu"], g["na"], LI.PROJ_PERIOD
    assert max(nz * n * n, nz * na * nu) > 2 ** 31
    need(4 * (3 * nz * n * n + 3 * nz * na * nu))
    angles = np.linspace(0.1, np.pi + 0.1, na, endpoint=False)
    P, PM = oracle.Projector(p, n, nu, angles, 0.0, 1), M.MatchedProjector(p, n, nu, angles, 0.0, 1)
    H = HipTools3D(nu, 0, nz, angles, 0.0, n, "gpu", 0, None)
    try:
        rng = np.random.default_rng(31)
        base_v = rng.standard_normal((p, n, n)).astype(np.float32)
        base_s = rng.standard_normal((p, na, nu)).astype(np.float32)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()   # noqa: E731
        vol_p, sino_p = dev(base_v), dev(base_s)
        vol, sino = LI.tiled(vol_p, nz), LI.tiled(sino_p, nz)
        ax = P.fp(base_v, None)
        out = torch.full_like(sino, float("nan"))
        H.forward(vol, None, out=out)
        assert_tiled(out, dev(ax), (geom, "forward"))
        out.fill_(float("nan"))
        H.residual(vol, sino, None, "LS", None, out)
        assert_tiled(out, dev(ax - base_s), (geom, "LS residual"))
        del out
        for adjoint, op in (("unmatched", P), ("matched", PM)):
            grad = op.bp(base_s, None)
            out = torch.full_like(vol, float("nan"))
            H.backward(sino, None, out=out, adjoint=adjoint)
            assert H.kernel_path("bp").startswith("matched") == (adjoint == "matched")
            assert_tiled(out, dev(grad), (geom, adjoint, "backward"))
            out.fill_(float("nan"))
            H.adjoint = adjoint
            H.grad_step(sino, vol, out, EP.LINV, True, None)       # x_t = the volume
            assert_tiled(out, dev(EP.restate("fista", grad, base_v, nonneg=True)[0]), (geom, adjoint, "FISTA epilogue"))
            del out
        assert_tiled(vol, vol_p, (geom, "the volume was written"))
        assert_tiled(sino, sino_p, (geom, "the sinogram was written"))
    finally:
        H.release_scratch()
