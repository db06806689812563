"""The private quad-interleaved X_t of the FISTA loop (TOMO_VOLUME_ZQUAD, include/tomo_mi355x.h): its producers (momentum,
converter), the forward projector's LDS-DMA staging from it, the back projector's gradient-step epilogue reading it, and
the driver end to end against the forced-planar switch.  Data movement plus unchanged arithmetic: every comparison is
array_equal.  The projector shapes are the smallest at which both stepping axes plan the whole-row double-buffered form;
each test asserts the kernel path string, so a planner change cannot turn it into a test of the planar path."""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FULL = (0.1, math.pi + 0.1)   # the parity tests' angle range: both stepping axes, both signs of the detector slope
QV = "quad-interleaved volume, LDS-DMA staging"


def _tools(nz, n, nu, na, cor=0.0, os_n=None, rng=FULL):
    from tomobar_amd.projector import HipTools3D
    return HipTools3D(nu, 0, nz, np.linspace(rng[0], rng[1], na, endpoint=False), cor, n, "gpu", 0, os_n)


def _randn(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape, dtype=np.float32)).cuda()


def _relay(planar):
    """[nz][n][n] -> [ceil(nz/4)][n][n][4] with zero padding slices, by torch."""
    nz, n, _ = planar.shape
    nq = (nz + 3) // 4
    pad = torch.zeros((nq * 4, n, n), dtype=planar.dtype, device=planar.device)
    pad[:nz] = planar
    return pad.reshape(nq, 4, n, n).permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------------------------------ 1. producers
@pytest.mark.parametrize("n", [40, 64, 100])      # below a 64 x 64 tile, on it, past it
@pytest.mark.parametrize("nz", [1, 4, 6, 9])      # a lone quad, an exact one, zero-filled tails
def test_producers_match_the_planar_momentum_relaid(nz, n):
    H = _tools(nz, n, 128, 8)
    x, xold = _randn((nz, n, n), 1), _randn((nz, n, n), 2)
    for beta in (0.0, 0.7391357421875 + 2.0 ** -20):
        want = torch.empty_like(x)
        H.set_volume_layout("planar")
        H.momentum(x, xold, want, beta)
        H.set_volume_layout("zquad", require_ok=False)
        got = H.volume_buffer().fill_(float("nan"))
        H.momentum(x, xold, got, beta)
        assert got.shape == ((nz + 3) // 4, n, n, 4)
        assert torch.equal(got, _relay(want))
        if nz % 4:
            assert torch.equal(got[-1, :, :, nz % 4:], torch.zeros_like(got[-1, :, :, nz % 4:]))   # exactly zero
        assert torch.equal(H.volume_as_planar(got), want)
    conv = H.volume_to_zquad(x, out=H.volume_buffer().fill_(float("nan")))
    assert torch.equal(conv, _relay(x))
    H.set_volume_layout("planar")


def test_buffers_of_the_other_layout_are_refused():
    H = _tools(6, 64, 128, 8)
    x = _randn((6, 64, 64), 1)
    H.set_volume_layout("zquad", require_ok=False)
    with pytest.raises(ValueError):
        H.momentum(x, x, torch.empty_like(x), 0.5)           # planar X_t under the zquad layout
    with pytest.raises(ValueError):
        H.grad_step(H.residual_buffer(None), x, torch.empty_like(x), 1e-3, True, None)
    H.set_volume_layout("planar")


# ------------------------------------------------------------------------------------------------ 2. forward projector
# name, nz, n, nu, na, angle range, cor, OS number, the form both axes must take, angles per workgroup.  The angle range
# splits evenly between the stepping axes; a class runs groups of 13 where they pad to no more slots than groups of 8.
FP_CASES = [
    ("1pass", 6, 120, 128, 24, FULL, 0.0, 1, "1 passes, 4 rows/chunk", 13),              # n = 64 + 56: partial producer tiles; 12 of 13 slots
    ("2pass_kc4", 5, 200, 128, 40, FULL, 0.0, 1, "2 passes, 4 rows/chunk", 8),           # 20 an axis: groups of 8, 8, 4
    ("2pass_kc2", 2, 1300, 1024, 16, FULL, 0.0, 1, "2 passes, 2 rows/chunk", 8),         # 8 an axis: one full group
    ("2pass_groups_of_13", 3, 200, 128, 52, FULL, 0.0, 1, "2 passes, 4 rows/chunk", 13),  # 26 an axis: two full groups of 13
    ("wide_detector_offset_cor", 7, 100, 192, 24, FULL, 13.5, 1, "1 passes, 4 rows/chunk", 13),   # rays leave sideways
    ("few_angles_os", 4, 120, 128, 18, FULL, -2.5, 3, "1 passes, 4 rows/chunk", 8),      # 6 angles a subset: 3 + 3, below one group
]


@pytest.mark.parametrize("case", FP_CASES, ids=[c[0] for c in FP_CASES])
def test_residual_from_the_zquad_volume_equals_the_planar_one(case):
    name, nz, n, nu, na, rng, cor, os_n, form, group = case
    H = _tools(nz, n, nu, na, cor, os_n if os_n > 1 else None, rng)
    vol = _randn((nz, n, n), 5)
    b = torch.rand((nz, na, nu), device="cuda") + 0.5
    w = torch.rand((nz, na, nu), device="cuda")
    subs = [None] if os_n == 1 else [0, os_n - 1]
    for s in subs:
        assert H.volume_zquad_ok(s), name
    for layout in ("zquad", "planar"):
        H.set_residual_layout(layout)
        for s in subs:
            for fid in ("LS", "PWLS", "KL"):
                wt = w if fid == "PWLS" else None
                H.set_volume_layout("planar")
                want = H.residual(vol if fid != "KL" else vol.abs(), b, wt, fid, s, H.residual_buffer(s))
                assert "whole-row" in H.kernel_path("fp") and QV not in H.kernel_path("fp")
                H.set_volume_layout("zquad")
                xq = H.volume_to_zquad(vol if fid != "KL" else vol.abs())
                got = H.residual(xq, b, wt, fid, s, H.residual_buffer(s).fill_(float("nan")))
                path = H.kernel_path("fp")
                assert path.count(QV) == 2 and path.count(form) == 2 and path.startswith("y:") and " x:" in path, path
                assert path.count(QV + ", 13 angles)") == (2 if group == 13 else 0) and path.count(QV + ")") == (2 if group == 8 else 0), path
                assert torch.equal(got, want), (name, layout, s, fid)
    # the transposed twin is a one-shot token: a second projection of the same buffer is refused, not quietly converted
    with pytest.raises(ValueError):
        H.residual(xq, b, None, "LS", subs[-1], H.residual_buffer(subs[-1]))
    H.set_volume_layout("planar")
    H.set_residual_layout("planar")


def test_an_ineligible_geometry_says_no_and_stays_planar():
    from tomobar_amd.methodsIR_CuPy import RecToolsIRCuPy
    nz, n, na = 4, 200, 20                      # a 100-pixel detector: 256-pixel tiles, not the whole-row form
    H = _tools(nz, n, 100, na)
    assert not H.volume_zquad_ok(None)
    with pytest.raises(ValueError):
        H.set_volume_layout("zquad")
    assert H.volume_layout() == "planar"
    H.set_volume_layout("zquad", require_ok=False)
    xq = H.volume_to_zquad(_randn((nz, n, n), 5))
    with pytest.raises(ValueError):             # the entry point refuses: no quiet conversion
        H.residual(xq, torch.zeros((nz, na, 100), device="cuda"), None, "LS", None, H.residual_buffer(None))
    H.set_volume_layout("planar")
    rt = RecToolsIRCuPy(100, 0, nz, 0.0, np.linspace(FULL[0], FULL[1], na, endpoint=False), n, 0, None)
    rt.FISTA({"projection_data": torch.rand((nz, na, 100), device="cuda"), "data_axes_labels_order": ["detY", "angles", "detX"]},
             {"iterations": 2, "lipschitz_const": 5e4, "nonnegativity": True},
             {"method": "PD_TV", "regul_param": 0.002, "iterations": 2})
    assert "tiled-pipelined" in rt.Atools.kernel_path("fp") and QV not in rt.Atools.kernel_path("fp")


# ------------------------------------------------------------------------------------------------ 3. back-projector epilogue
@pytest.mark.parametrize("nonneg", [True, False])
@pytest.mark.parametrize("nz,n,misaligned", [(16, 64, False),      # whole bricks: the LDS hand-over and dwordx4 stores
                                             (22, 44, False),      # partial bricks on all three axes, nz % 4 != 0
                                             (16, 64, True)])      # output pointer off by one float: epi_aligned false
def test_gradient_step_from_the_zquad_volume_equals_the_planar_one(nz, n, misaligned, nonneg):
    na, nu = 12, 128
    H = _tools(nz, n, nu, na)
    xt = _randn((nz, n, n), 7)
    H.set_residual_layout("zquad")
    res = H.residual(xt, _randn((nz, na, nu), 8), None, "LS", None, H.residual_buffer(None))

    def out_buffer():
        flat = torch.full((nz * n * n + 4,), float("nan"), device="cuda")
        return flat[1:1 + nz * n * n].view(nz, n, n) if misaligned else flat[:nz * n * n].view(nz, n, n)

    want, got = out_buffer(), out_buffer()
    assert (want.data_ptr() % 16 != 0) == misaligned
    H.grad_step(res, xt, want, 3e-3, nonneg, None)
    H.set_volume_layout("zquad", require_ok=False)
    xq = H.volume_to_zquad(xt)
    H.grad_step(res, xq, got, 3e-3, nonneg, None)
    assert "brick" in H.kernel_path("bp")
    assert not torch.isnan(got).any() and (got < 0).any() != nonneg
    assert torch.equal(got, want)
    H.set_volume_layout("planar")
    H.set_residual_layout("planar")


# ------------------------------------------------------------------------------------------------ 4. end to end
@pytest.mark.parametrize("nz", [6, 8])
def test_fista_os_pdtv_zquad_equals_the_forced_planar_run(nz):
    from tomobar_amd import ops
    from tomobar_amd.methodsIR_CuPy import RecToolsIRCuPy
    n, na, os_n = 128, 48, 3
    angles = np.linspace(FULL[0], FULL[1], na, endpoint=False)
    data = {"projection_data": torch.rand((nz, na, n), device="cuda") * n, "data_axes_labels_order": ["detY", "angles", "detX"]}
    reg = {"method": "PD_TV", "regul_param": 0.002, "iterations": 4}
    rt = RecToolsIRCuPy(n, 0, nz, 0.0, angles, n, 0, os_n)

    def run(x0):
        alg = {"iterations": 2, "lipschitz_const": 2e4, "nonnegativity": True, "initialise": x0}
        out = rt.FISTA(dict(data), alg, dict(reg)).clone()
        assert rt.Atools.volume_layout() == "planar" and rt.Atools.residual_layout() == "planar"   # reset in `finally`
        return out, rt.Atools.kernel_path("fp")

    for seed in (None, 3):       # the second call starts elsewhere: nothing of the first call's token may survive
        x0 = None if seed is None else torch.rand((nz, n, n), device="cuda")
        got, path = run(x0)
        assert path.count(QV) == 2, path
        ops.set_variant("fp", 5)     # the A/B switch of the shipped library: the drivers keep the planar X_t
        try:
            want, path = run(x0)
        finally:
            ops.set_variant("fp", 0)
        assert "whole-row" in path and QV not in path, path
        assert torch.equal(got, want)
        assert float(got.abs().max()) > 0.0
