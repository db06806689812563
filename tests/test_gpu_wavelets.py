"""MI355X: the wavelet shrinkage behind the `_WAVELETS` suffix (tomobar_amd/csrc/wavelet_kernels.hip, docs/kernels/wavelets.md)
against its float32 numpy restatement tests/_wavelet_oracle.py, bit for bit (there is no reference implementation:
formula-level parity, unpinned) -- the C entry points, WAVELETS_cupy, prox_regul with `<kind>_WAVELETS` and the three
drivers that reach it.

Shapes: a tile is 32 x 32 coefficients (64 x 64 samples).  (1, 1) .. (16, 24) are shorter than the 10 taps at some level, so
the circular apron wraps more than once ((16, 24): at levels 2 and 3); (150, 200) is 3 x 4 ragged tiles at level 1, 2 x 2 at
level 2 and one at level 3, with odd sizes (75, 19 x 25) on the way; the 3D shapes add grid z, (3, 70, 131) with an odd
width over three tiles."""
import types

import numpy as np
import pytest
import torch

import _wavelet_oracle as W
from _march_gpu import host, same_bits
from _tgv_oracle import phantom

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 3), (1, 37), (37, 1), (13, 37), (16, 24), (150, 200), (7, 13, 37), (3, 70, 131)]
_ids = lambda s: "x".join(map(str, s))   # noqa: E731
_want = {}


def above_every_detail(f):
    """a threshold above every detail coefficient of every level (from the float64 transform, doubled)"""
    return 2.0 * max(float(np.abs(b).max()) for lev in W.forward(f, 0.0, np.float64) for b in lev[1:]) + 1.0


def thresholds(f):
    return (0.0, 0.02, above_every_detail(f))


def want(shape, t):
    """the oracle's (pyramid, W_t) of the phantom, computed once per (shape, t)"""
    key = (shape, float(t))
    if key not in _want:
        f = phantom(shape)
        levels = W.forward(f, t, np.float32)
        _want[key] = (W.pack(levels), W.inverse(levels, shape, np.float32))
    return _want[key]


def mix_of(shape):
    return (phantom(shape)[..., ::-1] * np.float32(0.37)).copy()


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_shrink_and_forward_equal_the_oracle(shape):
    from tomobar_amd import ops
    f = phantom(shape)
    x = torch.from_numpy(f).cuda()
    m_host = mix_of(shape)
    for t in thresholds(f):
        pyr, w = want(shape, t)
        same_bits(host(ops.wavelet_forward(x, np.float32(t))), pyr, (shape, t, "pyramid"))
        # without mix
        out = torch.full_like(x, float("nan"))
        assert ops.wavelet_shrink(x, np.float32(t), out=out) is out
        same_bits(host(out), w, (shape, t, "shrink"))
        # with mix in an array of its own, and with mix aliasing out
        mixed = (m_host + w) * np.float32(0.5)
        m = torch.from_numpy(m_host).cuda()
        out = torch.full_like(x, float("nan"))
        ops.wavelet_shrink(x, np.float32(t), out=out, mix=m)
        same_bits(host(out), mixed, (shape, t, "mix"))
        same_bits(host(m), m_host, (shape, t, "mix was written"))
        ops.wavelet_shrink(x, np.float32(t), out=m, mix=m)
        same_bits(host(m), mixed, (shape, t, "mix aliasing out"))
        same_bits(host(x), f, (shape, t, "the input was written"))


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_inverse_of_the_oracle_pyramid(shape):
    from tomobar_amd import ops
    pyr, w = want(shape, 0.02)
    p = torch.from_numpy(pyr).cuda()
    out = torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
    ops.wavelet_inverse(p, shape, out=out)
    same_bits(host(out), w, (shape, "inverse"))
    m_host = mix_of(shape)
    m = torch.from_numpy(m_host).cuda()
    ops.wavelet_inverse(torch.from_numpy(pyr).cuda(), shape, out=m, mix=m)
    same_bits(host(m), (m_host + w) * np.float32(0.5), (shape, "inverse, mix aliasing out"))


def test_c_entry_points_refuse_invalid_arguments():
    import ctypes as C
    from tomobar_amd import _lib as L
    lib = L.lib()
    x = torch.zeros((4, 6), dtype=torch.float32, device="cuda")
    p = torch.zeros(int(lib.tomo_wavelet_scratch_bytes(6, 4, 1, 2)) // 4, dtype=torch.float32, device="cuda")
    X, P, null = C.c_void_p(x.data_ptr()), C.c_void_p(p.data_ptr()), C.c_void_p(0)
    assert lib.tomo_wavelet_scratch_bytes(6, 4, 1, 2) == 4 * 4 * (2 * 3 + 1 * 2 + 1 * 1)
    assert lib.tomo_wavelet_scratch_bytes(6, 4, 5, 3) == 5 * lib.tomo_wavelet_scratch_bytes(6, 4, 1, 2)
    assert lib.tomo_wavelet_scratch_bytes(0, 4, 1, 2) == 0 and lib.tomo_wavelet_scratch_bytes(6, 4, 1, 4) == 0
    bad = [lib.tomo_wavelet_shrink(0, X, X, null, 6, 4, 1, 2, -1.0, null),
           lib.tomo_wavelet_shrink(0, X, X, null, 6, 4, 1, 2, float("nan"), null),
           lib.tomo_wavelet_shrink(0, X, X, null, 6, 0, 1, 2, 0.1, null),
           lib.tomo_wavelet_shrink(0, X, X, null, 6, 4, 0, 3, 0.1, null),
           lib.tomo_wavelet_shrink(0, X, X, null, 6, 4, 1, 1, 0.1, null),
           lib.tomo_wavelet_shrink(0, null, X, null, 6, 4, 1, 2, 0.1, null),
           lib.tomo_wavelet_shrink(0, X, null, null, 6, 4, 1, 2, 0.1, null),
           lib.tomo_wavelet_shrink(-1, X, X, null, 6, 4, 1, 2, 0.1, null),
           lib.tomo_wavelet_forward(0, X, P, 6, 4, 1, 2, -0.5, null),
           lib.tomo_wavelet_forward(0, X, null, 6, 4, 1, 2, 0.5, null),
           lib.tomo_wavelet_inverse(0, null, X, null, 6, 4, 1, 2, null),
           lib.tomo_wavelet_inverse(0, P, X, null, 0, 4, 1, 2, null)]
    assert bad == [L.E_INVALID] * len(bad)
    torch.cuda.synchronize()
    assert float(x.abs().sum()) == 0.0


# -------------------------------------------------------------------------------------------------- WAVELETS_cupy
def test_wavelets_cupy_surface():
    import tomobar_amd
    from tomobar_amd.regularisersCuPy import WAVELETS_cupy, last_prox
    assert tomobar_amd.WAVELETS_cupy is WAVELETS_cupy
    plane = phantom((13, 37))
    want2d = want((13, 37), 0.02)[1]
    before = last_prox()
    for axis in range(3):   # a singleton axis in each position runs as one 2D slice and keeps its shape
        x = torch.from_numpy(np.expand_dims(plane, axis)).cuda()
        got = WAVELETS_cupy(x, 0.02)
        assert tuple(got.shape) == tuple(x.shape)
        same_bits(np.squeeze(host(got), axis), want2d, ("singleton axis", axis))
    assert last_prox() == before
    vol = phantom((7, 13, 37))
    want3d = want((7, 13, 37), 0.02)[1]
    xt = torch.from_numpy(np.ascontiguousarray(vol.transpose(2, 1, 0))).cuda().permute(2, 1, 0)
    assert not xt.is_contiguous()
    keep = xt.clone()
    same_bits(host(WAVELETS_cupy(xt, 0.02, 0)), want3d, "non-contiguous input")
    assert torch.equal(xt, keep), "the input array was written"
    x = torch.from_numpy(vol).cuda()
    out = torch.full_like(x, float("nan"))
    res = WAVELETS_cupy(x, 0.02, out=out)
    assert res.data_ptr() == out.data_ptr()
    same_bits(host(out), want3d, "out=")
    # a threshold of 0 is accepted: the identity up to rounding.  The bound: 12 one-axis passes (3 levels x 2 axes, there
    # and back), each a sum of 10 rounded products -- at most 11 u sum|h| max|x| with sum|h| < 2, u = 2^-24 --, and the
    # orthonormal passes do not amplify what the earlier ones left
    ident = host(WAVELETS_cupy(x, 0.0))
    same_bits(ident, want((7, 13, 37), 0.0)[1], "threshold 0")
    assert np.abs(ident - vol).max() <= 12 * 11 * 2 * 2.0 ** -24 * np.abs(vol).max()
    with pytest.raises(ValueError, match="float32"):
        WAVELETS_cupy(x.double(), 0.02)
    with pytest.raises(ValueError, match="negative"):
        WAVELETS_cupy(x, -0.02)
    with pytest.raises(ValueError, match="gpu_device"):
        WAVELETS_cupy(x, 0.02, -1)
    with pytest.raises(ValueError, match="2D or 3D"):
        WAVELETS_cupy(x[None], 0.02)
    # the z-slab property: W of a range of planes is that range of W of the volume
    for z0, z1 in ((0, 3), (3, 7), (2, 5)):
        same_bits(host(WAVELETS_cupy(x[z0:z1], 0.02)), want3d[z0:z1], ("planes", z0, z1))


# -------------------------------------------------------------------------------------------------- prox_regul
T = 0.03
KIND_REG = {
    "ROF_TV": dict(regul_param=0.4, iterations=6, time_marching_step=0.01),
    "PD_TV": dict(regul_param=0.4, iterations=6, methodTV=0, PD_LipschitzConstant=8.0),
    "TGV": dict(regul_param=0.4, iterations=6, PD_LipschitzConstant=12.0),
    "NDF": dict(regul_param=1.0, iterations=6, time_marching_step=0.05, edge_threshold=2.0),
    "Diff4th": dict(regul_param=1.0, iterations=6, time_marching_step=0.005, edge_threshold=2.0),
}
CASES = [(k, False) for k in KIND_REG] + [("PD_TV", True)]


def _self(slab=None):
    return types.SimpleNamespace(nonneg_regul=0, Atools=types.SimpleNamespace(device_index=0), slab=slab)


@pytest.mark.parametrize("kind, exact", CASES, ids=[k + ("-exact_roundings" if e else "") for k, e in CASES])
def test_prox_regul_averages_the_kind_with_the_oracle_shrinkage(kind, exact, shape=(7, 13, 37)):
    from tomobar_amd.regularisersCuPy import last_prox, prox_regul
    f = phantom(shape)
    x = torch.from_numpy(f).cuda()
    reg = dict(KIND_REG[kind], method=kind, **({"exact_roundings": True} if exact else {}))
    plain = host(prox_regul(_self(), x, dict(reg)))            # the shipped kernel of the kind
    record = last_prox()
    w = want(shape, T)[1]                                      # the oracle's shrinkage
    for out in (None, torch.full_like(x, float("nan"))):
        got = prox_regul(_self(), x, dict(reg, method=kind + "_WAVELETS", regul_param2=T), out=out)
        assert out is None or got.data_ptr() == out.data_ptr()
        same_bits(host(got), (plain + w) * np.float32(0.5), (kind, exact, out is None))
        assert last_prox()[0] == record[0] == 6
    same_bits(host(x), f, "the input was written")
    assert not np.array_equal(plain, (plain + w) * np.float32(0.5))
    # the default threshold is regul_param2 = 0.001
    got = prox_regul(_self(), x, dict(reg, method=kind + "_WAVELETS"))
    same_bits(host(got), (plain + want(shape, 0.001)[1]) * np.float32(0.5), (kind, "default threshold"))


def test_prox_regul_refusals_and_slab_mode(shape=(7, 13, 37)):
    from tomobar_amd import slab as S
    from tomobar_amd.regularisersCuPy import prox_regul, reserve_prox_scratch
    x = torch.from_numpy(phantom(shape)).cuda()
    with pytest.raises(ValueError, match="does not combine with WAVELETS"):
        prox_regul(_self(), x, dict(method="LLT_ROF_WAVELETS", regul_param=0.5, regul_param2=0.2, iterations=3, time_marching_step=0.01))
    with pytest.raises(ValueError, match="unknown regularisation method 'WAVELETS'"):
        prox_regul(_self(), x, dict(method="WAVELETS", regul_param=0.5, iterations=3))
    # one rank of a one-rank world: the slab driver, then the shrinkage of the rank's own planes
    reg = dict(KIND_REG["NDF"], method="NDF_WAVELETS", regul_param2=T)
    reserve_prox_scratch(_self(), shape, reg)
    whole = host(prox_regul(_self(), x, dict(reg)))
    same_bits(host(prox_regul(_self(S.SlabComm(0, 1)), x, dict(reg))), whole, "slab mode")
    # TGV on a slab rank: its one usable case, the singleton-axis volume
    reg = dict(KIND_REG["TGV"], method="TGV_WAVELETS", regul_param2=T)
    flat = x[:1].contiguous()
    same_bits(host(prox_regul(_self(S.SlabComm(0, 1)), flat, dict(reg))), host(prox_regul(_self(), flat, dict(reg))), "TGV")
    with pytest.raises(ValueError, match="TGV is not available in z-slab mode"):
        prox_regul(_self(S.SlabComm(0, 1)), x, dict(reg))


# -------------------------------------------------------------------------------------------------- drivers
NZ, NN, NA = 16, 32, 40
ANGLES = np.linspace(0, np.pi, NA, endpoint=False)
REG = dict(method="PD_TV_WAVELETS", regul_param=0.002, regul_param2=0.004, iterations=8, PD_LipschitzConstant=8.0)


def _rt(os_number):
    from tomobar_amd.methodsIR_CuPy import RecToolsIRCuPy
    return RecToolsIRCuPy(NN, 0, NZ, 0.0, ANGLES, NN, 0, os_number)


def _data():
    sino = torch.from_numpy(np.random.default_rng(11).random((NZ, NA, NN)).astype(np.float32)).cuda()
    return {"projection_data": sino, "data_axes_labels_order": ["detY", "angles", "detX"]}


@pytest.mark.parametrize("driver", ["FISTA", "ADMM", "OSEM"])
def test_drivers_equal_the_prox_composed_by_hand(driver, monkeypatch):
    """two outer iterations of three subsets with PD_TV_WAVELETS against the same driver whose prox is put together here:
    prox_regul with plain PD_TV, a stand-alone shrinkage of the same X, the average by torch"""
    import tomobar_amd.methodsIR_CuPy as IR
    from tomobar_amd import ops
    algo = {"iterations": 2}
    rho = 2.0
    if driver != "OSEM":
        algo["lipschitz_const"] = 3000.0
    if driver == "ADMM":
        algo["ADMM_rho_const"] = rho
    reg = dict(REG)
    got = host(getattr(_rt(3), driver)(_data(), dict(algo), reg))
    assert {k: reg[k] for k in REG} == REG, "the caller's values were rewritten"

    real, seen = IR.prox_regul, []

    def by_hand(self, X, r, out=None):
        seen.append(r["regul_param2"])
        res = real(self, X, dict(r, method="PD_TV"), out=out)
        w = ops.wavelet_shrink(ops.contiguous(X), np.float32(r["regul_param2"]))
        res.copy_((res + w) * 0.5)
        return res

    monkeypatch.setattr(IR, "prox_regul", by_hand)
    hand = host(getattr(_rt(3), driver)(_data(), dict(algo), dict(REG)))
    assert len(seen) >= 2 and seen == [REG["regul_param2"] / (rho if driver == "ADMM" else 1.0)] * len(seen)
    same_bits(got, hand, driver)
    monkeypatch.setattr(IR, "prox_regul", real)
    plain = host(getattr(_rt(3), driver)(_data(), dict(algo), dict(REG, method="PD_TV")))
    assert np.all(np.isfinite(got)) and not np.array_equal(got, plain)
