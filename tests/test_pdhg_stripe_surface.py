"""No GPU: the surface of PDHG's stripe variable (``_data_["stripe_lambda"]``; docs/kernels/pdhg.md).  The two entry points are
declared in include/tomo_mi355x.h and bound through ``_lib.SIGNATURES`` like every other; this file checks what is their own --
both declared, bound and exported by both libraries with the stated types, the segment length in step across header, binding
and oracle --, the refusals of the C-ABI, the key in all eight drivers, and that without the key ``RecToolsIRCuPy.PDHG`` makes
the calls it always made.  Their streams are held by tests/test_gpu_streams.py (case "pdhg_stripe")."""
import ctypes as C
import os
import re
import sys
import types

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import _pdhg_call_log as CALLS  # noqa: E402
import _pdhg_stripe_oracle as S  # noqa: E402,F401  (the restatement imports without a GPU)
from test_stream_coverage import header_prototypes  # noqa: E402  (the header's parser; read, not collected from here)

HEADER = ("include", "tomo_mi355x.h")
NAMES = {"tomo_pdhg_sino_dual_stripe": (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 4 + [C.c_float, C.c_void_p]),
         "tomo_pdhg_stripe_update": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_float, C.c_float, C.c_void_p])}
DRIVERS = ("PDHG", "SPDHG", "FISTA", "ADMM", "OSEM", "SIRT", "CGLS", "Landweber")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as fh:
        return fh.read()


# ------------------------------------------------------------------------------------------------ the header and the binding
def test_the_header_declares_what_the_binding_binds_and_both_libraries_export_it():
    from tomobar_amd import _lib
    main = _read(*HEADER)
    declared = set(re.findall(r"\b(tomo_[a-z0-9_]+)\s*\(", main))      # comments included, as tests/test_host_logic.py reads
    protos = header_prototypes()
    assert set(NAMES) <= declared and set(NAMES) <= set(protos) and set(NAMES) <= set(_lib.SIGNATURES)
    for flavour in ("shipped", "dev"):
        with _lib.use_flavour(flavour) as handle:
            for name, (res, args) in NAMES.items():
                assert hasattr(handle, name), f"{name} declared in {'/'.join(HEADER)} but not exported ({flavour})"
                fn = getattr(handle, name)
                assert fn.restype is res and list(fn.argtypes) == list(args)
                assert _lib.SIGNATURES[name][0] is res and list(_lib.SIGNATURES[name][1]) == list(args)
    for name in NAMES:      # one ctypes argument per parameter, pointers as void pointers
        kinds = [C.c_void_p if "*" in p else {"int": C.c_int, "float": C.c_float}[p.split()[0]] for p in protos[name].split(",")]
        assert kinds == list(_lib.SIGNATURES[name][1]), name
    assert re.search(r"#define\s+TOMO_ABI_VERSION\s+10\b", main) and _lib.ABI_VERSION == 10
    seg = int(re.search(r"#define\s+TOMO_PDHG_STRIPE_SEG\s+(\d+)", main).group(1))
    assert seg == _lib.PDHG_STRIPE_SEG == S.SEG == 64
    doc = " ".join(_read("INTEGRATION.md").split())
    assert all(f"`{n}`" in doc for n in NAMES)


def test_a_library_without_the_new_symbols_is_stale(monkeypatch):
    from tomobar_amd import _lib
    monkeypatch.setitem(_lib.SIGNATURES, "tomo_pdhg_no_such_entry", (C.c_int, []))
    with pytest.raises(ImportError, match="stale.*tomo_pdhg_no_such_entry"):
        _lib._load("shipped")


def test_the_new_source_is_built_into_both_libraries():
    make = _read("tomobar_amd", "csrc", "Makefile")
    assert re.search(r"^SRCS\s*:=.*\bpdhg_stripe\.hip\b", make, flags=re.M)
    src = _read("tomobar_amd", "csrc", "pdhg_stripe.hip")
    assert '#include "tomo_common.h"' in src and "__global__" in src      # tomo_common.h includes the public header
    assert '#include "tomo_mi355x.h"' in _read("tomobar_amd", "csrc", "tomo_common.h")


# ------------------------------------------------------------------------------------------------ C-ABI
def test_invalid_arguments_are_refused_before_the_device_is_touched():
    from tomobar_amd import _lib
    lib = _lib.lib()
    p = [C.c_void_p(0x1000 * k) for k in range(1, 9)]   # never dereferenced: every case fails validation
    nul = C.c_void_p(0)

    def dual(y=p[0], r=p[1], b=p[2], sg=nul, sbar=p[4], part=p[5], nz=2, na=70, nu=8, fid=0, sigma=0.25):
        return lib.tomo_pdhg_sino_dual_stripe(y, r, b, sg, sbar, part, nz, na, nu, fid, sigma, None)

    def update(s=p[0], sbar=p[1], part=p[2], nz=2, na=70, nu=8, tau_s=0.1, theta=0.3):
        return lib.tomo_pdhg_stripe_update(s, sbar, part, nz, na, nu, tau_s, theta, None)

    bad = [(dual, dict(fid=3)), (dual, dict(fid=-1)), (dual, dict(nz=0)), (dual, dict(na=0)), (dual, dict(nu=-4)),
           (dual, dict(sigma=0.0)), (dual, dict(sigma=-0.5)), (dual, dict(sigma=float("nan"))), (dual, dict(sigma=float("inf"))),
           (dual, dict(y=nul)), (dual, dict(r=nul)), (dual, dict(b=nul)), (dual, dict(sbar=nul)), (dual, dict(part=nul)),
           (dual, dict(r=p[0])), (dual, dict(b=p[0])), (dual, dict(sg=p[0])), (dual, dict(sbar=p[0])), (dual, dict(part=p[0])),
           (dual, dict(part=p[1])), (dual, dict(part=p[2])), (dual, dict(sg=p[3], part=p[3])), (dual, dict(part=p[4])),
           (update, dict(nz=0)), (update, dict(na=0)), (update, dict(nu=0)), (update, dict(tau_s=0.0)), (update, dict(tau_s=float("nan"))),
           (update, dict(theta=-1.0)), (update, dict(theta=float("inf"))), (update, dict(s=nul)), (update, dict(sbar=nul)),
           (update, dict(part=nul)), (update, dict(sbar=p[0])), (update, dict(part=p[0])), (update, dict(part=p[1]))]
    for fn, kw in bad:
        assert fn(**kw) == _lib.E_INVALID, (fn.__name__, kw)
        with pytest.raises(ValueError):
            _lib.check(fn(**kw))
    assert update(theta=-1.0) == _lib.E_INVALID and "theta" in lib.tomo_last_error().decode()


# ------------------------------------------------------------------------------------------------ the key
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
        return dicts_check(me or _self(OS_number=4 if method_run == "SPDHG" else 1), d, algo, reg, method_run=method_run)
    finally:
        ops.to_device = keep


@pytest.mark.parametrize("method_run", DRIVERS)
def test_the_key_is_read_and_never_filled(method_run):
    assert "stripe_lambda" not in _dicts(method_run=method_run)[0]
    d = _dicts(data={"stripe_lambda": None}, method_run=method_run)[0]
    assert d["stripe_lambda"] is None


@pytest.mark.parametrize("fidelity", ["LS", "L1", "KL"])
@pytest.mark.parametrize("reg", [None, {"method": "PD_TV"}, {"method": "PD_TGV"}], ids=["none", "PD_TV", "PD_TGV"])
@pytest.mark.parametrize("algo", [{}, {"PDHG_preconditioner": "diagonal"}, {"nonnegativity": True}], ids=["scalar", "diagonal", "nonneg"])
def test_pdhg_takes_the_key_with_every_term_regulariser_and_step_rule(fidelity, reg, algo):
    d, a, r = _dicts(data={"stripe_lambda": 2.5, "data_fidelity": fidelity}, algo=dict(algo), reg=reg and dict(reg))
    assert d["stripe_lambda"] == 2.5


@pytest.mark.parametrize("value", [0, 0.0, -1.0, float("nan")])
def test_a_weight_that_is_not_positive_is_refused(value):
    with pytest.raises(ValueError, match=r"stripe_lambda.*must be positive"):
        _dicts(data={"stripe_lambda": value})


@pytest.mark.parametrize("method_run", [m for m in DRIVERS if m != "PDHG"])
def test_every_other_driver_refuses_the_key(method_run):
    with pytest.raises(ValueError, match=r"^_data_\['stripe_lambda'\] is available in PDHG only$"):
        _dicts(data={"stripe_lambda": 1.0}, method_run=method_run)


def test_the_existing_refusals_keep_their_words():
    for key in ("ringGH_lambda", "huber_threshold", "studentst_threshold"):
        with pytest.raises(ValueError, match=re.escape(f"_data_['{key}'] is available in FISTA only (PDHG: the 'L1' data fidelity is the robust term)")):
            _dicts(data={"stripe_lambda": 1.0, key: 0.5})
    with pytest.raises(ValueError, match="PDHG supports the 'LS', 'KL' and 'L1' data fidelities, not 'PWLS'"):
        _dicts(data={"stripe_lambda": 1.0, "data_fidelity": "PWLS"})
    with pytest.raises(ValueError, match="PDHG is not available in z-slab mode"):
        _dicts(data={"stripe_lambda": 1.0}, me=_self(slab=object()))


# ------------------------------------------------------------------------------------------------ the driver's calls
VOL, SINO = CALLS.VOL, CALLS.SINO
STRIPE_OPS = ("pdhg_sino_dual_stripe", "pdhg_stripe_update")


@pytest.fixture
def driver(monkeypatch):
    """a RecToolsIRCuPy whose projector and launches are recorders on CPU tensors: (the object, the log of calls); fills are
    logged with their shapes and the step builder with the number of its arguments"""
    from tomobar_amd import ops
    rt, log = CALLS.recording_driver(monkeypatch, fill_shape=True, more_ops=STRIPE_OPS)
    monkeypatch.setattr(ops, "pdhg_diag_steps", lambda *args: log.append(f"pdhg_diag_steps {len(args)}"))
    return rt, log


def _data(**kw):
    import torch
    return dict({"projection_data": torch.zeros(SINO, dtype=torch.float32)}, **kw)


def _fill(value, shape):
    return f"fill {float(value)} {tuple(shape)}"


# what the parent's driver does: x0 = 0, the work arrays, q = 0 three times, y = 0, the layouts; five launches per iteration
SET_UP = [_fill(0, VOL), "pdhg_work_arrays"] + 3 * [_fill(0, VOL)] + [_fill(0, SINO)]
LAYOUTS = ["A.invalidate", "A.set_residual_layout planar", "A.set_volume_layout planar"]
TEAR_DOWN = ["A.set_residual_layout planar", "A.set_volume_layout planar", "A.invalidate"]
LOOP = ["A.forward", "pdhg_sino_dual", "A.backward", "pdhg_tv_dual", "pdhg_primal"]
DIAG_STEPS = [_fill(1, VOL), "A.forward", "pdhg_diag_steps 3", _fill(1, SINO), "A.backward", "pdhg_diag_steps 4"]
DIAG_LOOP = ["A.forward", "pdhg_sino_dual_diag", "A.backward", "pdhg_tv_dual", "pdhg_primal_diag"]


@pytest.mark.parametrize("more", [{}, {"stripe_lambda": None}], ids=["absent", "None"])
def test_without_the_key_the_driver_makes_the_calls_of_the_parent(driver, more):
    rt, log = driver
    rt.PDHG(_data(**more), dict(iterations=2, lipschitz_const=50.0, recon_mask_radius=None), {"method": "PD_TV"})
    assert log == SET_UP + LAYOUTS + 2 * LOOP + TEAR_DOWN
    assert "stripes" not in rt.last_run and not set(STRIPE_OPS) & set(log)
    del log[:]
    rt.PDHG(_data(**more), dict(iterations=2, PDHG_preconditioner="diagonal", recon_mask_radius=None), {"method": "PD_TV"})
    assert log == [c + " tau" if c == "pdhg_work_arrays" else c for c in SET_UP] + LAYOUTS + DIAG_STEPS + 2 * DIAG_LOOP + TEAR_DOWN
    assert "stripes" not in rt.last_run


def test_with_the_key_the_stripe_launches_take_the_place_of_step_2(driver):
    """s, s-bar and the partial sums are zero-filled once, before the loop; step 2 is the fused launch, step 6 follows it; the
    other launches stay; with the diagonal steps the row sums gain the 1 of S (a fourth argument of the step builder)"""
    rt, log = driver
    stripes = [_fill(0, (SINO[0], SINO[2]))] * 2 + [_fill(0, (1, SINO[0], SINO[2]))]
    loop = ["A.forward", *STRIPE_OPS, "A.backward", "pdhg_tv_dual", "pdhg_primal"]
    rt.PDHG(_data(stripe_lambda=2.0), dict(iterations=2, lipschitz_const=50.0, recon_mask_radius=None), {"method": "PD_TV"})
    assert log == SET_UP + stripes + LAYOUTS + 2 * loop + TEAR_DOWN
    assert tuple(rt.last_run["stripes"].shape) == (SINO[0], SINO[2])
    del log[:]
    rt.PDHG(_data(stripe_lambda=2.0), dict(iterations=2, PDHG_preconditioner="diagonal", recon_mask_radius=None), None)
    set_up = [c + " tau" if c == "pdhg_work_arrays" else c for c in SET_UP]
    del set_up[2:5]       # no TV block: no q
    steps = [c.replace("pdhg_diag_steps 3", "pdhg_diag_steps 4") for c in DIAG_STEPS]
    loop = ["A.forward", *STRIPE_OPS, "A.backward", "pdhg_primal_diag"]
    assert log == set_up + stripes + LAYOUTS + steps + 2 * loop + TEAR_DOWN
