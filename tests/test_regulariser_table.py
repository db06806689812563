"""The one table of regularisers (tomobar_amd/supp/regularisers.py) and everything that reads it: which method a
``_regularisation_["method"]`` string means, what prox_regul then calls with which arguments in whole-volume and in z-slab
mode, which scratch arena reserve_prox_scratch asks for, which keys dicts_check fills.  No GPU: the functions the
dispatch ends in are replaced by recorders.  The expected calls are written out literally (copied from the if-chains the
table replaced), so the dispatch, scratch and dicts tests state the behaviour independently of the table."""
import itertools
import math
import types

import pytest
import torch

ORDER = ("ROF_TV", "PD_TV", "TGV", "NDF", "Diff4th", "LLT_ROF")   # the precedence: the first name found in the string wins
METHODS = list(ORDER) + [f"{a}_{b}" for a, b in itertools.permutations(ORDER, 2)]
NEITHER = (None, "FGP_TV", 123)
UNKNOWN = "unknown regularisation method 'FGP_TV': ROF_TV, PD_TV and TGV are supported, as are NDF, Diff4th and LLT_ROF"


def expected(method):
    return next((k for k in ORDER if k in method), None) if isinstance(method, str) else None


def test_method_strings():
    assert len(METHODS) == 36 and len(set(METHODS)) == 36
    assert [expected(m) for m in ORDER] == list(ORDER) and all(expected(m) is None for m in NEITHER)
    assert expected("NDF_TGV") == "TGV" and expected("LLT_ROF_PD_TV") == "PD_TV" and expected("LLT_ROF_Diff4th") == "Diff4th"


# ------------------------------------------------------------------------------------------------ 1. precedence
def test_kind_of_is_the_first_name_of_the_precedence_tuple_in_the_string():
    from tomobar_amd.supp import regularisers as T
    assert tuple(k.name for k in T.KINDS) == ORDER
    for method in METHODS:
        assert T.kind_of(method).name == expected(method), method
    for method in NEITHER:
        assert T.kind_of(method) is None, method


def test_table_module_imports_neither_torch_nor_ops():
    import pathlib
    import subprocess
    import sys
    code = ("import sys; import tomobar_amd.supp.regularisers, tomobar_amd; "
            "assert 'torch' not in sys.modules and 'tomobar_amd.ops' not in sys.modules")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=str(pathlib.Path(__file__).parents[1]))


# ------------------------------------------------------------------------------------------------ 2. dispatch
# the dictionary of the dispatch tests, without and with the optional keys
REG = dict(regul_param=0.11, iterations=7, time_marching_step=0.22, methodTV=1, PD_LipschitzConstant=9.5, tolerance=0.001)
OPTIONAL = dict(edge_threshold=0.33, NDF_penalty="PM", regul_param2=0.44, TGV_alpha1=0.55, TGV_alpha2=0.66,
                half_precision=True)
# name -> (function in regularisersCuPy, driver in slab, positional arguments after the array (slab: and the communicator)
# with REG alone, the same with REG + OPTIONAL); self.nonneg_regul = 1, the device index (whole volume only) = 0
WHOLE = {
    "ROF_TV": ("ROF_TV_cupy", (0.11, 7, 0.22, 0, False), (0.11, 7, 0.22, 0, True)),
    "PD_TV": ("PD_TV_cupy", (0.11, 7, 1, 1, 9.5, 0, False), (0.11, 7, 1, 1, 9.5, 0, True)),
    "TGV": ("TGV_cupy", (0.11, 7, 1.0, 2.0, 9.5, 0), (0.11, 7, 0.55, 0.66, 9.5, 0)),
    "NDF": ("NDF_cupy", (0.11, 0.01, 7, 0.22, "Huber", 0), (0.11, 0.33, 7, 0.22, "PM", 0)),
    "Diff4th": ("Diff4th_cupy", (0.11, 0.01, 7, 0.22, 0), (0.11, 0.33, 7, 0.22, 0)),
    "LLT_ROF": ("LLT_ROF_cupy", (0.11, 0.001, 7, 0.22, 0), (0.11, 0.44, 7, 0.22, 0)),
}
SLAB = {
    "ROF_TV": ("rof_tv_slab", (0.11, 7, 0.22, False), (0.11, 7, 0.22, True)),
    "PD_TV": ("pd_tv_slab", (0.11, 7, 1, 1, 9.5, False), (0.11, 7, 1, 1, 9.5, True)),
    "NDF": ("ndf_slab", (0.11, 0.01, 7, 0.22, "Huber"), (0.11, 0.33, 7, 0.22, "PM")),
    "Diff4th": ("diff4th_slab", (0.11, 0.01, 7, 0.22), (0.11, 0.33, 7, 0.22)),
    "LLT_ROF": ("llt_rof_slab", (0.11, 0.001, 7, 0.22), (0.11, 0.44, 7, 0.22)),
}
NO_HALF = ("TGV", "NDF", "Diff4th", "LLT_ROF")


def _self(slab=None):
    return types.SimpleNamespace(nonneg_regul=1, Atools=types.SimpleNamespace(device_index=0), slab=slab)


@pytest.fixture
def calls(monkeypatch):
    """every function prox_regul can end in, replaced by a recorder: (name, args, kwargs) per call; a slab driver reports
    that it stopped after 5 iterations at a relative change of 0.25"""
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

    for name, _, _ in WHOLE.values():
        monkeypatch.setattr(R, name, recorder(name, False))
    for name, _, _ in SLAB.values():
        monkeypatch.setattr(S, name, recorder(name, True))
    return log


def _same(got, want):
    """equal, with the types equal too (False is not 0, 1 is not 1.0)"""
    return tuple(got) == tuple(want) and [type(v) for v in got] == [type(v) for v in want]


def _reg(method, optional, name):
    reg = dict(REG, method=method, **(OPTIONAL if optional else {}))
    if optional and name in NO_HALF:
        del reg["half_precision"]
    return reg


@pytest.mark.parametrize("optional", [False, True], ids=["defaults", "optional_keys"])
@pytest.mark.parametrize("shape, slab", [((4, 5, 6), False), ((1, 5, 6), True)], ids=["whole_volume", "singleton_axis_with_slab"])
def test_prox_regul_whole_volume_calls(calls, shape, slab, optional):
    """without a slab, and on a slab rank whose volume has a singleton axis (TGV included): the *_cupy function"""
    from tomobar_amd import regularisersCuPy as R
    X, out = torch.zeros(shape), torch.zeros(shape)
    comm = object() if slab else None
    for method in METHODS:
        del calls[:]
        fn, plain, full = WHOLE[expected(method)]
        assert R.prox_regul(_self(comm), X, _reg(method, optional, expected(method)), out=out) == fn, method
        (name, args, kwargs), = calls
        assert name == fn and args[0] is X and _same(args[1:], full if optional else plain), (method, args)
        assert set(kwargs) == {"out", "tolerance"} and kwargs["out"] is out and kwargs["tolerance"] == 0.001, (method, kwargs)


@pytest.mark.parametrize("optional", [False, True], ids=["defaults", "optional_keys"])
def test_prox_regul_slab_calls(calls, optional, monkeypatch):
    """a real 3D volume on a slab rank: the slab driver, its `info` recorded for last_prox; TGV refuses"""
    from tomobar_amd import regularisersCuPy as R
    X, out, comm = torch.zeros((4, 5, 6)), torch.zeros((4, 5, 6)), object()
    for method in METHODS:
        del calls[:]
        reg = _reg(method, optional, expected(method))
        if expected(method) == "TGV":
            with pytest.raises(ValueError) as e:
                R.prox_regul(_self(comm), X, reg, out=out)
            assert str(e.value) == "TGV is not available in z-slab mode" and calls == []
            with pytest.raises(ValueError) as e:
                R.check_prox_available(_self(comm), X.shape, reg)
            assert str(e.value) == "TGV is not available in z-slab mode"
            continue
        fn, plain, full = SLAB[expected(method)]
        R._record(-1, -1.0)
        assert R.prox_regul(_self(comm), X, reg, out=out) == fn, method
        (name, args, kwargs), = calls
        assert name == fn and args[0] is X and args[1] is comm and _same(args[2:], full if optional else plain), (method, args)
        assert set(kwargs) == {"out", "tolerance", "info"} and kwargs["out"] is out and kwargs["tolerance"] == 0.001
        assert R.last_prox() == (5, 0.25), method
    # what the driver is handed as `info`: all iterations done, no relative change evaluated
    seen = {}
    from tomobar_amd import slab as S
    monkeypatch.setattr(S, "ndf_slab", lambda *a, info, **kw: seen.update(info))
    R.prox_regul(_self(comm), X, dict(REG, method="NDF"))
    assert set(seen) == {"iterations_done", "rel_change"} and seen["iterations_done"] == 7 and math.isnan(seen["rel_change"])


@pytest.mark.parametrize("slab", [False, True], ids=["whole_volume", "slab"])
def test_prox_regul_refusals(calls, slab):
    from tomobar_amd import regularisersCuPy as R
    X, comm = torch.zeros((4, 5, 6)), object() if slab else None
    for name in NO_HALF:
        for method in (name, f"LLT_ROF_{name}", f"{name}_LLT_ROF"):
            if expected(method) != name:
                continue
            with pytest.raises(ValueError) as e:
                R.prox_regul(_self(comm), X, dict(REG, method=method, half_precision=True))
            assert str(e.value) == f"{name} does not support half_precision=True", method
    with pytest.raises(ValueError) as e:
        R.prox_regul(_self(comm), X, dict(REG, method="FGP_TV"))
    assert str(e.value) == UNKNOWN
    assert calls == []


# ------------------------------------------------------------------------------------------------ 3. scratch
@pytest.fixture
def reserved(monkeypatch):
    from tomobar_amd import regularisersCuPy as R
    log = []
    monkeypatch.setattr(R, "ops", types.SimpleNamespace(reserve_tv_scratch=lambda *args: log.append(args)))
    return log


@pytest.mark.parametrize("shape, passed", [((8, 9, 10), (8, 9, 10)), ((1, 9, 10), (9, 10)), ((8, 1, 10), (8, 10)), ((9, 10), (9, 10))],
                         ids=lambda v: "x".join(map(str, v)))
def test_reserve_prox_scratch_passes_shape_device_kind_half(reserved, shape, passed):
    from tomobar_amd import regularisersCuPy as R
    for method in METHODS:
        name = expected(method)
        for half in (False, True):
            del reserved[:]
            reg = {"method": method, "half_precision": half} if half else {"method": method}
            if half and name in NO_HALF:
                with pytest.raises(ValueError) as e:
                    R.reserve_prox_scratch(_self(), shape, reg)
                assert str(e.value) == f"{name} does not support half_precision=True" and reserved == []
                continue
            R.reserve_prox_scratch(_self(), shape, reg)
            (args,), want = reserved, (passed, "cuda:0", name, half)
            assert _same(args, want) and _same(args[0], passed), (method, half, args)


def test_reserve_prox_scratch_does_nothing_with_a_slab_or_without_a_method(reserved):
    from tomobar_amd import regularisersCuPy as R
    for method in METHODS:
        for shape in ((8, 9, 10), (1, 9, 10), (9, 10)):
            if expected(method) == "TGV" and shape == (8, 9, 10):
                with pytest.raises(ValueError, match="TGV is not available in z-slab mode"):
                    R.reserve_prox_scratch(_self(object()), shape, {"method": method})
            else:
                R.reserve_prox_scratch(_self(object()), shape, {"method": method})
    for comm in (None, object()):
        R.reserve_prox_scratch(_self(comm), (8, 9, 10), {"method": None})
        R.reserve_prox_scratch(_self(comm), (8, 9, 10), {})
        R.reserve_prox_scratch(_self(comm), (8, 9, 10), {"method": "FGP_TV"})
    assert reserved == []


# ------------------------------------------------------------------------------------------------ dicts_check
# name -> the keys dicts_check adds for it and their defaults; nothing for the two TV methods
EXTRA_KEYS = {"ROF_TV": {}, "PD_TV": {}, "TGV": {"TGV_alpha1": 1.0, "TGV_alpha2": 2.0},
              "NDF": {"NDF_penalty": "Huber", "edge_threshold": 0.01}, "Diff4th": {"edge_threshold": 0.01},
              "LLT_ROF": {"regul_param2": 0.001}}


def test_dicts_check_fills_the_keys_of_the_method_prox_regul_runs(monkeypatch):
    from tomobar_amd import ops
    from tomobar_amd.supp.dicts import dicts_check
    monkeypatch.setattr(ops, "to_device", lambda x, index: x)   # no GPU here: the projections stay where they are
    me = types.SimpleNamespace(Atools=types.SimpleNamespace(device_index=0), OS_number=1)

    def run(reg):
        return dicts_check(me, {"projection_data": torch.zeros((2, 3, 4))}, {}, reg, method_run="FISTA")[2]

    plain = set(run({"method": "ROF_TV"}))
    for method in METHODS:
        got = run({"method": method})
        want = EXTRA_KEYS[expected(method)]
        assert set(got) - plain == set(want) and all(got[k] == v for k, v in want.items()), method
        for key, value in want.items():   # every added key is checked: NDF_penalty against its names, the others for > 0
            with pytest.raises(ValueError) as e:
                run({"method": method, key: 0.0})
            assert str(e.value) == (f"_regularisation_['{key}'] must be 'Huber', 'PM' or 'Tukey'" if key == "NDF_penalty"
                                    else f"_regularisation_['{key}'] must be positive"), (method, key)
    # NDF: the penalty is checked before the threshold
    with pytest.raises(ValueError, match="NDF_penalty"):
        run({"method": "NDF", "NDF_penalty": "TV", "edge_threshold": -1.0})
    for method in NEITHER:
        assert set(run({"method": method, "edge_threshold": -1.0})) - plain == {"edge_threshold"}


# ------------------------------------------------------------------------------------------------ 4. table consistency
def test_table_names_exist_and_agree_with_slab_and_the_signatures():
    from tomobar_amd import _lib
    from tomobar_amd import regularisersCuPy as R
    from tomobar_amd import slab as S
    from tomobar_amd.supp import regularisers as T
    for k in T.KINDS:
        assert k.scratch in _lib.SIGNATURES and callable(getattr(R, k.cupy)), k.name
        assert len(_lib.SIGNATURES[k.scratch][1]) == (5 if k.scratch_half else 4), k.name
        assert (k.slab is None) == (k.slot is None) and (k.slab is None or callable(getattr(S, k.slab))), k.name
        assert (k.entry is None) == (k.ghost is None) and (k.entry is None or k.entry in _lib.SIGNATURES), k.name
        assert k.cupy == WHOLE[k.name][0] and k.slab == SLAB.get(k.name, (None,))[0]
        assert k.half == (k.name not in NO_HALF)
        assert {key: value for key, value, _ in k.defaults} == EXTRA_KEYS[k.name]
    assert T.BY_NAME == {k.name: k for k in T.KINDS}
    slots = {k.name: k.slot for k in T.KINDS if k.slot is not None}
    assert len(set(slots.values())) == len(slots) == 5
    assert slots == {"PD_TV": S.PLACED_SLOT_PD, "ROF_TV": S.PLACED_SLOT_ROF, "NDF": S.PLACED_SLOT_NDF,
                     "Diff4th": S.PLACED_SLOT_DIFF4TH, "LLT_ROF": S.PLACED_SLOT_LLT_ROF}
    ghosts = {k.name: k.ghost for k in T.KINDS if k.ghost is not None}
    assert ghosts == {"NDF": 1, "Diff4th": S.DIFF4TH_GHOST, "LLT_ROF": S.LLT_ROF_GHOST}
