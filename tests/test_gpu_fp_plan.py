"""The forward projector's kernel choice, pinned exactly: for every case of tests/golden/make_fp_plan_paths.py the kernel
path string of a forward projection and of an LS residual, and the SHA-256 of both outputs, must match the recording in
tests/golden/fp_plan_paths.json (variant 0: shipped library; the A/B variants: dev flavour)."""
import importlib.util
import json
import os

import pytest

pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _generator():
    spec = importlib.util.spec_from_file_location("make_fp_plan_paths", os.path.join(HERE, "golden", "make_fp_plan_paths.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _generator()
PARAMS = [pytest.param(case, v, id=f"{case[0]}-v{v}", marks=() if v == 0 else pytest.mark.dev_variants)
          for case in G.CASES for v in case[-1]]


@pytest.fixture(scope="module")
def recorded():
    with open(G.FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("case,variant", PARAMS)
def test_fp_plan_reproduces_recorded_paths_and_outputs(recorded, case, variant):
    got = G.record(case, variant)
    want = {k: recorded[k] for k in (G.key(case, variant, s) for s in G.subsets(case))}
    assert got == want
