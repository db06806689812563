"""The host dispatch of the TV operators, pinned exactly: for every (operator, variant, dual type) of
tests/golden/make_tv_dispatch_digests.py the SHA-256 of every output must match the recording in
tests/golden/tv_dispatch_digests.json (variants 0 and 22: shipped library; the others: dev flavour).  The fixture was
recorded before pd_plan / pd_launch_one replaced the per-family dispatch functions; no tolerance applies."""
import importlib.util
import json
import os

import pytest

pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _generator():
    spec = importlib.util.spec_from_file_location("make_tv_dispatch_digests", os.path.join(HERE, "golden", "make_tv_dispatch_digests.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _generator()
PARAMS = [pytest.param(case, id=G.key(case).replace("/", "-"),
                       marks=() if case[1] in G.SHIPPED[case[0]] else pytest.mark.dev_variants) for case in G.CASES]


@pytest.fixture(scope="module")
def recorded():
    with open(G.FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("case", PARAMS)
def test_tv_dispatch_reproduces_recorded_outputs(recorded, case):
    got = G.record(case)
    want = recorded[G.key(case)]
    assert sorted(got) == sorted(want)
    assert {k: v for k, v in got.items() if want[k] != v} == {}
