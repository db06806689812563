"""Multi-process (gloo, CPU) tests of the LLT_ROF z-slab driver tomobar_amd.slab.llt_rof_slab: the suite of
tests/_march_gloo_suite.py -- the driver with the oracle's single-iteration function as the compute step against the oracle's
whole-volume result, bit for bit -- collected for LLT_ROF."""
import os
import sys

import pytest

pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _march_gloo_suite  # noqa: E402

globals().update(_march_gloo_suite.suite("LLT_ROF"))
