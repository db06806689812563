"""MI355X tests of the LLT_ROF regulariser: the suite of tests/_march_gpu_suite.py -- the shipped kernel against the float32
numpy restatement tests/_llt_rof_oracle.py, bit for bit (docs/kernels/llt_rof.md) -- collected for LLT_ROF."""
import os
import sys

import pytest

pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _march_gpu_suite  # noqa: E402

globals().update(_march_gpu_suite.suite("LLT_ROF"))
