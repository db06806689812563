"""MI355X tests of the Diff4th regulariser: the suite of tests/_march_gpu_suite.py -- the shipped kernel against the float32
numpy restatement tests/_diff4th_oracle.py, bit for bit (docs/kernels/diff4th.md) -- collected for Diff4th."""
import os
import sys

import pytest

pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _march_gpu_suite  # noqa: E402

globals().update(_march_gpu_suite.suite("Diff4th"))
