"""MI355X tests of the NDF regulariser: the suite of tests/_march_gpu_suite.py -- the shipped kernel against the float32
numpy restatement tests/_ndf_oracle.py, bit for bit (docs/kernels/ndf.md) -- collected for NDF."""
import os
import sys

import pytest

pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _march_gpu_suite  # noqa: E402

globals().update(_march_gpu_suite.suite("NDF"))
