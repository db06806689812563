"""bench.py end to end at a tiny shape: a plain run prints the headline only (no event profile, rooflines, CPU baseline or
halo statistics) and --dump-outputs writes what the timed call returned; --full adds the other legs; with two ranks
(sharing the one GPU: gloo, "oversubscribed") every rank dumps its own slab."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = ["--n", "192", "--nz", "24", "--angles", "96", "--os", "4", "--inner", "6", "--steps", "1", "--warmup", "1"]
FULL_ONLY = ("roofline", "kernels", "roofline_bp", "roofline_fp", "cpu_baseline", "halo", "north_star")


def _run(*extra, timeout=600):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "TOMO_BENCH_ARGV", "TOMO_BENCH_CHILD", "BENCH_CONFIG", "BENCH_STRONG",
              "BENCH_NORTH_STAR", "BENCH_NORTH_STAR_TEST", "BENCH_LIVE_PMC"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py")] + TINY + list(extra)
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_is_the_headline_and_dumps_the_reconstruction(tmp_path):
    line = _run("--gpus", "1", "--dump-outputs", str(tmp_path))
    assert line["steps"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0 and line["config"]["output_finite"]
    assert not [k for k in FULL_ONLY if k in line], line.keys()
    assert line["dumped_outputs"] == [{"rank": 0, "z_range": [0, 24], "files": ["recon"]}]
    rec = np.load(tmp_path / "recon.npy")
    assert rec.shape == (24, 192, 192) and rec.dtype == np.float32 and np.isfinite(rec).all() and rec.max() > 0


def test_full_run_adds_the_other_legs():
    line = _run("--gpus", "1", "--full", "--no-pmc")
    for k in ("roofline", "kernels", "roofline_bp", "roofline_fp", "cpu_baseline"):
        assert k in line, k
    assert line["kernels"]["bp"]["launches"] > 0 and line["cpu_baseline"]["value"] > 0


def test_every_rank_dumps_its_slab(tmp_path):
    line = _run("--gpus", "2", "--dump-outputs", str(tmp_path))
    assert line["n_gpus"] == 2 and line["config"]["oversubscribed"] is True and "halo" not in line
    assert line["dumped_outputs"] == [{"rank": r, "z_range": [24 * r, 24 * (r + 1)], "files": [f"recon_rank{r}"]}
                                      for r in range(2)]
    for r in range(2):
        rec = np.load(tmp_path / f"recon_rank{r}.npy")
        assert rec.shape == (24, 192, 192) and rec.dtype == np.float32 and np.isfinite(rec).all() and rec.max() > 0
