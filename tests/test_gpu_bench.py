"""A plain ``bench.py`` run on one GPU (``-m gpu``): the lean headline line and ``--dump-outputs``.

The line names its figure and the time of one timed step, times exactly ``--steps`` steps, and carries none of what
``--full`` adds. The dumped arrays are the last timed step's per-atom energies and dE/dR, finite, and sum to the
energy the line reports.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCHER_VARS = ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in LAUNCHER_VARS}   # a plain command, not a rank of a launch
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--boxes", "1", "--dump-outputs", str(tmp_path)],
                         capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["metric"] == "atom-steps/sec (energy+forces) PET 10k-atom box"
    assert line["unit"] == "atom-steps/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["steps"] == 3 and line["warmup"] == 1
    assert line["ms_per_step"] > 0 and line["value"] > 0
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 - 10000) < 1e-6 * 10000   # one 10 000-atom box per step
    for extra in ("roofline", "host_resident_inputs", "box1000", "train64x1000", "soap100k", "cpu_baseline"):
        assert extra not in line, extra

    a = np.load(tmp_path / "atomic_energy.npy")
    g = np.load(tmp_path / "positions_gradient.npy")
    e = np.load(tmp_path / "box_energy.npy")
    assert a.shape == (10000,) and a.dtype == np.float32
    assert g.shape == (10000, 3) and g.dtype == np.float32
    assert e.shape == (1,) and e.dtype == np.float64
    assert np.isfinite(a).all() and np.isfinite(g).all() and np.abs(g).max() > 0
    assert abs(e[0] - line["config"]["total_energy_rank0"]) <= 1e-9 * abs(e[0])
