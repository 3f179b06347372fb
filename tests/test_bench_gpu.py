"""A plain bench.py run (no --full) on the GPU: the headline line only, --steps timed steps, and --dump-outputs writing the frame and its ray
classes of the last timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(gpu, tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 7 and line["warmup"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "Mrays/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert "roofline" not in line and "cpu_baseline" not in line and "secondary" not in line
    img = np.load(tmp_path / "image.npy")
    rays = np.load(tmp_path / "rays_per_frame.npy")
    assert img.dtype == np.float32 and img.shape == (1080, 1920, 3) and np.isfinite(img).all() and img.max() > 0
    assert rays.dtype == np.float64 and rays[0] == line["config"]["rays_per_frame"]["total"]
