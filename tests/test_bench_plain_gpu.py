"""bench.py without --full (-m gpu): the run times the headline steps only, prints the contract keys, and --dump-outputs writes what
the last timed step computed -- the same files, bit for bit, in two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _bench(*flags):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *flags], capture_output=True, text=True, timeout=540,
                         env=env, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout
    return json.loads(lines[0])


@pytest.mark.timeout(600)
def test_plain_bench_run_dumps_the_last_steps_outputs(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    steps = 3
    lines = [_bench("--gpus", "1", "--steps", str(steps), "--warmup", "1", "--dump-outputs", str(tmp_path / d)) for d in ("a", "b")]
    for line in lines:
        assert line["steps"] == steps and line["full"] is False and line["higher_is_better"] is True
        assert line["unit"] == "rays/s" and line["dtype"].startswith("fp16x3") and "training step" in line["metric"]
        assert line["value"] > 0 and abs(line["value"] * line["ms_per_step"] * 1e-3 - 4096) < 1e-6 * 4096
        assert "configs" not in line and "cpu_baseline" not in line and "rocm_eager_baseline" not in line and line["kernels"] == {}
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    for want in ("rgb_map", "disp_map", "acc_map", "rgb0", "raw", "loss", "grad_coarse", "grad_fine", "params_coarse", "params_fine"):
        assert want + ".npy" in names, names
    total = 0
    for nm in names:
        a, b = np.load(tmp_path / "a" / nm), np.load(tmp_path / "b" / nm)
        total += a.nbytes
        assert a.dtype == np.float32 and np.array_equal(a, b, equal_nan=True), nm
    assert total <= 64 << 20
    rgb, grad = np.load(tmp_path / "a" / "rgb_map.npy"), np.load(tmp_path / "a" / "grad_fine.npy")
    assert rgb.shape == (4096, 3) and np.isfinite(rgb).all() and np.load(tmp_path / "a" / "raw.npy").shape == (4096, 192, 4)
    assert grad.shape == (595844,) and np.isfinite(grad).all() and np.abs(grad).max() > 0
