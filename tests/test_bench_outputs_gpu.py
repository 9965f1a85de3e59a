"""bench.py's plain run and --dump-outputs on the GPU, at a small size: the line reports the timed steps only (no extra legs without
--full), and two runs with the same arguments write the same outputs of the last timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(out_dir):
    env = dict(os.environ, CSBSR_BENCH_WATCHDOG="300")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "CSBSR_FORCE_DEVICE", "CSBSR_FORCE_DIST"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", "2", "--lr-size", "64", "--steps", "3", "--warmup", "1",
           "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_plain_run_dumps_the_last_step(tmp_path):
    d = _run(tmp_path / "a")
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "imgs/s"
    assert d["with_launch_events"] is None and d["with_h2d_inside_step"] is None and d["other_precision"] is None and d["roofline"] is None
    assert "cpu_baseline" not in d
    names = {"loss", "segment_loss", "sr_loss", "segment_preds", "sr_preds", "kernel_preds", "params"}
    files = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert set(files) == names
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in files.values())
    assert sum(os.path.getsize(tmp_path / "a" / (n + ".npy")) for n in names) <= 64 * 2 ** 20
    assert files["sr_preds"].shape == (2, 3, 256, 256) and files["segment_loss"].shape == (2,)
    assert files["params"].shape == (1 << 22,)           # 89 M fp32 master parameters: a fixed sample
    assert abs(float(files["loss"]) - d["loss"]) <= 1e-5 + 1e-5 * abs(d["loss"])       # (the line rounds to 5 decimals)
    # the same arguments give the same inputs, so the same outputs (the step is deterministic: tests/test_determinism_gpu.py)
    _run(tmp_path / "b")
    for n in names:
        np.testing.assert_allclose(np.load(tmp_path / "b" / (n + ".npy")), files[n], rtol=1e-5, atol=1e-6, err_msg=n)
