"""bench.py's two kinds of run: a plain run measures the headline figure only; --full adds the instrumented per-call pass, the mIoU
parity pair and the CPU oracle baseline (tests/test_dist_gpu.py runs --full with two ranks)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_full_is_off_by_default_and_all_kernels_needs_it():
    import bench
    args = bench.parse(["--gpus", "1", "--steps", "5", "--warmup", "2"])
    assert not args.full and args.steps == 5 and args.warmup == 2
    assert bench.parse(["--full", "--all-kernels", "k.json"]).full
    with pytest.raises(SystemExit):
        bench.parse(["--all-kernels", "k.json"])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_nothing_else(tmp_path):
    """One GPU, small size: the line carries the headline fields, the instrumented pass, mIoU pair and CPU baseline did not run, and
    --dump-outputs still writes what the last timed step computed."""
    env = dict(os.environ, DGTD_GEMM_CANDIDATES="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--size", "64",
           "--batch", "2", "--dump-outputs", str(tmp_path)]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + "\n" + p.stderr[-4000:]
    lines = p.stdout.splitlines()
    assert len(lines) == 1, p.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["unit"] == "images/s" and out["higher_is_better"] is True and out["dtype"] == "bf16"
    assert out["metric"].startswith("training images/sec (64x64 RGB-D, bs=2 per GPU")
    assert out["value"] > 0 and out["ms_per_step"] > 0
    assert abs(out["value"] - 2 * 2 / (2 * out["ms_per_step"] / 1e3)) <= 1e-3 * out["value"] + 1e-3
    assert out["roofline"] is None and out["entries"] == [] and out["kernels"] == [] and out["attention_mfma"] == []
    assert "miou" not in out and "cpu_baseline" not in out
    assert "instrumented pass" not in p.stderr and "mIoU parity" not in p.stderr and "CPU oracle" not in p.stderr
    assert np.load(tmp_path / "loss.npy").shape == (1,)
    assert np.load(tmp_path / "params_sample.npy").size > 0 and np.load(tmp_path / "params_sums.npy").shape[1] == 2
