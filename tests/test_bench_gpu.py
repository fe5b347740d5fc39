"""bench.py without --full: the headline line and nothing else; --dump-outputs writes what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_plain_run_dumps_last_step(tmp_path):
    d = tmp_path / "out"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2",
                          "--settle", "0", "--batch", "128", "--dump-outputs", str(d)], cwd=ROOT, capture_output=True, text=True,
                         timeout=600, env={k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")})
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    res = json.loads(lines[0])
    assert res["steps"] == 5 and res["warmup"] == 2 and res["ms_per_step"] > 0
    assert res["value"] == pytest.approx(128 / (res["ms_per_step"] * 1e-3), rel=1e-9)
    # the secondary legs are --full's
    assert res["roofline"] is None and res["ms_per_step_with_upload"] is None
    for k in ("cpu_baseline", "elbo_parity", "other_workloads", "dp_overhead_1rank", "transformer_variants"):
        assert k not in res
    loss = np.load(d / "loss.npy")
    params = np.load(d / "params.npy")
    assert loss.dtype == np.float32 and loss.shape == (4,) and loss[0] == np.float32(res["final_loss"])
    assert params.dtype == np.float32 and params.ndim == 1 and np.isfinite(params).all()
    assert os.path.getsize(d / "loss.npy") + os.path.getsize(d / "params.npy") <= 64e6
