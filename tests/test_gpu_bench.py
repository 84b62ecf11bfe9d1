"""bench.py's plain run on the MI355X: `--gpus 1 --steps K --warmup W --dump-outputs DIR` times K steps, prints the contract's
line without the `--full` objects, and writes what the last step left behind (parameter arena, momentum, Fisher diagonal, the
last Fisher batch's gradient and loss, the training loss / #correct sums)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_bench_run_line_and_dump(tmp_path):
    out = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", out], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert (line["steps"], line["warmup"], line["unit"], line["higher_is_better"]) == (3, 1, "images/s", True)
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(400 * 1e3 / line["ms_per_step"], rel=1e-4)
    for k in ("roofline", "cpu_baseline", "configs_ms_per_step", "sweep_s", "sharded_sweep", "details"):
        assert k not in line, k
    assert "bench-details" not in r.stderr
    d = {f[:-4]: np.load(os.path.join(out, f)) for f in os.listdir(out)}
    assert sorted(d) == ["fisher", "grad", "loss", "momentum", "params", "train_stats"]
    n = d["params"].size
    for k in ("params", "momentum", "fisher", "grad"):
        assert d[k].dtype == np.float32 and d[k].shape == (n,) and np.isfinite(d[k]).all(), k
    assert d["loss"].dtype == np.float32 and d["loss"].shape == (1,) and np.isfinite(d["loss"]).all() and d["loss"][0] > 0
    # train batches of 200: the first step, 1 warm-up step, 3 timed steps
    s = d["train_stats"]
    assert s.dtype == np.float64 and s.shape == (2,) and s[0] > 0 and s[1] == np.round(s[1]) and 0 <= s[1] <= 5 * 200
    # the Fisher diagonal sums g^2 / 8000 over every Fisher batch so far, the last one (whose gradient is dumped) included
    last = d["grad"].astype(np.float64) ** 2 / 8000.0
    assert (d["fisher"] >= last * (1 - 1e-5) - 1e-6 * float(d["fisher"].max())).all()
