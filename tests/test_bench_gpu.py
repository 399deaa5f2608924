"""bench.py's plain run (the driver's `--gpus 1 --steps K --warmup W`): one timed run of exactly K steps and the contract line,
nothing else measured; `--dump-outputs DIR` writes what that run computed in its last step, and two runs with the same arguments
compute the same thing."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C3_D = [6, 8, 8, 10, 10, 12, 12, 12]


def _plain(steps, dump):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "5",
                        "--dump-outputs", str(dump)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.split("\n") if l.strip()]
    return json.loads(lines[-1])


@pytest.mark.timeout(600)
def test_plain_bench_times_the_steps_and_dumps_the_last_step(tmp_path):
    import nfisam_hip as nh
    d = _plain(40, tmp_path / "a")
    assert d["steps"] == 40 and d["warmup"] == 5 and d["n_gpus"] == 1 and d["full"] is False
    assert d["metric"].startswith("flow-training samples/sec") and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["value"] > 1e7 and 0 < d["ms_per_step"] < 5.0
    assert abs(d["value"] - 8 * 2000 * 40 / (1e-3 * d["ms_per_step"] * 40)) < 1e-6 * d["value"]
    assert d["timing"].startswith("one run of the 40-step plan")
    for k in ("roofline", "regimes", "replicas", "exchange", "cpu_baseline", "wall_clock_per_incremental_update"):
        assert k not in d, k                 # measured by `--full` only
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(["params_clique%d.npy" % c for c in range(8)] + ["last_step_loss.npy"]), names
    a = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    assert sum(v.nbytes for v in a.values()) < 64 << 20
    for c, D in enumerate(C3_D):
        v = a["params_clique%d" % c]
        assert v.dtype == np.float32 and v.shape == (nh.param_count(D, 9, 8),) and np.all(np.isfinite(v))
    loss = a["last_step_loss"]
    assert loss.dtype == np.float32 and loss.shape == (8,) and np.all(np.isfinite(loss))
    assert abs(float(loss.mean()) - d["final_loss"]) < 1e-5 * max(1.0, abs(d["final_loss"]))
    # the same arguments: the same inputs, so the same outputs
    e = _plain(40, tmp_path / "b")
    for n, v in a.items():
        np.testing.assert_allclose(np.load(tmp_path / "b" / (n + ".npy")), v, rtol=1e-5, atol=1e-6, err_msg=n)
    assert e["first_loss"] == pytest.approx(d["first_loss"], rel=1e-6)
