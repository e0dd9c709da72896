"""-m gpu: the plain benchmark command - `bench.py --gpus 1 --steps K --warmup W` times exactly K steps, prints the headline
fields and nothing that --full measures, and --dump-outputs writes what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_reports_the_headline_and_dumps_the_last_step(tmp_path):
    env = dict(os.environ)
    env.pop("SED_POISON", None)
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "3",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads(r.stdout.strip().split("\n")[-1])
    assert d["metric"] == "10-s clips/sec mean-teacher train step (64-mel x 628)" and d["unit"] == "clips/s"
    assert d["higher_is_better"] is True and d["dtype"] == "f32" and d["steps"] == 7 and d["warmup"] == 3
    assert d["ms_per_step"] > 0 and abs(d["value"] - 24 * 1e3 / d["ms_per_step"]) < 1e-3 * d["value"]
    for moved in ("ms_per_step_events", "cpu_baseline", "steady_state", "extra_configs", "feature_path"):
        assert moved not in d, moved
    assert "kernels" not in d["roofline"]
    names = {"meters", "student_params", "student_bn_running", "adam_exp_avg", "adam_exp_avg_sq", "strong", "weak",
             "teacher_params", "teacher_bn_running", "strong_ema", "weak_ema"}
    assert {p.name for p in out.iterdir()} == {n + ".npy" for n in names}
    a = {n: np.load(out / (n + ".npy")) for n in names}
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    assert a["student_params"].shape == a["teacher_params"].shape == a["adam_exp_avg"].shape == (214356,)
    assert a["strong"].shape == (24, 78, 10) and a["weak"].shape == (24, 10)
    assert abs(float(a["meters"][0]) - d["loss"]) < 1e-5
    assert not np.array_equal(a["student_params"], a["teacher_params"])
