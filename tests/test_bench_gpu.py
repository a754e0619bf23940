"""bench.py as the driver runs it, at the tiny shape: a plain run times exactly --steps steps of a fixed size, measures the
headline workload only and writes no detail file unless asked; --dump-outputs writes the same outputs in two runs with
the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None), env.pop("RANK", None), env.pop("LOCAL_RANK", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "tiny", "--steps", "3", "--warmup", "1"]
    p = subprocess.run(cmd + list(args), env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.splitlines()[-1])


def test_plain_run_times_the_given_steps_and_dumps_reproducible_outputs(tmp_path):
    a = _bench("--dump-outputs", str(tmp_path / "a"))
    assert a["steps"] == 3 and a["warmup"] == 1 and a["ms_per_step"] > 0 and a["plan_violations"] == 0
    assert a["roofline"] is None and a["cpu_baseline"] is None and a["detail"] is None
    for k in ("S", "f32_conv", "through_plugin", "nchw_input", "St", "A", "train_S"):
        assert k not in a, k
    detail = tmp_path / "b.json"
    b = _bench("--dump-outputs", str(tmp_path / "b"), "--detail", str(detail))
    with open(detail) as f:
        d = json.load(f)
    sps = d["scenes_per_step"]
    assert sps == a["config"]["scenes_per_step"] == 9                     # 8 scenes, rounded up to whole rounds over 3 slots
    assert len(d["windows_scenes_per_s"]) == 1                           # one window of exactly --steps steps
    # what the run did, counted where it does it: Workload.step() calls and the scenes they ran
    assert d["timed_steps"] == 3 and d["steps_run"] == 1 + 3 and d["scenes_run"] == (1 + 3) * sps
    assert d["ms_per_step"] == pytest.approx(d["window_s"] / 3 * 1e3, rel=1e-9)
    assert d["value"] == pytest.approx(3 * sps / d["window_s"], rel=1e-9)
    assert b["value"] == pytest.approx(d["value"], rel=1e-3)
    out = {}
    for run in ("a", "b"):
        out[run] = {k: np.load(tmp_path / run / f"{k}.npy") for k in ("bboxes", "scores", "rows")}
    rows = out["a"]["rows"]
    assert rows.shape[0] == sps and rows.sum() == out["a"]["bboxes"].shape[0] == out["a"]["scores"].shape[0] > 0
    assert out["a"]["bboxes"].dtype == out["a"]["scores"].dtype == np.float32
    assert np.isfinite(out["a"]["bboxes"]).all() and np.isfinite(out["a"]["scores"]).all()
    for k in ("bboxes", "scores", "rows"):
        assert np.array_equal(out["a"][k], out["b"][k]), k                 # bit for bit: same scenes, same seeds, same graphs
