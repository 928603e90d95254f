"""bench.py's plain run (headline only) and --dump-outputs, on a small configuration of the bench step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--steps", "3", "--warmup", "1", "--batch", "2", "--size", "64", "--dtype", "f32"]


def _bench(args, env=None):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def test_plain_bench_times_the_steps_and_dumps_the_last_one(tmp_path):
    out = tmp_path / "dump"
    line = _bench(["--gpus", "1"] + SMALL + ["--dump-outputs", str(out)])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["dtype"] == "f32" and line["higher_is_better"] is True
    assert line["unit"] == "tiles/s" and line["ms_per_step"] > 0
    assert abs(line["value"] - 2 * 3 / (line["ms_per_step"] * 3e-3)) < 1e-2 * line["value"]
    for k in ("roofline", "roofline_alone", "inference_roofline", "surface", "cpu_baseline", "fp32_parity_tiles_per_s"):
        assert k not in line, k   # --full only
    assert line["inference_tiles_per_s"] is None
    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert set(got) == {"loss", "preds", "confmat", "params", "grads", "buffers"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 * 10 ** 6
    assert abs(float(got["loss"][0]) - line["final_loss"]) < 1e-4
    assert got["preds"].size == 2 * 64 * 64 and got["preds"].min() >= 0 and got["preds"].max() < 13
    # the confusion matrix counts every pixel of the warm-up and timed steps
    assert got["confmat"].shape == (13 * 13,) and got["confmat"].sum() == 4 * 2 * 64 * 64
    assert np.isfinite(got["params"]).all() and np.isfinite(got["grads"]).all() and np.abs(got["grads"]).max() > 0


def test_plain_bench_n_gt_1_reports_the_slowest_rank_only():
    env = dict(os.environ, FLAIR_BENCH_BACKEND="gloo", FLAIR_BENCH_DEVICES="0,0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    line = _bench(["--gpus", "2"] + SMALL, env=env)
    assert line["n_gpus"] == 2 and line["config"]["global_batch"] == 4
    assert abs(line["value"] - 4 * 3 / (line["ms_per_step"] * 3e-3)) < 1e-2 * line["value"]
    assert "exchange" not in line
