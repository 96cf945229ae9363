"""bench.py's plain run on one GPU: the result line's headline fields, exactly `--steps` timed steps, nothing of `--full`,
and `--dump-outputs`: finite float32 / float64 arrays, at most 64 MB, identical for identical arguments."""
import json
import os
import sys

import numpy as np
import pytest

from tests.proc_util import run_group

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
           "--dump-outputs", str(out_dir)]
    out = run_group(cmd, env, ROOT, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_plain_run_line_and_reproducible_outputs(tmp_path):
    a, b = _plain_run(tmp_path / "a"), _plain_run(tmp_path / "b")
    for res in (a, b):
        assert res["steps"] == 3 and res["ms_per_step"] > 0 and res["higher_is_better"] is True
        assert res["value"] == pytest.approx(1e3 / res["ms_per_step"], rel=1e-3)  # B = 256 on one GPU
        assert res["dtype"] == "bf16" and res["unit"] == "grad-steps/s" and res["config"]["losses_finite"] is True
        assert all(res[k] is None for k in ("step_time", "strong", "configs", "roofline")) and "cpu_baseline" not in res
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert {"latent_plan.npy", "param_actor.npy", "param_q1.npy", "metric_actor_loss.npy", "metric_q1_loss.npy"} <= set(names)
    total = 0
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype in (np.float32, np.float64) and x.size > 0, n
        assert np.isfinite(x).all(), n
        assert np.array_equal(x, y), n
        total += x.nbytes
    assert total <= 64 << 20
    assert np.load(tmp_path / "a" / "latent_plan.npy").shape == (256, 16)
