"""bench.py as a command: a plain run prints the headline line alone, `--steps` sets the timed
steps, and `--dump-outputs` writes what the last timed step computed — checked bit for bit against
the same seeded trainer stepped in this process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(n_envs=2048, hidden=64, n_hidden=2, batch=512, updates_per_step=2,
             envs_per_group=256)
STEPS, WARMUP = 3, 2  # 5 x 2048 rows into a ring of 10 000: the last step's rows wrap


def test_plain_run_line_and_dumped_outputs(tmp_path):
    import bench
    from nav import _lib
    from nav.trainer import VecTrainer
    _lib.require_gpu()
    out = os.path.join(tmp_path, "dump")
    r = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
         "--warmup", str(WARMUP), "--envs", "2048", "--hidden", "64", "--layers", "2",
         "--batch", "512", "--updates", "2", "--envs-per-group", "256", "--dump-outputs", out],
        capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["full"] is False
    assert line["unit"] == "env-steps/s" and line["higher_is_better"] is True and line["dtype"]
    assert line["ms_per_step"] > 0
    # value and ms_per_step are the same measurement: envs x steps / the timed region
    assert line["value"] == pytest.approx(2048 / (line["ms_per_step"] * 1e-3), rel=1e-9)
    # nothing of the --full legs in a plain run
    for k in ("roofline", "kernels", "timed_long", "tick_forms", "step_kernel_sweep",
              "cpu_baseline", "utd_sweep"):
        assert k not in line, k

    # the same seeded trainer here: max(warmup, 1) + steps steps, then the arrays a caller sees
    torch.cuda.set_device(0)
    tr = VecTrainer(device="cuda:0", **SMALL)
    for _ in range(max(WARMUP, 1) + STEPS):
        tr.step()
    torch.cuda.synchronize()
    want = bench.step_outputs(tr)
    assert sorted(os.listdir(out)) == sorted(k + ".npy" for k in want)
    total = 0
    for k, t in want.items():
        got = np.load(os.path.join(out, k + ".npy"))
        total += got.nbytes
        assert got.dtype == (np.float32 if t.dtype == torch.float32 else np.float64), k
        assert np.isfinite(got).all(), k
        np.testing.assert_array_equal(got, t.cpu().numpy().astype(got.dtype), err_msg=k)
    assert total <= bench.DUMP_BUDGET_BYTES
    # the replay rows are this step's, in env order: their slots end at the ring's write position
    pos, cap = tr.replay.position, tr.replay.capacity
    assert pos == (5 * 2048) % cap and pos < tr.n
    rows = torch.cat([tr.replay.rows[cap - (tr.n - pos):], tr.replay.rows[:pos]])
    assert torch.equal(want["replay_rows"], rows)
    assert not torch.equal(want["net_actor"], want["net_target_actor"])  # the learner ran
