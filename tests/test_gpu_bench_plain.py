"""-m gpu: a plain bench.py run (no --full) -- ONE timed region of exactly --steps steps, no legs beside the headline -- and what
--dump-outputs writes: the pose the timed refinement returned after its last step, with its step norm and cost, as float64 .npy."""
import os

import numpy as np
import pytest

from bench_util import run_bench

pytestmark = pytest.mark.gpu


def test_plain_run_times_its_steps_and_dumps_the_last_step(tmp_path):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "RPE_BENCH_INJECT_LOST_GRID"):
        env.pop(k, None)
    d = tmp_path / "outputs"
    r, line, j = run_bench(["--gpus", "1", "--steps", "30", "--warmup", "5", "--dump-outputs", str(d)], env, timeout=600)
    assert line["steps"] == 30 and line["warmup"] == 5 and line["ms_per_step"] > 0 and line["metric"] == "correspondence-residuals/sec"
    assert abs(line["value"] - line["config"]["valid_corr_per_step"] / (line["ms_per_step"] * 1e-3)) < 1e-6 * line["value"]
    assert j["timing"]["repeats"] == 1 and j["roofline"]["launches_timed"] == 0 and j["untuned"] is None and j["cpu_baseline"] is None
    assert "valid" not in j and j["config"]["resident_state"]["resident_loop_ran"] is True and j["roofline"]["steps_per_launch"] == 30
    for k in ("pose_error_vs_cpu", "convergence", "roofline_hbm", "ransac_scoring", "fp64"):
        assert k not in j, k
    got = {p.name: np.load(p) for p in d.iterdir()}
    assert set(got) == {"pose.npy", "step_norm.npy", "cost.npy"} and all(a.dtype == np.float64 for a in got.values())
    pose = got["pose.npy"]
    R = pose[:9].reshape(3, 3)
    assert pose.shape == (12,) and np.all(np.isfinite(pose)) and np.allclose(R @ R.T, np.eye(3), atol=1e-9)
    assert got["step_norm.npy"][0] < 1e-6 and got["cost.npy"][0] > 0            # converged long before the 30th step
    import bench
    sc = bench.make_shard(0, 307200)
    assert bench.rot_err(R, sc.R) < 1e-2 and np.linalg.norm(pose[9:] - sc.t) < 2e-2
