"""bench.py as a command on the GPU: a plain run (small budget) times the steps asked for, leaves the CPU baselines
to --full, and with --dump-outputs writes exactly what plan_batch returned in its last timed step."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from squirrel_motion_planner_amd import scenes
from squirrel_motion_planner_amd.planner import GpuPlanner, Scene

sys.path.insert(0, ROOT)
import bench  # noqa: E402

pytestmark = pytest.mark.gpu


def test_plain_run_line_and_dump(tmp_path):
    steps, samples, seed = 2, 20000, 1
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--samples", str(samples), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["warmup"] == 1 and d["unit"] == "configs/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f64" and d["cpu_baseline"] is None
    assert d["ms_per_step"] > 0 and d["value"] > 0
    assert len(d["time_to_first_feasible_path_host_steps_s"]) <= steps
    # the last timed step's query, planned here: same seed, query id and budget
    sc = scenes.box_room()
    gp = GpuPlanner(path_optimality_threshold=-math.inf)
    gp.set_scene(Scene.from_keys(sc.keys, sc.res))
    r = gp.plan(GpuPlanner.make_query(sc.start, sc.goal, sc.env_x, sc.env_y, samples=samples,
                                      seed=seed + 1000 * (steps - 1), query_id=0))
    assert sorted(os.listdir(out)) == ["q0_cost_rows.npy", "q0_path.npy", "q0_stats.npy"]
    path, rows, stats = (np.load(out / ("q0_%s.npy" % n)) for n in ("path", "cost_rows", "stats"))
    assert path.dtype == rows.dtype == stats.dtype == np.float64
    assert np.array_equal(path, r["path"])
    assert np.array_equal(rows, r["cost_rows"][:, [0, 2, 3, 4]])
    want = np.concatenate([np.atleast_1d(np.asarray(r[k], np.float64)) for k in bench.DUMP_STATS])
    assert np.array_equal(stats, want)
    assert stats[bench.DUMP_STATS.index("configs_checked")] >= samples
