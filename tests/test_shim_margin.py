"""The C++ shim's margin calls -- isEdgeClear and repairTrajectory then shortcutTrajectory with a margin on one planned
room3 trajectory (tests/cpp/shim_margin.cpp) -- answer as the Python mirror does for the same scene, seed and budget.
CPU: the program builds with -Wall -Werror, links and fails loudly without a GPU."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_shim_clearance import BT, ITERS, LIBDIR, MODEL, SEED, case

SAMPLES, WINDOW = 64, 4
# (map, self) margins in metres.  By the CPU oracle's plan and the clearance restatement the trajectory stays 0.5 m from
# the map and 2.35 cm from itself, its last pose the nearest: the first pair leaves it clear (the sweeps run: the map
# is within the prefilter's reach), the second makes its last pose unclear.
MARGINS = ((0.35, 0.0), (0.0, 0.024))


def build_shim(tmpdir):
    exe = os.path.join(str(tmpdir), "shim_margin")
    subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "shim_margin.cpp"), "-L", LIBDIR, "-lsmp_gpu",
                    "-Wl,-rpath," + LIBDIR, "-o", exe], check=True, capture_output=True, text=True)
    return exe


def run_shim(exe, sc, margin):
    args = [exe, MODEL, BT, str(ITERS), str(SEED), "%.17g" % margin[0], "%.17g" % margin[1], str(SAMPLES), str(WINDOW)]
    args += ["%.17g" % v for v in list(sc.start) + list(sc.goal) + list(sc.env_x) + list(sc.env_y)]
    return subprocess.run(args, capture_output=True, text=True, timeout=300)


def test_shim_margin_builds_and_fails_loudly_without_gpu(tmp_path):
    exe = build_shim(tmp_path)
    p = run_shim(exe, case(), MARGINS[0])
    if p.returncode == 3:
        assert "no usable GPU" in p.stdout or "NO_DEVICE" in p.stdout.upper(), p.stdout
    else:
        assert p.returncode == 0, p.stderr


def rows_of(lines, tag):
    return np.array([[float(v) for v in l.split()[1:]] for l in lines if l.split()[0] == tag], np.float64).reshape(-1, 8)


@pytest.mark.gpu
def test_shim_matches_the_python_mirror(tmp_path):
    from squirrel_motion_planner_amd.planner import BiRRTstarPlanner
    exe = build_shim(tmp_path)
    sc = case()
    pl = BiRRTstarPlanner(seed=SEED)
    pl.initialize()
    pl.setOctree(open(BT, "rb").read())
    pl.setPlanningSceneInfo(sc.env_x, sc.env_y)
    assert pl.init_planner(list(sc.start), list(sc.goal), 1, True, True)
    assert pl.run_planner(1, 0, ITERS)
    planned = [list(w) for w in pl.getJointTrajectoryRef()]
    outcomes = []
    for margin in MARGINS:
        p = run_shim(exe, sc, margin)
        assert p.returncode == 0, p.stdout + p.stderr
        lines = p.stdout.splitlines()
        head = {l.split()[0]: l.split()[1:] for l in lines if l.split()[0] not in ("row", "srow")}
        assert head["status"] == ["1"] and head["waypoints"] == [str(len(planned))]
        traj = [list(w) for w in planned]
        clear, last = pl.isEdgeClear(traj[0], traj[-1], margin)
        assert head["clear"] == [str(int(clear)), str(last)]
        ok = pl.repairTrajectory(traj, True, True, SAMPLES, 4, 1, margin=margin)
        r = pl.repair_info
        f = head["repair"]
        assert [int(v) for v in f[:9]] == [int(ok), len(traj), r["n_blocked_edges"], r["n_gaps"], r["n_repaired"],
                                           r["n_items"], r["n_free"], r["rounds_used"], r["first_blocked"]]
        assert (float(f[9]), float(f[10])) == (r["cost_in"], r["cost_out"])
        assert np.array_equal(rows_of(lines, "row"), np.array(traj))
        sok = pl.shortcutTrajectory(traj, True, True, WINDOW, margin=margin)
        s = pl.shortcut_info
        f = head["shortcut"]
        assert [int(v) for v in f[:4]] == [int(sok), len(traj), s["n_edges"], s["n_valid"]]
        assert float(f[4]) == s["cost_out"]
        assert np.array_equal(rows_of(lines, "srow"), np.array(traj))
        outcomes.append((ok, sok))
    assert outcomes[0] == (True, True) and outcomes[1][0] is False
