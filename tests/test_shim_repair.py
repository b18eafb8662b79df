"""The C++ shim's repairTrajectory, followed by shortcutTrajectory (tests/cpp/shim_repair.cpp), answers as the Python
mirror does on the same trajectory and scene.  CPU: the program builds with -Wall -Werror, links and fails loudly
without a GPU."""
import os
import subprocess

import numpy as np
import pytest

import repair_restatement as P
from conftest import ROOT

LIBDIR = os.path.join(ROOT, "squirrel_motion_planner_amd", "lib")
MODEL = os.path.join(ROOT, "squirrel_motion_planner_amd", "data", "robotino_model.json")
BT = os.path.join(ROOT, "tests", "golden", "room3.bt")
INFO = ("n_blocked_edges", "n_gaps", "n_repaired", "n_items", "n_free", "rounds_used", "first_blocked")


def build_shim(tmpdir):
    exe = os.path.join(str(tmpdir), "shim_repair")
    subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "shim_repair.cpp"), "-L", LIBDIR, "-lsmp_gpu",
                    "-Wl,-rpath," + LIBDIR, "-o", exe], check=True, capture_output=True, text=True)
    return exe


def trajectory():
    """Five poses across room3 (the scene of room3.bt, no floor inserted) whose middle one stands inside the room's
    furniture: by the oracle one gap (1, 3), which a detour of the second round closes (half width 1 m)."""
    from squirrel_motion_planner_amd import scenes
    return np.array([[x, y, 0.8] + scenes.ARM_UNFOLDED
                     for x, y in ((0.25, 2.0), (1.0, 3.0), (2.0, 3.0), (3.0, 3.0), (3.75, 2.5))])


def run_shim(exe, w, samples, rounds, seed):
    args = [exe, MODEL, BT, str(samples), str(rounds), str(seed), str(len(w))] + ["%.17g" % v for v in w.reshape(-1)]
    return subprocess.run(args, capture_output=True, text=True, timeout=120)


def test_shim_repair_builds_and_fails_loudly_without_gpu(tmp_path):
    exe = build_shim(tmp_path)
    p = run_shim(exe, trajectory(), 32, 3, 1)
    if p.returncode == 3:
        assert "no usable GPU" in p.stdout or "NO_DEVICE" in p.stdout.upper(), p.stdout
    else:
        assert p.returncode == 0, p.stderr


def test_the_trajectory_is_repairable_by_the_oracle():
    """The non-vacuity of the GPU test below, on the CPU: room3's keys without a floor are the scene of room3.bt."""
    from oracle import oracle as O
    import shortcut_restatement as R
    keys = np.load(os.path.join(ROOT, "tests", "golden", "room3_keys.npz"))["keys"].astype(np.int64)
    orc = O.Oracle(R.orobot(), O.OracleScene(keys, 0.05))
    w = trajectory()
    assert list(orc.check_configs(w)) == [1, 1, 0, 1, 1]
    r = P.repair(orc, w, samples=32, rounds=3, seed=1)
    assert r["status"] == P.OK and r["gaps"] == [[1, 3, 1]] and r["closed_round"] == [1]
    assert P.repair(orc, w, samples=4, rounds=1, seed=1)["status"] == P.ERR_NO_SOLUTION


def shim_answers(exe, w, samples, rounds, seed):
    p = run_shim(exe, w, samples, rounds, seed)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.splitlines()
    head = [l.split()[1:] for l in lines if l.startswith("repair ")]
    shead = [l for l in lines if l.startswith("shortcut ")]
    rows = np.array([[float(v) for v in l.split()[1:]] for l in lines if l.startswith("row ")])
    srows = np.array([[float(v) for v in l.split()[1:]] for l in lines if l.startswith("srow ")])
    assert len(head) == 1
    return head[0], shead, rows, srows


def mirror():
    from squirrel_motion_planner_amd.planner import BiRRTstarPlanner
    pl = BiRRTstarPlanner()
    pl.initialize()
    pl.setOctree(open(BT, "rb").read())
    return pl


@pytest.mark.gpu
def test_shim_matches_the_python_mirror(tmp_path):
    exe = build_shim(tmp_path)
    w = trajectory()
    pl = mirror()
    traj = [list(map(float, r)) for r in w]
    assert not pl.shortcutTrajectory(traj, True, True) and np.array_equal(np.array(traj), w)  # blocked as it is
    assert pl.repairTrajectory(traj, True, True, samples=32, rounds=3, seed=1)
    ri = pl.repair_info
    assert ri["n_gaps"] == 1 and ri["n_repaired"] == 1 and ri["rounds_used"] == 2 and len(traj) > len(w)
    repaired = np.array(traj)
    assert pl.shortcutTrajectory(traj, True, True)
    head, shead, rows, srows = shim_answers(exe, w, 32, 3, 1)
    assert head[:2] == ["1", str(len(repaired))]
    assert [int(v) for v in head[2:9]] == [ri[f] for f in INFO]
    assert float(head[9]) == ri["cost_in"] and float(head[10]) == ri["cost_out"]
    assert np.array_equal(rows, repaired)
    assert shead == ["shortcut 1 %d" % len(traj)]
    assert np.array_equal(srows, np.array(traj))


@pytest.mark.gpu
def test_shim_unrepaired_trajectory_matches_the_python_mirror(tmp_path):
    """Four samples of one round close nothing: both leave the trajectory untouched and report the blocked edge; and a
    trajectory that ends on the colliding pose is refused (its goal is invalid)."""
    exe = build_shim(tmp_path)
    w = trajectory()
    pl = mirror()
    traj = [list(map(float, r)) for r in w]
    assert not pl.repairTrajectory(traj, True, True, samples=4, rounds=1, seed=1)
    ri = pl.repair_info
    assert np.array_equal(np.array(traj), w) and ri["first_blocked"] == 1 and ri["n_repaired"] == 0
    head, shead, rows, srows = shim_answers(exe, w, 4, 1, 1)
    assert head[:2] == ["0", str(len(w))]
    assert [int(v) for v in head[2:9]] == [ri[f] for f in INFO]
    assert np.array_equal(rows, w) and shead == ["shortcut 0 %d" % len(w)] and np.array_equal(srows, w)
    traj = [list(map(float, r)) for r in w[:3]]
    assert not pl.repairTrajectory(traj, True, True, samples=4, rounds=1, seed=1) and len(traj) == 3
    head, _, rows, _ = shim_answers(exe, w[:3], 4, 1, 1)
    assert head[:2] == ["0", "3"] and np.array_equal(rows, w[:3])
