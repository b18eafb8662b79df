"""The C++ shim's isEdgeValid and shortcutTrajectory (tests/cpp/shim_shortcut.cpp) answer as the Python mirror does on
the same trajectory and scene.  CPU: the program builds with -Wall -Werror, links and fails loudly without a GPU."""
import os
import subprocess

import numpy as np
import pytest

import shortcut_restatement as R
from conftest import ROOT

LIBDIR = os.path.join(ROOT, "squirrel_motion_planner_amd", "lib")
MODEL = os.path.join(ROOT, "squirrel_motion_planner_amd", "data", "robotino_model.json")
BT = os.path.join(ROOT, "tests", "golden", "room3.bt")


def build_shim(tmpdir):
    exe = os.path.join(str(tmpdir), "shim_shortcut")
    subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "shim_shortcut.cpp"), "-L", LIBDIR, "-lsmp_gpu",
                    "-Wl,-rpath," + LIBDIR, "-o", exe], check=True, capture_output=True, text=True)
    return exe


def trajectory():
    """Eight poses across room3 (the scene of room3.bt, no floor inserted): base and arm move together, so several
    edges are longer than a planner step."""
    from squirrel_motion_planner_amd import scenes
    a = np.array([0.0, 0.0, 0.0] + scenes.ARM_FOLDED)
    b = np.array([2.0, 1.5, 0.8] + scenes.ARM_UNFOLDED)
    t = np.array([0.0, 0.1, 0.3, 0.35, 0.6, 0.7, 0.9, 1.0])[:, None]
    w = a[None, :] + t * (b - a)[None, :]
    w[2, 1] += 0.25  # two detours a shortcut removes
    w[5, 0] -= 0.2
    return w


def run_shim(exe, w, window):
    args = [exe, MODEL, BT, str(window), str(len(w))] + ["%.17g" % v for v in w.reshape(-1)]
    return subprocess.run(args, capture_output=True, text=True, timeout=120)


def test_shim_shortcut_builds_and_fails_loudly_without_gpu(tmp_path):
    exe = build_shim(tmp_path)
    p = run_shim(exe, trajectory(), 0)
    if p.returncode == 3:
        assert "no usable GPU" in p.stdout or "NO_DEVICE" in p.stdout.upper(), p.stdout
    else:
        assert p.returncode == 0, p.stderr


def blocked_trajectory():
    """The same poses and a ninth inside the room's furniture: by the oracle the last edge collides at point 43 of its
    61, so the reference's last valid index is 42 and no route remains."""
    from squirrel_motion_planner_amd import scenes
    return np.concatenate([trajectory(), [np.array([2.0, 3.0, 0.8] + scenes.ARM_UNFOLDED)]])


def shim_answers(exe, w, window):
    p = run_shim(exe, w, window)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.splitlines()
    edges = [tuple(map(int, l.split()[1:])) for l in lines if l.startswith("edge ")]
    head = [l for l in lines if l.startswith("shortcut ")]
    rows = np.array([[float(v) for v in l.split()[1:]] for l in lines if l.startswith("row ")])
    return edges, head, rows


def mirror():
    from squirrel_motion_planner_amd.planner import BiRRTstarPlanner
    pl = BiRRTstarPlanner()
    pl.initialize()
    pl.setOctree(open(BT, "rb").read())
    return pl


@pytest.mark.gpu
@pytest.mark.parametrize("window", [0, 2])
def test_shim_matches_the_python_mirror(tmp_path, window):
    exe = build_shim(tmp_path)
    w = trajectory()
    pl = mirror()
    edges = [pl.isEdgeValid(list(w[i]), list(w[i + 1]), True, True) for i in range(len(w) - 1)]
    traj = [list(map(float, r)) for r in w]
    ok = pl.shortcutTrajectory(traj, True, True, window)
    assert ok and len(traj) != len(w) and pl.shortcut_info["cost_out"] < pl.shortcut_info["cost_in"]
    m, _ = R.density(w[:-1], w[1:], R.orobot().rev, R.N_SEG, R.STEP)
    assert m.max() >= 2
    assert edges == [(True, R.N_SEG * int(mm)) for mm in m]  # free edges: the index of the last point
    got_edges, head, rows = shim_answers(exe, w, window)
    assert got_edges == [(i, int(v), last) for i, (v, last) in enumerate(edges)]
    assert head == ["shortcut 1 %d" % len(traj)]
    assert np.array_equal(rows, np.array(traj))


@pytest.mark.gpu
def test_shim_blocked_trajectory_matches_the_python_mirror(tmp_path):
    exe = build_shim(tmp_path)
    w = blocked_trajectory()
    pl = mirror()
    edges = [pl.isEdgeValid(list(w[i]), list(w[i + 1]), True, True) for i in range(len(w) - 1)]
    assert edges[-1] == (False, 42) and all(v for v, _ in edges[:-1])
    traj = [list(map(float, r)) for r in w]
    assert not pl.shortcutTrajectory(traj, True, True, 0)
    assert np.array_equal(np.array(traj), w) and pl.shortcut_info["first_blocked"] == len(w) - 2
    got_edges, head, rows = shim_answers(exe, w, 0)
    assert got_edges == [(i, int(v), last) for i, (v, last) in enumerate(edges)]
    assert head == ["shortcut 0 %d" % len(w)]
    assert np.array_equal(rows, w)
