"""The C++ shim's attached-object calls -- attachBox, setSelfFilter, plan, detachObject on a map that holds the grasped
bar's own voxels (tests/cpp/shim_attach.cpp) -- answer as the Python mirror does for the same map, seed and budget.
CPU: the program builds with -Wall -Werror, links and fails loudly without a GPU."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from oracle import octomap_bt
from test_gpu_attach import OBJECT, Q_GOAL, Q_MAP, RES, carve_keys_case

LIBDIR = os.path.join(ROOT, "squirrel_motion_planner_amd", "lib")
MODEL = os.path.join(ROOT, "squirrel_motion_planner_amd", "data", "robotino_model.json")
ITERS, SEED = 100, 4
ENV = (-3.0, 3.0, -3.0, 3.0)
HALF, POSE = (0.03, 0.03, 0.10), [1, 0, 0, 0, 1, 0, 0, 0, 1, 0.0, 0.0, 0.15]


def build_shim(tmpdir):
    exe = os.path.join(str(tmpdir), "shim_attach")
    subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "shim_attach.cpp"), "-L", LIBDIR, "-lsmp_gpu",
                    "-Wl,-rpath," + LIBDIR, "-o", exe], check=True, capture_output=True, text=True)
    return exe


def write_map(tmpdir):
    """The carve tests' map (room3, floor, pillar and the bar's cells at Q_MAP) as an octomap binary file."""
    path = os.path.join(str(tmpdir), "grasp.bt")
    with open(path, "wb") as f:
        f.write(octomap_bt.write_bt(carve_keys_case()[0], RES))
    return path


def run_shim(exe, bt):
    args = [exe, MODEL, bt, str(ITERS), str(SEED), "%.17g" % RES]
    args += ["%.17g" % v for v in list(Q_MAP) + list(Q_GOAL) + list(ENV)]
    return subprocess.run(args, capture_output=True, text=True, timeout=300)


def test_shim_attach_builds_and_fails_loudly_without_gpu(tmp_path):
    exe = build_shim(tmp_path)
    p = run_shim(exe, write_map(tmp_path))
    if p.returncode == 3:
        assert "no usable GPU" in p.stdout or "NO_DEVICE" in p.stdout.upper(), p.stdout
    else:
        assert p.returncode == 0, p.stderr


@pytest.mark.gpu
def test_shim_matches_the_python_mirror(tmp_path):
    from squirrel_motion_planner_amd.planner import BiRRTstarPlanner
    exe = build_shim(tmp_path)
    bt = write_map(tmp_path)
    p = run_shim(exe, bt)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.splitlines()
    head = {l.split()[0]: l.split()[1:] for l in lines if l.split()[0] != "row"}
    rows = np.array([[float(v) for v in l.split()[1:]] for l in lines if l.split()[0] == "row"], np.float64).reshape(-1, 8)

    data = open(bt, "rb").read()
    pl = BiRRTstarPlanner(seed=SEED)
    pl.initialize()
    pl.attachBox("hand_palm_link", HALF, POSE, 0.01)
    assert pl._gpu.robot.link_names[-1] == OBJECT and pl._gpu.robot.self_rounds_info()["n_sph"] == 54
    with pytest.raises(Exception):
        pl.attachBox("hand_palm_link", HALF, POSE, 0.01)  # the name is in use
    assert head["attach"] == ["1"] and head["refused"] == ["0"]
    pl.setOctree(data)
    pl.setPlanningSceneInfo(ENV[:2], ENV[2:])
    uncarved = pl.init_planner(list(Q_MAP), list(Q_GOAL), 1, True, True)
    assert uncarved is False and head["uncarved"] == ["0"]
    self_c, map_c = [], []
    pl.getCollisions(list(Q_MAP), self_c, map_c)
    assert head["maplinks"] == map_c == [OBJECT]
    pl.setSelfFilter(list(Q_MAP), RES, [OBJECT])
    pl.setOctree(data)
    pl.reset_planner_and_config()
    pl.setPlanningSceneInfo(ENV[:2], ENV[2:])
    assert pl.init_planner(list(Q_MAP), list(Q_GOAL), 1, True, True)
    assert pl.run_planner(1, 0, ITERS)
    traj = np.array(pl.getJointTrajectoryRef())
    assert head["carved"] == ["1", "1", str(len(traj))]
    assert np.array_equal(rows, traj)
    pl.detachObject()
    pl.setSelfFilter(None)
    pl.setOctree(data)
    assert head["detached"] == [str(int(pl.isConfigValid(list(Q_MAP), True, True)))]
    assert pl._gpu.robot.link_names[-1] != OBJECT
