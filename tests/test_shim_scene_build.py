"""The C++ shim's setOctreeBinary builds the scene on the GPU (tests/cpp/shim_scene.cpp): isConfigValid through it
answers as the Python host path (Scene.from_bt + set_scene) does.  CPU: it builds, links and fails loudly without a
GPU."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

LIBDIR = os.path.join(ROOT, "squirrel_motion_planner_amd", "lib")
MODEL = os.path.join(ROOT, "squirrel_motion_planner_amd", "data", "robotino_model.json")
BT = os.path.join(ROOT, "tests", "golden", "room3.bt")


def build_shim(tmpdir):
    exe = os.path.join(str(tmpdir), "shim_scene")
    subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "shim_scene.cpp"), "-L", LIBDIR, "-lsmp_gpu",
                    "-Wl,-rpath," + LIBDIR, "-o", exe], check=True, capture_output=True, text=True)
    return exe


def configs():
    rng = np.random.default_rng(31)
    q = np.column_stack([rng.uniform(-6.0, 6.0, 12), rng.uniform(-6.0, 6.0, 12), rng.uniform(-3.0, 3.0, 12),
                         np.tile([1.0, 0.4, 0.0, 1.2, 0.0], (12, 1))])
    return q


def run_shim(exe, q, want):
    args = [exe, MODEL, BT, str(len(q))] + ["%.17g" % v for v in q.reshape(-1)] + [str(int(w)) for w in want]
    return subprocess.run(args, capture_output=True, text=True, timeout=120)


def test_shim_scene_builds_and_fails_loudly_without_gpu(tmp_path):
    exe = build_shim(tmp_path)
    q = configs()
    p = run_shim(exe, q, np.ones(len(q), np.uint8))
    if p.returncode == 3:
        assert "no usable GPU" in p.stdout or "NO_DEVICE" in p.stdout.upper(), p.stdout
    else:
        assert p.returncode in (0, 1), p.stderr


@pytest.mark.gpu
def test_shim_set_octree_binary_matches_host_path(tmp_path):
    from squirrel_motion_planner_amd.planner import GpuPlanner, Scene
    exe = build_shim(tmp_path)
    q = configs()
    gp = GpuPlanner()
    gp.set_scene(Scene.from_bt(open(BT, "rb").read()))
    want = gp.check_configs(q)
    only_self = gp.check_configs(q, check_map=False)
    assert 0 < want.sum() < len(want) and (only_self > want).any()  # some are invalid because of the map alone
    p = run_shim(exe, q, want)
    assert p.returncode == 0, p.stdout + p.stderr
    assert len(p.stdout.splitlines()) == len(q)
