"""The far-goal calls from C++ (tests/cpp/shim_far.cpp): the host-only part of the C ABI -- smp_far_opts_default,
smp_base_lattice_fit, smp_base_route -- against lattice_restatement.py, which needs no GPU, and smp_node::planFar over
BiRRTstarPlanner::run_planner_far on room3 against the Python mirror's run_planner_far for the same scene, seed and
budget.  CPU: the program builds with -Wall -Werror, links and fails loudly without a GPU."""
import os
import subprocess

import numpy as np
import pytest

import lattice_restatement as T
from conftest import ROOT
from test_shim_clearance import BT, ITERS, LIBDIR, MODEL, SEED, case

PITCH, N_THETA, HANDOVER, MARGIN = 0.2, 4, 0.8, 0.0


def build_shim(tmpdir):
    exe = os.path.join(str(tmpdir), "shim_far")
    subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "shim_far.cpp"), "-L", LIBDIR, "-lsmp_gpu",
                    "-Wl,-rpath," + LIBDIR, "-o", exe], check=True, capture_output=True, text=True)
    return exe


def run_shim(exe, sc):
    args = [exe, MODEL, BT, str(ITERS), str(SEED), "%.17g" % PITCH, str(N_THETA), "%.17g" % HANDOVER, "%.17g" % MARGIN]
    args += ["%.17g" % v for v in list(sc.start) + list(sc.goal) + list(sc.env_x) + list(sc.env_y)]
    return subprocess.run(args, capture_output=True, text=True, timeout=300)


def rows_of(lines, tag, width=8, dtype=np.float64):
    return np.array([[float(v) for v in l.split()[1:]] for l in lines if l.split()[0] == tag], dtype).reshape(-1, width)


def check_host_part(lines):
    head = {l.split()[0]: l.split()[1:] for l in lines if l.split()[0] in ("opts", "fit", "route")}
    assert [float(v) for v in head["opts"]] == [0.1, 8] + list(T.ARM) + [2.0, 0.0, 0, 2]
    lat = T.fit((-1.0, 0.3), (0.5, 1.6), 0.25, 2)
    assert [int(v) for v in head["fit"][:5]] == [0, lat.nx, lat.ny, 2, 1] and (lat.nx, lat.ny) == (6, 5)
    assert [float(v) for v in head["fit"][5:]] == [lat.x0, lat.y0, lat.dtheta]
    free = np.ones((2, 5, 6), bool)
    free[0, :, 3] = False
    exp = T.route(lat, free, T.node_config(lat, 0, 2, 0)[:3], T.node_config(lat, 5, 2, 0)[:3], 0)
    assert exp["status"] == T.OK and sorted(set(exp["chain"][:, 2].tolist())) == [0, 1]
    assert [int(v) for v in head["route"][:4]] == [0, len(exp["chain"]), len(exp["rows"]), exp["n_settled"]]
    assert float(head["route"][4]) == exp["cost"]
    assert np.array_equal(rows_of(lines, "chain", 3, np.int32), exp["chain"])
    assert np.array_equal(rows_of(lines, "rrow"), exp["rows"])


def test_shim_far_builds_and_fails_loudly_without_gpu(tmp_path):
    exe = build_shim(tmp_path)
    p = run_shim(exe, case())
    check_host_part(p.stdout.splitlines())
    if p.returncode == 3:
        assert "no usable GPU" in p.stdout or "NO_DEVICE" in p.stdout.upper(), p.stdout
    else:
        assert p.returncode == 0, p.stderr


@pytest.mark.gpu
def test_shim_matches_the_python_mirror(tmp_path):
    from squirrel_motion_planner_amd.planner import BiRRTstarPlanner
    exe = build_shim(tmp_path)
    sc = case()
    p = run_shim(exe, sc)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.splitlines()
    check_host_part(lines)
    head = {l.split()[0]: l.split()[1:] for l in lines if l.split()[0] in ("status", "far", "waypoints")}
    pl = BiRRTstarPlanner(seed=SEED)
    pl.initialize()
    pl.setOctree(open(BT, "rb").read())
    pl.setPlanningSceneInfo(sc.env_x, sc.env_y)
    assert pl.init_planner(list(sc.start), list(sc.goal), 1, True, True)
    ok = pl.run_planner_far(0, ITERS, pitch=PITCH, n_theta=N_THETA, handover_distance=HANDOVER, map_margin=MARGIN)
    d, far = pl.stats, pl.far_info
    assert ok == (d["status"] == 0) and len(pl.getJointTrajectoryRef()) == (len(d["path"]) if ok else 0)
    print("status", d["status"], {k: far[k] for k in ("stage", "n_route_rows", "handover_node")})
    assert head["status"] == [str(int(d["status"] == 0))]
    assert far["n_route_rows"] > 0  # the case has a base stage
    f = head["far"]
    assert [int(v) for v in f[:6]] == [far["stage"], far["n_route_rows"]] + list(far["handover_node"]) + \
        [far["route"]["n_chain"]]
    assert float(f[6]) == far["route"]["cost"]
    assert [int(v) for v in f[7:]] == [far["map"]["n_nodes"], far["map"]["n_free"], far["check"]["n_edges"],
                                       far["check"]["n_valid"]]
    if d["status"] == 0:
        assert head["waypoints"] == [str(len(d["path"]))]
        assert np.array_equal(rows_of(lines, "row"), d["path"])
    else:
        assert head["waypoints"] == ["0"]
