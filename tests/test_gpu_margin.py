"""The margin checks (smp_check_configs_margin, smp_check_edges_margin, smp_sample_detours_margin,
smp_shortcut_path_margin, smp_repair_path_margin) against margin_restatement.py: the CPU oracle's validity and the
clearance restatement's distances compared with the margin, carried through the restatements of the path passes.  Flags,
indices, counters and costs exactly; via configurations and output rows bit for bit.  test_margin_cpu.py pins, on the
CPU, that these inputs hold every kind of answer."""
import ctypes

import numpy as np
import pytest

import clearance_restatement as C
import gpu_info
import margin_restatement as G
import repair_restatement as P
import shortcut_restatement as R
from squirrel_motion_planner_amd import _lib as L
from squirrel_motion_planner_amd.planner import GpuPlanner, Robot, Scene

pytestmark = pytest.mark.gpu
_pd = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def gp():
    return GpuPlanner(Robot())


_GSCENES = {}


def use_scene(gp, name, disabled=()):
    if name not in _GSCENES:
        if name == "blocked":
            _, keys, res = P.detour_scene("blocked")
        else:
            sc, _ = R.scene(name)
            keys, res = sc.keys, sc.res
        _GSCENES[name] = Scene.from_keys(keys, res)
    gp.set_scene(_GSCENES[name])
    gp.set_disabled_map_links(list(disabled))


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ------------------------------------------------------------------------------------------ check_clear
@pytest.mark.parametrize("name", G.SCENES)
@pytest.mark.parametrize("margin", G.POSE_MARGINS)
@pytest.mark.parametrize("n", [1, 33, 97])
def test_check_clear(gp, name, margin, n):
    exp = G.poses_expected(name, *margin)[:n]
    use_scene(gp, name)
    got = gp.check_clear(C.poses(name)[:n], margin=margin)
    bad = np.flatnonzero(got != exp)
    assert len(bad) == 0, (bad[:8], got[bad[:8]], exp[bad[:8]])


@pytest.mark.parametrize("name", G.SCENES)
@pytest.mark.parametrize("margin", G.POSE_MARGINS)
def test_check_clear_each_flag_alone(gp, name, margin):
    use_scene(gp, name)
    q = C.poses(name)
    for self_, map_ in ((True, False), (False, True), (False, False)):
        got = gp.check_clear(q, self_, map_, margin=margin)
        assert np.array_equal(got, G.poses_expected(name, *margin, self_, map_)), (self_, map_)


@pytest.mark.parametrize("name", G.SCENES)
@pytest.mark.parametrize("margin", G.POSE_MARGINS)
def test_check_clear_disabled_arm_link(gp, name, margin):
    exp = G.poses_expected(name, *margin, disabled=True)
    use_scene(gp, name, [C.DISABLED_LINK])
    try:
        got = gp.check_clear(C.poses(name), margin=margin)
    finally:
        gp.set_disabled_map_links([])
    assert np.array_equal(got, exp)


# ------------------------------------------------------------------------------------------ check_edges
@pytest.mark.parametrize("name", G.SCENES)
@pytest.mark.parametrize("margin", G.EDGE_MARGINS)
def test_check_edges(gp, name, margin):
    a, b = C.edges(name)
    first, M = G.edges_expected(name, *margin)
    use_scene(gp, name)
    got, npts = gp.check_edges(a, b, margin=margin)
    print(name, margin, "first", got.tolist())
    assert np.array_equal(got, first)
    assert np.array_equal(npts, M + 1)


def test_more_edges_than_workgroups(gp):
    """The table repeated until it holds more edges than twice the CU count, so that every workgroup goes round the
    work loop more than once."""
    name, margin = "c2", (0.02, 0.0)
    a, b = C.edges(name)
    first, M = G.edges_expected(name, *margin)
    reps = 2 * gpu_info.device_cus() // len(a) + 1
    use_scene(gp, name)
    got, npts = gp.check_edges(np.tile(a, (reps, 1)), np.tile(b, (reps, 1)), margin=margin)
    assert len(got) > 2 * gpu_info.device_cus()
    assert np.array_equal(got, np.tile(first, reps)) and np.array_equal(npts, np.tile(M + 1, reps))


# ------------------------------------------------------------------------------------------ zero margin
@pytest.mark.parametrize("margin", [None, (0.0, 0.0)])
def test_zero_margin_is_the_plain_call(gp, margin):
    """A NULL or zero margin equals the plain entry point in every output field, for all five calls."""
    name = "c2"
    use_scene(gp, name)
    q = C.poses(name)
    assert np.array_equal(gp.check_clear(q, margin=margin), gp.check_configs(q))
    a, b = C.edges(name)
    f0, n0 = gp.check_edges(a, b)
    if margin is None:  # (the keyword's None is the plain entry point itself: hand the margin call a NULL pointer)
        f1, n1 = np.zeros(len(a), np.int64), np.zeros(len(a), np.int32)
        ra, rb = np.ascontiguousarray(a), np.ascontiguousarray(b)
        L.check(L.lib().smp_check_edges_margin(gp.h, ra.ctypes.data_as(_pd), rb.ctypes.data_as(_pd), len(a), 1, 1, None,
                                               f1.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                               n1.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))),
                "smp_check_edges_margin")
    else:
        f1, n1 = gp.check_edges(a, b, margin=margin)
    assert np.array_equal(f0, f1) and np.array_equal(n0, n1)
    margin = (0.0, 0.0)  # the remaining calls through the margin entry points
    scn, ga, gb, samples, h, seed, rnd, _, _, _ = P.detour_cases()["b_3x5"]
    d0 = gp.sample_detours(ga, gb, samples, h, seed=seed, round=rnd)
    d1 = gp.sample_detours(ga, gb, samples, h, seed=seed, round=rnd, margin=margin)
    assert all(np.array_equal(d0[k], d1[k]) for k in d0) and same_bits(d0["v"], d1["v"])
    w = C.path12()
    times = ("kernel_ms", "total_ms")
    p0, i0 = gp.shortcut_path(w)
    p1, i1 = gp.shortcut_path(w, margin=margin)
    assert same_bits(p0, p1) and all(i0[k] == i1[k] for k in i0 if k not in times)
    w = P.c2_colliding_path()
    p0, i0 = gp.repair_path(w, samples=64, rounds=3, seed=1)
    p1, i1 = gp.repair_path(w, samples=64, rounds=3, seed=1, margin=margin)
    assert same_bits(p0, p1) and all(i0[k] == i1[k] for k in i0 if k not in times)


# ------------------------------------------------------------------------------------------ detours
@pytest.mark.parametrize("margin", [(0.02, 0.0), (0.02, 0.02)])
def test_sample_detours(gp, margin):
    scn, a, b, samples, h, seed, rnd, _, self_, map_ = P.detour_cases()["a_blocked_gap"]
    exp = G.detours_expected("a_blocked_gap", *margin)
    use_scene(gp, scn)
    got = gp.sample_detours(a, b, samples, h, seed=seed, round=rnd, check_self=self_, check_map=map_, margin=margin)
    print(margin, "free", int(got["free"].sum()), "expected", int(exp["free"].sum()))
    assert same_bits(got["v"], exp["v"])
    assert np.array_equal(got["M1"], exp["M1"]) and np.array_equal(got["M2"], exp["M2"])
    assert np.array_equal(got["free"], exp["free"])


# ------------------------------------------------------------------------------------------ the pipeline
def test_pipeline(gp):
    """Repair at a map margin of 2 cm, then the all-pairs shortcut at the same margin; every adjacent edge of the final
    route is more than 2 cm clear by smp_clearance_edges."""
    margin = G.PIPE_MARGIN
    rep, cut = G.pipeline_repair(), G.pipeline_shortcut()
    use_scene(gp, "c2")
    w = C.path12()
    with pytest.raises(L.SmpError) as e:
        gp.shortcut_path(w, margin=margin)
    assert e.value.status == L.SMP_ERR_NO_SOLUTION and e.value.info["first_blocked"] == 3
    path, info = gp.repair_path(w, samples=G.PIPE_SAMPLES, rounds=4, seed=1, margin=margin)
    print({f: info[f] for f in P.INFO}, "rows", len(path), "kernel ms", info["kernel_ms"])
    for f in P.INFO:
        assert info[f] == rep[f], f
    assert same_bits(path, rep["path"])
    short, sinfo = gp.shortcut_path(path, margin=margin)
    print({f: sinfo[f] for f in ("n_edges", "n_valid", "cost_in", "cost_out")}, "kernel ms", sinfo["kernel_ms"])
    assert same_bits(short, cut["path"])
    for f in ("n_edges", "n_valid", "configs_checked", "cost_in", "cost_out", "first_blocked"):
        assert sinfo[f] == cut[f], f
    _, plain = gp.shortcut_path(path)
    assert sinfo["cost_out"] != plain["cost_out"]
    e = gp.edge_clearance(short[:-1], short[1:], 0.3)
    print("least map clearance", float(e["map"].min()))
    assert (e["map"] > margin[0]).all()


def test_unclear_start(gp):
    use_scene(gp, "c2")
    with pytest.raises(L.SmpError) as e:
        gp.repair_path(C.path12(), samples=G.PIPE_SAMPLES, margin=(0.05, 0.0))
    assert e.value.status == L.SMP_ERR_START_INVALID


def test_no_solution(gp):
    use_scene(gp, "c2")
    with pytest.raises(L.SmpError) as e:
        gp.repair_path(C.path12(), samples=64, rounds=4, margin=(0.03, 0.02))
    assert e.value.status == L.SMP_ERR_NO_SOLUTION
    assert e.value.info["first_blocked"] == 0 and e.value.info["n_items"] == 256 and e.value.info["n_free"] == 0


# ------------------------------------------------------------------------------------------ argument errors
def test_argument_errors(gp):
    use_scene(gp, "c2")
    q = C.poses("c2")[:4]
    a, b = C.edges("c2")
    w = C.path12()
    fresh = GpuPlanner(Robot())  # no scene
    calls = (lambda g, m: g.check_clear(q, margin=m), lambda g, m: g.check_edges(a[:2], b[:2], margin=m),
             lambda g, m: g.sample_detours(a[:1], b[:1], 4, 0.5, margin=m), lambda g, m: g.shortcut_path(w, margin=m),
             lambda g, m: g.repair_path(w, samples=4, rounds=1, margin=m))
    for call in calls:
        for m in ((float("nan"), 0.0), (0.0, float("inf")), (-0.01, 0.0), (0.0, -1.0), (20.0, 0.0)):
            with pytest.raises(L.SmpError) as e:
                call(gp, m)
            assert e.value.status == L.SMP_ERR_ARG, m
        with pytest.raises(L.SmpError) as e:
            call(fresh, (0.02, 0.0))
        assert e.value.status == L.SMP_ERR_ARG


def test_margin_of_metres(gp):
    """A margin below the clamp is a valid one however wide: the items' reach is then most of the grid."""
    q = C.poses("c2")[:4]
    exp = G.oracle("c2", 3.0, 0.0).check_configs(q)
    assert not exp.any()  # (nowhere in the room is 3 m from the floor)
    use_scene(gp, "c2")
    assert np.array_equal(gp.check_clear(q, margin=(3.0, 0.0)), exp)
