"""One-via detours (smp_sample_detours) and path repair (smp_repair_path) against the numpy restatement in
repair_restatement.py: the via configurations and the output waypoints bit for bit, the leg densities, the free flags,
the counters and the costs exactly, with the draws from the oracle's Philox stream and the validity of every point from
the CPU oracle.  test_repair_cpu.py pins, without a GPU, that the inputs are not vacuous."""
import ctypes

import numpy as np
import pytest

import repair_restatement as P
import shortcut_restatement as R
from squirrel_motion_planner_amd import _lib as L
from squirrel_motion_planner_amd.planner import GpuPlanner, Robot, Scene

pytestmark = pytest.mark.gpu
_pd = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def gp():
    return GpuPlanner(Robot())


@pytest.fixture(scope="module")
def gp31():
    return GpuPlanner(Robot(), num_traj_segments=31)


_GSCENES = {}


def use_scene(gp, keys, res, tag):
    if tag not in _GSCENES:
        _GSCENES[tag] = Scene.from_keys(keys, res)
    gp.set_scene(_GSCENES[tag])
    gp.set_disabled_map_links([])


@pytest.mark.parametrize("name", sorted(P.detour_cases()))
def test_sample_detours_parity(gp, gp31, name):
    scn, a, b, samples, h, seed, rnd, n, self_, map_ = P.detour_cases()[name]
    exp = P.detour_expected(name)
    g = gp31 if n == 31 else gp
    assert g.params.num_traj_segments == n
    _, keys, res = P.detour_scene(scn)
    use_scene(g, keys, res, scn)
    got = g.sample_detours(a, b, samples, h, seed=seed, round=rnd, check_self=self_, check_map=map_)
    print(name, "items", exp["free"].size, "free", int(got["free"].sum()), "expected", int(exp["free"].sum()))
    assert got["v"].shape == exp["v"].shape
    assert np.array_equal(got["v"].view(np.uint64), exp["v"].view(np.uint64))  # bit for bit
    assert np.array_equal(got["M1"], exp["M1"]) and np.array_equal(got["M2"], exp["M2"])
    assert np.array_equal(got["free"], exp["free"])


def test_sample_detours_honours_disabled_map_links(gp):
    """One link's map collisions disabled, against the oracle built with the same setting."""
    from oracle import oracle as O
    scn, a, b, samples, h, seed, rnd, _, _, _ = P.detour_cases()["a_blocked_gap"]
    _, keys, res = P.detour_scene(scn)
    link = "shell_base_link_front"
    names = R.orobot().link_names
    assert link in names
    me = np.array([0 if n == link else 1 for n in names], np.uint8)
    want = P.sample_detours(O.Oracle(R.orobot(), O.OracleScene(keys, res), map_enabled=me), a, b, samples, h, seed, rnd)
    assert not np.array_equal(want["free"], P.detour_expected("a_blocked_gap")["free"])
    use_scene(gp, keys, res, scn)
    gp.set_disabled_map_links([link])
    try:
        got = gp.sample_detours(a, b, samples, h, seed=seed, round=rnd)
    finally:
        gp.set_disabled_map_links([])
    assert np.array_equal(got["free"], want["free"])


def test_sample_detours_errors(gp):
    scn, a, b, samples, h, seed, rnd, _, _, _ = P.detour_cases()["b_3x5"]
    _, keys, res = P.detour_scene(scn)
    use_scene(gp, keys, res, scn)
    assert gp.sample_detours(a[:0], b[:0], 4, h)["free"].shape == (0, 4)  # no gap: SMP_OK
    for kw in (dict(samples=0, half_width=h), dict(samples=4, half_width=float("nan"))):
        with pytest.raises(L.SmpError) as e:
            gp.sample_detours(a, b, **kw)
        assert e.value.status == L.SMP_ERR_ARG
    bad = a.copy()
    bad[1, 3] = float("inf")
    with pytest.raises(L.SmpError) as e:
        gp.sample_detours(bad, b, 4, h)
    assert e.value.status == L.SMP_ERR_ARG
    with pytest.raises(L.SmpError) as e:
        gp.sample_detours(np.repeat(a, 6000, 0), np.repeat(b, 6000, 0), 64, h)  # 1 152 000 items
    assert e.value.status == L.SMP_ERR_CAPACITY
    fresh = GpuPlanner(Robot())  # no scene
    with pytest.raises(L.SmpError) as e:
        fresh.sample_detours(a, b, 4, h)
    assert e.value.status == L.SMP_ERR_ARG
    with pytest.raises(L.SmpError) as e:
        fresh.repair_path(P.repair_input("free_path")[0])
    assert e.value.status == L.SMP_ERR_ARG


def run_repair(gp, name):
    w, _, (keys, res) = P.repair_input(name)
    _, scn, samples, rounds, seed = P.REPAIR_CASES[name]
    use_scene(gp, keys, res, scn)
    return w, gp.repair_path(w, samples=samples, rounds=rounds, seed=seed)


@pytest.mark.parametrize("name", ["blocked_case", "late_round", "c2_two_gaps", "c2_mixed_rounds", "free_path"])
def test_repair_parity_with_the_restatement(gp, name):
    exp = P.repair_expected(name)
    assert exp["status"] == P.OK
    w, (path, info) = run_repair(gp, name)
    print(name, {f: info[f] for f in P.INFO}, "rows", len(path), "kernel ms", info["kernel_ms"])
    for f in P.INFO:
        assert info[f] == exp[f], f
    assert path.shape == exp["path"].shape
    assert np.array_equal(path.view(np.uint64), exp["path"].view(np.uint64))
    assert info["kernel_ms"] > 0 and info["total_ms"] >= info["kernel_ms"]


@pytest.mark.parametrize("name", ["stays_blocked", "c2_partly_open", "start_invalid", "goal_invalid"])
def test_repair_failures_match_the_restatement(gp, name):
    exp = P.repair_expected(name)
    assert exp["status"] != P.OK
    with pytest.raises(L.SmpError) as e:
        run_repair(gp, name)
    assert e.value.status == exp["status"]
    info = e.value.info
    print(name, {f: info[f] for f in P.INFO})
    for f in P.INFO:
        assert info[f] == exp[f], f


def test_blocked_through_the_c_abi(gp):
    """Gaps that stay open: SMP_ERR_NO_SOLUTION, first_blocked set, no output buffer; NULL opts are the defaults and a
    NULL info is allowed."""
    name = "stays_blocked"
    exp = P.repair_expected(name)
    w, _, (keys, res) = P.repair_input(name)
    _, scn, samples, rounds, seed = P.REPAIR_CASES[name]
    assert (samples, rounds) == (4, 1)
    use_scene(gp, keys, res, scn)
    ww = np.ascontiguousarray(w)
    out, n_out = _pd(), ctypes.c_int64(7)
    info = L.RepairInfo()
    opts = L.RepairOpts(samples, rounds, seed)
    rc = L.lib().smp_repair_path(gp.h, ww.ctypes.data_as(_pd), len(ww), 1, 1, ctypes.byref(opts), ctypes.byref(out),
                                 ctypes.byref(n_out), ctypes.byref(info))
    assert rc == L.SMP_ERR_NO_SOLUTION and not out and n_out.value == 0
    assert info.first_blocked == exp["first_blocked"] == 1 and info.n_repaired == 0 and info.cost_out == 0.0
    for bad in (L.RepairOpts(0, 1, 1), L.RepairOpts(4, 0, 1)):
        n_out.value = 7
        rc = L.lib().smp_repair_path(gp.h, ww.ctypes.data_as(_pd), len(ww), 1, 1, ctypes.byref(bad), ctypes.byref(out),
                                     ctypes.byref(n_out), None)
        assert rc == L.SMP_ERR_ARG and not out and n_out.value == 0
    rc = L.lib().smp_repair_path(gp.h, ww.ctypes.data_as(_pd), 1, 1, 1, None, ctypes.byref(out), ctypes.byref(n_out),
                                 None)
    assert rc == L.SMP_ERR_ARG
    nan = ww.copy()
    nan[3, 0] = float("nan")
    rc = L.lib().smp_repair_path(gp.h, nan.ctypes.data_as(_pd), len(nan), 1, 1, None, ctypes.byref(out),
                                 ctypes.byref(n_out), None)
    assert rc == L.SMP_ERR_ARG
    # NULL opts: samples 256, rounds 4, seed 1 -- the same call as the wrapper's defaults
    rc = L.lib().smp_repair_path(gp.h, ww.ctypes.data_as(_pd), len(ww), 1, 1, None, ctypes.byref(out),
                                 ctypes.byref(n_out), None)
    assert rc == L.SMP_OK and out and n_out.value > len(ww)
    try:
        rows = np.ctypeslib.as_array(out, shape=(n_out.value, 8)).copy()
    finally:
        L.lib().smp_buffer_free(out)
    path, info = gp.repair_path(w)
    assert np.array_equal(rows, path) and info["n_items"] % 256 == 0


@pytest.mark.parametrize("name", ["blocked_case", "c2_two_gaps"])
def test_output_is_usable(gp, name):
    """Every output row is free by the planner's checker and by the oracle, every hop is one planner step at most
    (m = 1) and free as an edge of its own; on the blocked_case scene smp_shortcut_path, which alone reports the path
    blocked, shortens the repaired one."""
    w, (path, info) = run_repair(gp, name)
    _, orc, _ = P.repair_input(name)
    assert orc.check_configs(path).all()
    assert gp.check_configs(path).all()
    m, _ = R.density(path[:-1], path[1:], R.orobot().rev, R.N_SEG, R.STEP)
    assert (m == 1).all()
    first, npts = gp.check_edges(path[:-1], path[1:])
    assert (first == -1).all() and (npts == R.N_SEG + 1).all()
    if name == "blocked_case":
        with pytest.raises(L.SmpError) as e:
            gp.shortcut_path(w)
        assert e.value.status == L.SMP_ERR_NO_SOLUTION
    short, sinfo = gp.shortcut_path(path)  # SMP_OK
    # the repaired path itself is one of the candidates' routes; its hops sum to cost_out up to the rounding of the via
    # nodes (a few ulp per hop)
    assert sinfo["first_blocked"] == -1 and sinfo["cost_out"] <= info["cost_out"] * (1 + 1e-12)
    assert gp.check_configs(short).all()
