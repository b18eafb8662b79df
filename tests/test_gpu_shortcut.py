"""Path shortcutting (smp_shortcut_path) against the numpy restatement in shortcut_restatement.py: the output waypoints
bit for bit, the counters and costs exactly, with the validity of every point taken from the CPU oracle."""
import numpy as np
import pytest

import shortcut_restatement as R
from squirrel_motion_planner_amd import _lib as L
from squirrel_motion_planner_amd.planner import GpuPlanner, Robot, Scene

pytestmark = pytest.mark.gpu
FIELDS = ("n_edges", "n_valid", "configs_checked", "cost_in", "cost_out", "first_blocked")


@pytest.fixture(scope="module")
def gp():
    return GpuPlanner(Robot())


_GSCENES = {}


def use_scene(gp, name):
    if name not in _GSCENES:
        sc, _ = R.scene(name)
        _GSCENES[name] = Scene.from_keys(sc.keys, sc.res)
    gp.set_scene(_GSCENES[name])
    gp.set_disabled_map_links([])


def nonadjacent(exp):
    return np.array([f for (i, j), f in zip(exp["pairs"], exp["first"]) if j - i > 1])


@pytest.mark.parametrize("name", ["c2", "c4"])
def test_parity_with_the_restatement(gp, name):
    w = R.shortcut_input(name)
    exp = R.shortcut_expected(name)
    assert len(w) <= 12 and exp["path"] is not None
    na = nonadjacent(exp)
    assert (na < 0).any() and (na >= 0).any()  # a shortcut exists, and one is refused
    if name == "c2":
        assert exp["cost_out"] < exp["cost_in"]
    use_scene(gp, name)
    path, info = gp.shortcut_path(w)
    print(name, {f: info[f] for f in FIELDS}, "rows", len(path), "kernel ms", info["kernel_ms"])
    for f in FIELDS:
        assert info[f] == exp[f], f
    assert path.shape == exp["path"].shape
    assert np.array_equal(path, exp["path"])
    assert info["kernel_ms"] > 0 and info["total_ms"] >= info["kernel_ms"]


@pytest.mark.parametrize("name", ["c2", "c4"])
def test_output_is_valid_again(gp, name):
    """Every output row is free, every hop is at most one planner step (m = 1), and the hops checked as edges of their
    own are free."""
    use_scene(gp, name)
    path, _ = gp.shortcut_path(R.shortcut_input(name))
    assert R.oracle_for(name).check_configs(path).all()
    assert gp.check_configs(path).all()
    m, _ = R.density(path[:-1], path[1:], R.orobot().rev, R.N_SEG, R.STEP)
    assert (m == 1).all()
    first, npts = gp.check_edges(path[:-1], path[1:])
    assert (first == -1).all() and (npts == R.N_SEG + 1).all()


def test_window_two(gp):
    name = "c2"
    exp = R.shortcut_expected(name, 2)
    full = R.shortcut_expected(name)
    assert exp["path"] is not None and exp["n_edges"] == 2 * len(R.shortcut_input(name)) - 3
    assert exp["cost_out"] != full["cost_out"] and not np.array_equal(exp["path"], full["path"])
    use_scene(gp, name)
    path, info = gp.shortcut_path(R.shortcut_input(name), window=2)
    for f in FIELDS:
        assert info[f] == exp[f], f
    assert np.array_equal(path, exp["path"])
    path_full, _ = gp.shortcut_path(R.shortcut_input(name))
    assert not np.array_equal(path, path_full)


def test_blocked_path(gp):
    """A box on the straight stretch of the empty room's path (R.blocked_case): both end waypoints stay valid, no
    route remains."""
    w, keys, res, exp, valid = R.blocked_case()
    assert valid[0] and valid[-1] and exp["path"] is None and exp["first_blocked"] >= 0
    gp.set_scene(Scene.from_keys(keys, res))
    gp.set_disabled_map_links([])
    with pytest.raises(L.SmpError) as e:
        gp.shortcut_path(w)
    assert e.value.status == L.SMP_ERR_NO_SOLUTION
    info = e.value.info
    print({f: info[f] for f in FIELDS})
    for f in FIELDS:
        assert info[f] == exp[f], f
    # no output through the C ABI either
    import ctypes
    pd = ctypes.POINTER(ctypes.c_double)
    out, n_out = pd(), ctypes.c_int64(7)
    ww = np.ascontiguousarray(w)
    rc = L.lib().smp_shortcut_path(gp.h, ww.ctypes.data_as(pd), len(ww), 1, 1, 0, ctypes.byref(out), ctypes.byref(n_out),
                                   None)
    assert rc == L.SMP_ERR_NO_SOLUTION and not out and n_out.value == 0


def test_two_waypoints_and_one(gp):
    """k = 2: the single candidate, free, with its via nodes inserted.  k = 1: an argument error."""
    name = "c4"
    w = R.shortcut_input(name)
    exp = R.shortcut_expected(name)
    e = next(k for k, ((i, j), f) in enumerate(zip(exp["pairs"], exp["first"])) if f < 0 and exp["m"][k] >= 2)
    i, j = exp["pairs"][e]
    two = np.array([w[i], w[j]])
    want = R.shortcut(R.oracle_for(name), two, R.orobot().rev, R.N_SEG, R.STEP)
    assert want["n_edges"] == 1 and len(want["path"]) == exp["m"][e] + 1
    use_scene(gp, name)
    path, info = gp.shortcut_path(two)
    assert info["n_edges"] == 1 and info["n_valid"] == 1
    assert np.array_equal(path, want["path"])
    with pytest.raises(L.SmpError) as err:
        gp.shortcut_path(two[:1])
    assert err.value.status == L.SMP_ERR_ARG
