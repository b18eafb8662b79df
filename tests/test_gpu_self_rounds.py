"""The job tiles' self test in rounds (collide_wide: one item per lane, a sphere's partners in balanced rounds, the
primitives wave-uniform) against the CPU oracle, on configurations where a lost pair, round or lane shows: for every
link pair that is some configuration's only colliding pair, one such configuration -- no other pair rescues its flag.
Every comparison is exact equality of the validity flags; the flat-list form (SMP_SELF_FLAT) must give the same.
"""
import ctypes

import numpy as np
import pytest

from oracle import oracle as O
from squirrel_motion_planner_amd import _lib as L
from squirrel_motion_planner_amd import scenes
from squirrel_motion_planner_amd.planner import GpuPlanner, Robot, Scene

pytestmark = pytest.mark.gpu
_pd = ctypes.POINTER(ctypes.c_double)
CTS = [1, 2, 4, 8]
N_POOL = 20000


@pytest.fixture(scope="module")
def c2():
    return scenes.box_room()


@pytest.fixture(scope="module")
def ref(c2, orobot):
    """The pool and the oracle's verdicts, computed once: the selected set (first sole-collider configuration of every
    link pair that has one, then the pool's first 200) with its self-only flags, and the first 200 with self and map on
    the C2 scene."""
    rng = np.random.default_rng(31)
    pool = np.column_stack([rng.uniform(-1, 1, N_POOL), rng.uniform(-1, 1, N_POOL)] +
                           [rng.uniform(orobot.q_min[j] - 0.3, orobot.q_max[j] + 0.3, N_POOL) for j in range(2, 8)])
    orc = O.Oracle(orobot)
    valid = orc.check_configs(pool, 1, 0).astype(np.uint8)
    lm = np.zeros(orobot.n_links, np.uint8)
    ps = np.zeros(max(orobot.n_pairs, 1), np.uint8)
    first_sole = {}
    seen = np.zeros(len(ps), bool)
    n_sole = 0
    for i in np.flatnonzero(valid == 0):
        O.lib().orc_collisions(orc.h, O._p(np.ascontiguousarray(pool[i]), ctypes.c_double),
                               lm.ctypes.data_as(ctypes.c_void_p), ps.ctypes.data_as(ctypes.c_void_p))
        hit = np.flatnonzero(ps)
        assert len(hit) >= 1
        seen[hit] = True
        if len(hit) == 1:
            n_sole += 1
            first_sole.setdefault(int(hit[0]), int(i))
    idx = np.array(sorted(first_sole.values()) + list(range(200)), np.int64)
    orc_map = O.Oracle(orobot, O.OracleScene(c2.keys, c2.res))
    return {"q": pool[idx], "valid": valid[idx], "sole_pairs": len(first_sole), "n_sole": n_sole,
            "n_colliding": int((valid == 0).sum()), "pairs_seen": int(seen.sum()),
            "q_map": pool[:200], "valid_map": orc_map.check_configs(pool[:200], 1, 1).astype(np.uint8)}


def planner(c2):
    g = GpuPlanner(Robot())
    g.set_scene(Scene.from_keys(c2.keys, c2.res))
    g.set_disabled_map_links([])
    return g


@pytest.fixture(scope="module")
def gp(c2):
    return planner(c2)


@pytest.fixture(scope="module")
def gp_flat(c2):
    """A second planner, created under the switch that keeps its job tiles on the flat pair lists."""
    mp = pytest.MonkeyPatch()
    mp.setenv("SMP_SELF_FLAT", "1")
    try:
        return planner(c2)
    finally:
        mp.undo()


def gpu_flags(gp, q, flags, ct, grid):
    soa = np.ascontiguousarray(np.asarray(q, np.float64).T)
    v = np.full(len(q), 255, np.uint8)
    L.check(L.lib().smp_probe_check_shape(gp.h, soa.ctypes.data_as(_pd), len(q), flags[0], flags[1], -ct, grid,
                                          v.ctypes.data_as(ctypes.c_void_p)))
    return v


def test_inputs_hold_sole_colliders(ref):
    """A condition on the inputs, met by the oracle alone: the pool's colliding configurations, link pairs seen and
    sole colliders, and at least 50 distinct sole-collider link pairs in the selection."""
    assert (ref["n_colliding"], ref["pairs_seen"], ref["n_sole"], ref["sole_pairs"]) == (10321, 143, 1897, 57)
    assert ref["sole_pairs"] >= 50
    assert len(ref["q"]) == ref["sole_pairs"] + 200
    assert int((ref["valid"][:ref["sole_pairs"]] == 0).sum()) == ref["sole_pairs"]


@pytest.mark.parametrize("ct", CTS)
def test_self_flags_equal_the_oracle(gp, ref, ct):
    """Self on, map off: the selected set on 1 and on 7 workgroups, forwards and reversed."""
    assert ref["sole_pairs"] >= 50
    for grid in (1, 7):
        v = gpu_flags(gp, ref["q"], (1, 0), ct, grid)
        assert np.array_equal(v, ref["valid"]), "ct %d grid %d: mismatches at %s" % (
            ct, grid, np.flatnonzero(v != ref["valid"]))
        v = gpu_flags(gp, ref["q"][::-1], (1, 0), ct, grid)
        assert np.array_equal(v, ref["valid"][::-1]), "ct %d grid %d reversed: mismatches at %s" % (
            ct, grid, np.flatnonzero(v != ref["valid"][::-1]))


@pytest.mark.parametrize("ct", CTS)
def test_self_and_map_flags_equal_the_oracle(gp, ref, ct):
    """Self and map on, the C2 scene: the pool's first 200 on 1 and on 7 workgroups, forwards and reversed."""
    for grid in (1, 7):
        v = gpu_flags(gp, ref["q_map"], (1, 1), ct, grid)
        assert np.array_equal(v, ref["valid_map"]), "ct %d grid %d: mismatches at %s" % (
            ct, grid, np.flatnonzero(v != ref["valid_map"]))
        v = gpu_flags(gp, ref["q_map"][::-1], (1, 1), ct, grid)
        assert np.array_equal(v, ref["valid_map"][::-1]), "ct %d grid %d reversed: mismatches at %s" % (
            ct, grid, np.flatnonzero(v != ref["valid_map"][::-1]))


@pytest.mark.parametrize("ct", CTS)
def test_flat_form_gives_the_same_flags(gp, gp_flat, ref, ct):
    """The same sets through a planner created under SMP_SELF_FLAT: identical to the rounds and to the oracle."""
    for grid in (1, 7):
        for q, flags, ov in ((ref["q"], (1, 0), ref["valid"]), (ref["q_map"], (1, 1), ref["valid_map"])):
            vf = gpu_flags(gp_flat, q, flags, ct, grid)
            vr = gpu_flags(gp, q, flags, ct, grid)
            assert np.array_equal(vf, vr), "ct %d grid %d flags %s: forms differ at %s" % (
                ct, grid, flags, np.flatnonzero(vf != vr))
            assert np.array_equal(vf, ov), "ct %d grid %d flags %s: mismatches at %s" % (
                ct, grid, flags, np.flatnonzero(vf != ov))
