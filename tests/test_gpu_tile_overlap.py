"""The job tiles' last stage (collide_wide: prefilter, candidates, brick words, exact sweeps and the self test, in
whatever order they are issued) against the CPU oracle, on configurations where a lost candidate, a brick word at the
wrong slot, a skipped primitive or state left over by a tile that stopped early shows: a flag is map or self, and here
no second collision rescues it.  Every comparison is exact equality of the validity flags, for 1, 2, 4 and 8
configurations per tile, on 1 and on 7 workgroups, forwards and reversed.
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
N_DENSE = 200
FAR = 50.0  # metres: every centre cell of a configuration moved there is outside the grid


def draw(rng, sc, orobot, n):
    """n configurations: all x, then all y (uniform over the scene's sampling bounds), then joint by joint (uniform
    over the limits widened by 0.3)."""
    return np.column_stack([rng.uniform(*sc.env_x, n), rng.uniform(*sc.env_y, n)] +
                           [rng.uniform(orobot.q_min[j] - 0.3, orobot.q_max[j] + 0.3, n) for j in range(2, 8)])


@pytest.fixture(scope="module")
def c2():
    return scenes.box_room()


@pytest.fixture(scope="module")
def c5():
    return scenes.clutter_cloud()


@pytest.fixture(scope="module")
def ref(c2, orobot):
    """Pool 1 on the C2 scene and the oracle's verdicts, computed once."""
    pool = draw(np.random.default_rng(41), c2, orobot, N_POOL)
    orc = O.Oracle(orobot, O.OracleScene(c2.keys, c2.res))
    v_self = orc.check_configs(pool, 1, 0).astype(np.uint8)
    v_map = orc.check_configs(pool, 0, 1).astype(np.uint8)
    map_only = np.flatnonzero((v_self == 1) & (v_map == 0))
    lm = np.zeros(orobot.n_links, np.uint8)
    ps = np.zeros(max(orobot.n_pairs, 1), np.uint8)
    seen = np.zeros(orobot.n_links, bool)
    first_sole = {}
    n_sole = 0
    for i in map_only:
        O.lib().orc_collisions(orc.h, O._p(np.ascontiguousarray(pool[i]), ctypes.c_double),
                               lm.ctypes.data_as(ctypes.c_void_p), ps.ctypes.data_as(ctypes.c_void_p))
        hit = np.flatnonzero(lm)
        assert len(hit) >= 1
        seen[hit] = True
        if len(hit) == 1 and not ps.any():
            n_sole += 1
            first_sole.setdefault(int(hit[0]), int(i))
    idx = np.array(sorted(first_sole.values()) + list(range(200)), np.int64)
    r = {"n_map_only": len(map_only), "links_seen": int(seen.sum()), "n_sole": n_sole,
         "sole_links": sorted(orobot.link_names[l] for l in first_sole),
         "prim_links": {orobot.link_names[l] for l in orobot.prim_link[:orobot.n_prim]},
         "q": pool[idx], "n_sel": len(first_sole)}
    r["valid"] = {(0, 1): v_map[idx], (1, 1): orc.check_configs(pool[idx], 1, 1).astype(np.uint8)}
    # outside the grid: 8 self colliders and 8 self-free configurations of the pool, moved far away
    far = pool[np.concatenate([np.flatnonzero(v_self == 0)[:8], np.flatnonzero(v_self == 1)[:8]])].copy()
    far[:, 0] = FAR
    far[:, 1] = FAR
    r["q_far"] = far
    r["valid_far"] = orc.check_configs(far, 1, 1).astype(np.uint8)
    r["valid_far_self"] = orc.check_configs(far, 1, 0).astype(np.uint8)
    # early exits against leftovers: self collides and map free, map collides and self free, strictly alternating
    a = np.flatnonzero((v_self == 0) & (v_map == 1))[:32]
    b = map_only[:32]
    alt = np.empty(len(a) + len(b), np.int64)
    alt[0::2] = a
    alt[1::2] = b
    r["n_alt"] = (len(a), len(b))
    r["q_alt"] = pool[alt]
    r["valid_alt"] = orc.check_configs(pool[alt], 1, 1).astype(np.uint8)
    return r


@pytest.fixture(scope="module")
def ref_dense(c5, orobot):
    """200 configurations on the 2 cm scene and the oracle's verdicts (its exhaustive sweep: about 20 s)."""
    q = draw(np.random.default_rng(43), c5, orobot, N_DENSE)
    orc = O.Oracle(orobot, O.OracleScene(c5.keys, c5.res))
    return {"q": q, "valid": {f: orc.check_configs(q, *f).astype(np.uint8) for f in ((0, 1), (1, 1))}}


def planner(sc):
    g = GpuPlanner(Robot())
    g.set_scene(Scene.from_keys(sc.keys, sc.res))
    g.set_disabled_map_links([])
    return g


@pytest.fixture(scope="module")
def gp(c2):
    return planner(c2)


@pytest.fixture(scope="module")
def gp_dense(c5):
    return planner(c5)


def gpu_flags(gp, q, flags, ct, grid):
    soa = np.ascontiguousarray(np.asarray(q, np.float64).T)
    v = np.full(len(q), 255, np.uint8)
    L.check(L.lib().smp_probe_check_shape(gp.h, soa.ctypes.data_as(_pd), len(q), flags[0], flags[1], -ct, grid,
                                          v.ctypes.data_as(ctypes.c_void_p)))
    return v


def both_ways(gp, q, flags, ov, ct, grids=(1, 7)):
    for grid in grids:
        v = gpu_flags(gp, q, flags, ct, grid)
        assert np.array_equal(v, ov), "ct %d grid %d flags %s: mismatches at %s" % (ct, grid, flags, np.flatnonzero(v != ov))
        v = gpu_flags(gp, q[::-1], flags, ct, grid)
        assert np.array_equal(v, ov[::-1]), "ct %d grid %d flags %s reversed: mismatches at %s" % (
            ct, grid, flags, np.flatnonzero(v != ov[::-1]))


def test_inputs_hold_sole_map_colliders(ref):
    """A condition on the inputs, met by the oracle alone: the pool's map-only colliders, the links seen among them,
    the sole colliders, and at least 8 distinct sole links in the selection, a primitive link among them."""
    assert (ref["n_map_only"], ref["links_seen"], ref["n_sole"], ref["n_sel"]) == (3954, 27, 681, 9)
    assert ref["n_sel"] >= 8
    assert {"shell_base_link", "shell_base_link_front"} <= set(ref["sole_links"])
    assert ref["prim_links"] & set(ref["sole_links"])
    assert len(ref["q"]) == ref["n_sel"] + 200
    assert int((ref["valid"][(0, 1)][:ref["n_sel"]] == 0).sum()) == ref["n_sel"]


@pytest.mark.parametrize("ct", CTS)
def test_sole_map_colliders_equal_the_oracle(gp, ref, ct):
    """C2 scene: the first sole map collider of every link that has one, then the pool's first 200, with the map alone
    and with self and map."""
    assert ref["n_sel"] >= 8 and ref["prim_links"] & set(ref["sole_links"])
    for flags in ((0, 1), (1, 1)):
        both_ways(gp, ref["q"], flags, ref["valid"][flags], ct)


def test_dense_inputs_hold_free_and_colliding(ref_dense):
    v = ref_dense["valid"]
    assert (int(v[(0, 1)].sum()), int(v[(1, 1)].sum())) == (24, 15)
    assert int(v[(0, 1)].sum()) >= 20 and int((v[(0, 1)] == 0).sum()) >= 100


@pytest.mark.parametrize("ct", CTS)
def test_dense_scene_equals_the_oracle(gp_dense, ref_dense, ct):
    """2 cm scene: many candidates per configuration, the staging buffer filling, candidates that do not fit it and
    primitives whose reach exceeds 64 bricks."""
    assert int(ref_dense["valid"][(0, 1)].sum()) >= 20
    for flags in ((0, 1), (1, 1)):
        both_ways(gp_dense, ref_dense["q"], flags, ref_dense["valid"][flags], ct)


def test_far_and_alternating_inputs(ref):
    """Conditions on the inputs of the two tests below, met by the oracle alone: far away the map is silent and the
    self test keeps its 8 colliding and 8 free; the alternating sequence has 32 of either kind, all colliding."""
    assert int((ref["valid_far"] == 0).sum()) == 8 and int((ref["valid_far"] == 1).sum()) == 8
    assert np.array_equal(ref["valid_far"], ref["valid_far_self"])
    assert ref["n_alt"] == (32, 32)
    assert np.array_equal(ref["valid_alt"], np.zeros(64, np.uint8))


@pytest.mark.parametrize("ct", CTS)
def test_outside_the_grid_stays_self_only(gp, ref, ct):
    """Moved to x = y = 50 m no centre has a cell: with the map on, the flags are the self test's."""
    assert int((ref["valid_far"] == 0).sum()) == 8
    both_ways(gp, ref["q_far"], (1, 1), ref["valid_far"], ct)


@pytest.mark.parametrize("ct", CTS)
def test_early_exits_leave_nothing_behind(gp, ref, ct):
    """One workgroup, self colliders and map colliders strictly alternating: a tile that stopped after its first half
    leaves no candidate, brick word or slot that the next one reads."""
    assert ref["n_alt"] == (32, 32)
    both_ways(gp, ref["q_alt"], (1, 1), ref["valid_alt"], ct, grids=(1,))
