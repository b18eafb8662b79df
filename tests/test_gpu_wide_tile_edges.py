"""Edge shapes of the job tiles (collide_wide): one workgroup keeps its per-lane robot and scene constants in registers
for all the tiles it runs, so the smallest shapes at which that can go wrong are checked against the CPU oracle on the
C2 scene: partial and single tiles (a full tile after a partial one included), colliding and free configurations
strictly alternating (state left over from the tile or the configuration before), and the same batch on one and on
several workgroups.  Every comparison is exact equality of the validity flags.
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
FLAGS = [(1, 1), (1, 0), (0, 1)]
CTS = [1, 2, 4, 8]


def random_configs(sc, n, seed, orobot):
    rng = np.random.default_rng(seed)
    (x0, x1), (y0, y1) = sc.env_x, sc.env_y
    return np.column_stack([rng.uniform(x0, x1, n), rng.uniform(y0, y1, n)] +
                           [rng.uniform(orobot.q_min[j] - 0.3, orobot.q_max[j] + 0.3, n) for j in range(2, 8)])


@pytest.fixture(scope="module")
def c2():
    return scenes.box_room()


@pytest.fixture(scope="module")
def gp(c2):
    g = GpuPlanner(Robot())
    g.set_scene(Scene.from_keys(c2.keys, c2.res))
    g.set_disabled_map_links([])
    return g


@pytest.fixture(scope="module")
def ref(c2, orobot):
    """The oracle's flags, computed once: 200 random configurations under every flag pair (the first 25 serve the
    partial tiles), and the alternating sequence of 64 (colliding, free, colliding, ...) with self and map on."""
    orc = O.Oracle(orobot, O.OracleScene(c2.keys, c2.res))
    q = random_configs(c2, 200, 21, orobot)
    valid = {f: orc.check_configs(q, *f).astype(np.uint8) for f in FLAGS}
    pool = random_configs(c2, 2000, 22, orobot)
    pv = orc.check_configs(pool, 1, 1).astype(np.uint8)
    hit, free = np.flatnonzero(pv == 0)[:32], np.flatnonzero(pv != 0)[:32]
    assert len(hit) == 32 and len(free) == 32
    idx = np.empty(64, np.int64)
    idx[0::2], idx[1::2] = hit, free
    alt_v = pv[idx]
    assert np.array_equal(alt_v, np.tile(np.array([0, 1], np.uint8), 32))
    assert int((alt_v == 0).sum()) == int((alt_v == 1).sum()) == 32
    return {"q": q, "valid": valid, "alt_q": pool[idx], "alt_valid": alt_v}


def gpu_flags(gp, q, flags, ct, grid):
    soa = np.ascontiguousarray(np.asarray(q, np.float64).T)
    v = np.full(len(q), 255, np.uint8)
    L.check(L.lib().smp_probe_check_shape(gp.h, soa.ctypes.data_as(_pd), len(q), flags[0], flags[1], -ct, grid,
                                          v.ctypes.data_as(ctypes.c_void_p)))
    return v


def tile_counts(ct):
    return sorted({n for n in (1, ct - 1, ct, ct + 1, 3 * ct + 1) if n > 0})


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("ct", CTS)
def test_partial_and_single_tiles(gp, ref, ct, flags):
    """n = 1, ct - 1, ct, ct + 1, 3 ct + 1 configurations on one workgroup: it runs all the tiles in sequence."""
    for n in tile_counts(ct):
        v = gpu_flags(gp, ref["q"][:n], flags, ct, 1)
        ov = ref["valid"][flags][:n]
        assert np.array_equal(v, ov), "ct %d n %d flags %s: gpu %s oracle %s" % (ct, n, flags, v, ov)
        # a full tile after a partial one: the same workgroup, the tiles' order reversed
        v = gpu_flags(gp, ref["q"][:n][::-1], flags, ct, 1)
        assert np.array_equal(v, ov[::-1]), "ct %d n %d flags %s reversed: gpu %s oracle %s" % (ct, n, flags, v, ov[::-1])


@pytest.mark.parametrize("ct", CTS)
def test_alternating_outcomes(gp, ref, ct):
    """64 configurations strictly alternating colliding / free on one workgroup, forwards and reversed."""
    q, ov = ref["alt_q"], ref["alt_valid"]
    assert int((ov == 0).sum()) == int((ov == 1).sum()) == 32 and np.all(ov[1:] != ov[:-1])
    v = gpu_flags(gp, q, (1, 1), ct, 1)
    assert np.array_equal(v, ov), "ct %d: mismatches at %s" % (ct, np.flatnonzero(v != ov))
    v = gpu_flags(gp, q[::-1], (1, 1), ct, 1)
    assert np.array_equal(v, ov[::-1]), "ct %d reversed: mismatches at %s" % (ct, np.flatnonzero(v != ov[::-1]))


@pytest.mark.parametrize("ct", [8, 1])
def test_block_count_independence(gp, ref, ct):
    """200 random configurations on 1 and on 7 workgroups: identical to each other and to the oracle."""
    for flags in FLAGS:
        v1 = gpu_flags(gp, ref["q"], flags, ct, 1)
        v7 = gpu_flags(gp, ref["q"], flags, ct, 7)
        ov = ref["valid"][flags]
        assert np.array_equal(v1, v7), "ct %d flags %s: grids differ at %s" % (ct, flags, np.flatnonzero(v1 != v7))
        assert np.array_equal(v1, ov), "ct %d flags %s: mismatches at %s" % (ct, flags, np.flatnonzero(v1 != ov))
