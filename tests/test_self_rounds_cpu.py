"""The round schedule of the job tiles' self test (RobotDev::sr_*, smp_robot_self_rounds) against the model's flat
self-collision lists: every sphere pair in exactly one (lane, round) slot with its threshold's bits, the primitive masks
equal to the (primitive, sphere) list, the rounds balanced, and a model with more than one item per lane left on the
flat lists.  Host code only.
"""
import collections
import ctypes
import json
import math
import os

import numpy as np
import pytest

from squirrel_motion_planner_amd import _lib as L
from squirrel_motion_planner_amd.planner import Robot

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _description():
    return (open(os.path.join(GOLD, "robotino_plan.urdf")).read(), open(os.path.join(GOLD, "robotino_plan.srdf")).read())


def schedule(robot):
    info = (ctypes.c_int32 * 8)()
    L.check(L.lib().smp_robot_self_rounds(robot.h, info, None, None, None, None, None, None))
    n_sph, n_prim, n_sp, n_pp, ok, rounds, lanes, max_rounds = info
    v = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    s = {"n_sph": n_sph, "n_prim": n_prim, "ok": ok, "rounds": rounds, "lanes": lanes, "max_rounds": max_rounds,
         "sp_ab": np.zeros(n_sp, np.uint16), "sp_rr2": np.zeros(n_sp), "pp_ps": np.zeros(n_pp, np.uint16),
         "partner": np.zeros(lanes * max_rounds, np.int32), "rr2": np.zeros(lanes * max_rounds),
         "mask": np.zeros(n_sph, np.uint32)}
    L.check(L.lib().smp_robot_self_rounds(robot.h, info, v(s["sp_ab"]), v(s["sp_rr2"]), v(s["pp_ps"]), v(s["partner"]),
                                          v(s["rr2"]), v(s["mask"])))
    s["partner"] = s["partner"].reshape(lanes, max_rounds)
    s["rr2"] = s["rr2"].reshape(lanes, max_rounds)
    return s


@pytest.fixture(scope="module", params=["json", "urdf"])
def sched(request):
    return schedule(Robot() if request.param == "json" else Robot.from_urdf(*_description()))


def test_every_pair_in_one_slot_with_its_threshold(sched):
    s = sched
    flat = {}
    for ab, rr2 in zip(s["sp_ab"].tolist(), s["sp_rr2"].tolist()):
        key = (ab & 0xff, ab >> 8)
        assert key not in flat and key[::-1] not in flat
        flat[key] = rr2
    seen = collections.Counter()
    for lane in range(s["lanes"]):
        for r in range(s["max_rounds"]):
            o = int(s["partner"][lane, r])
            if o < 0:
                continue
            assert lane < s["n_sph"] and r < s["rounds"]
            key = (lane, o) if (lane, o) in flat else (o, lane)
            assert key in flat, "slot (%d, %d) holds (%d, %d), which is no pair of the model" % (lane, r, lane, o)
            seen[key] += 1
            # bit for bit: the same double
            assert np.float64(s["rr2"][lane, r]).tobytes() == np.float64(flat[key]).tobytes(), (lane, r)
    assert set(seen) == set(flat) and all(n == 1 for n in seen.values())
    assert sum(seen.values()) == len(s["sp_ab"])


def test_primitive_masks_are_the_flat_list(sched):
    s = sched
    from_masks = sorted((p, sp) for sp in range(s["n_sph"]) for p in range(32) if (int(s["mask"][sp]) >> p) & 1)
    flat = sorted((int(ps) & 0xff, int(ps) >> 8) for ps in s["pp_ps"])
    assert from_masks == flat and len(set(flat)) == len(flat)
    assert all(p < s["n_prim"] for p, _ in from_masks)


def test_rounds_are_balanced_and_robotino_qualifies(sched):
    s = sched
    owned = (s["partner"] >= 0).sum(axis=1)
    assert s["ok"] == 1
    assert s["rounds"] == int(owned.max())
    assert s["rounds"] <= math.ceil(len(s["sp_ab"]) / s["n_sph"]) + 1
    # a sphere's pairs fill its rounds from 0 without gaps
    for lane in range(s["lanes"]):
        assert np.all(s["partner"][lane, :owned[lane]] >= 0) and np.all(s["partner"][lane, owned[lane]:] < 0)
    # the committed model: 50 spheres + 6 primitives, 499 pairs, and the optimum of ceil(499 / 50) rounds
    assert (s["n_sph"], s["n_prim"], len(s["sp_ab"]), len(s["pp_ps"])) == (50, 6, 499, 187)
    assert s["rounds"] == 10


def test_model_with_more_items_than_lanes_keeps_the_flat_lists():
    """Nine more spheres on one link: 59 spheres + 6 primitives > 64 lanes.  The model still builds, with the flat lists
    complete and the schedule empty; eight more (64 items) still qualify."""
    urdf, srdf = _description()
    for extra, ok in ((9, 0), (8, 1)):
        spec = json.load(open(L.SPHERES_JSON))
        spec["links"]["hand_cableCanal_link"] = spec["links"]["hand_cableCanal_link"] + [
            [0.01 * i, 0.0, 0.0, 0.03] for i in range(extra)]
        s = schedule(Robot.from_urdf(urdf, srdf, json.dumps(spec)))
        assert s["n_sph"] == 50 + extra and s["n_sph"] + s["n_prim"] == 56 + extra
        assert s["ok"] == ok
        assert len(s["sp_ab"]) > 499 and len(s["pp_ps"]) > 187
        if ok:
            assert s["rounds"] == int((s["partner"] >= 0).sum(axis=1).max()) <= s["max_rounds"]
            assert int((s["partner"] >= 0).sum()) == len(s["sp_ab"])
        else:
            assert s["rounds"] == 0 and np.all(s["partner"] < 0)
