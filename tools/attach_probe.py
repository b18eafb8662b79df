"""Cost of planning with a grasped object and of the self filter, on one GPU in one process.

Carve, on C2 (scenes.box_room, 129 k keys at 5 cm) and C5 (scenes.clutter_cloud, 1.35 M keys at 2 cm), every collision
link of the bare robot at the scene's start pose, pad 5 cm: smp_carve_keys (kernel_ms: HIP events around the FK
pre-launch and the carve kernel; total_ms: host clock, call entry to return, key upload and flag download included), and
the device scene build with the carve set against the plain one (smp_scene_build.kernel_ms / total_ms of both, and the
carve launches' share of the carved build, smp_carve_info.kernel_ms).  The variants alternate; one warm-up each, then
REPS calls; medians.

Planning, the C2 bench query (1e6 collision-checked samples, path_optimality_threshold = -inf) through
GpuPlanner.plan with the bare robot and with the tests' bar on hand_palm_link as 2 spheres (A2: 58 items, the self
rounds) and as 10 spheres (A10: 66 items -- the first measurement of the two-items-per-lane, flat-list regime of the
job tiles), same seeds, alternating: configurations per second and microseconds per iteration each, and the ratio to
the bare robot.  Prints one JSON line.

    python tools/attach_probe.py [--reps 10] > profiles/attach.json
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from squirrel_motion_planner_amd import _lib as L  # noqa: E402
from squirrel_motion_planner_amd import scenes  # noqa: E402
from squirrel_motion_planner_amd.planner import GpuPlanner, Robot  # noqa: E402

PAD = 0.05


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def bar(n):
    return ([(0.0, 0.0, 0.05 + 0.20 * (k + 0.5) / n) for k in range(n)],
            [math.sqrt((0.1 / n) ** 2 + 0.03 ** 2 + 0.03 ** 2)] * n)


def carve_case(name, sc, reps):
    gp = GpuPlanner(Robot())
    keys = np.ascontiguousarray(np.asarray(sc.keys).reshape(-1, 3), np.uint16)
    q = list(sc.start)
    mask = gp.carve_keys(keys, sc.res, q, PAD)                      # warm-up
    gp.set_scene_keys(keys, sc.res)                                  # warm-up, plain
    gp.set_carve(q, PAD)
    gp.set_scene_keys(keys, sc.res)                                  # warm-up, carved
    ck, ct, pk, pt, bk, bt, bc = [], [], [], [], [], [], []
    for _ in range(reps):
        m = gp.carve_keys(keys, sc.res, q, PAD)
        assert np.array_equal(m, mask)
        c = gp.last_carve()
        ck.append(c["kernel_ms"]); ct.append(c["total_ms"])
        gp.set_carve(None)
        b = gp.set_scene_keys(keys, sc.res)
        pk.append(b["kernel_ms"]); pt.append(b["total_ms"])
        n_plain = b["n_occupied"]
        gp.set_carve(q, PAD)
        b = gp.set_scene_keys(keys, sc.res)
        bk.append(b["kernel_ms"]); bt.append(b["total_ms"]); bc.append(gp.last_carve()["kernel_ms"])
        n_carved_build = b["n_occupied"]
    return {"scene": name, "keys": int(len(keys)), "resolution": sc.res, "pad": PAD, "links": "all",
            "n_carved": int(mask.sum()), "n_occupied_plain": int(n_plain), "n_occupied_carved": int(n_carved_build),
            "carve_keys": {"kernel_ms": stats(ck), "total_ms": stats(ct),
                           "keys_per_second_kernel": len(keys) / (np.median(ck) * 1e-3)},
            "build_plain": {"kernel_ms": stats(pk), "total_ms": stats(pt)},
            "build_carved": {"kernel_ms": stats(bk), "total_ms": stats(bt), "carve_kernel_ms": stats(bc)},
            "carve_share_of_carved_build_kernel": float(np.median(bc) / np.median(bk)),
            "ratio_carved_over_plain_kernel": float(np.median(bk) / np.median(pk)),
            "ratio_carved_over_plain_total": float(np.median(bt) / np.median(pt))}


def plan_cases(reps, samples):
    sc = scenes.box_room()
    robots = {"base": Robot(), "A2": Robot().attach("hand_palm_link", *bar(2)),
              "A10": Robot().attach("hand_palm_link", *bar(10))}
    gps = {}
    for k, r in robots.items():
        gps[k] = GpuPlanner(r, path_optimality_threshold=-np.inf)
        gps[k].set_scene_keys(sc.keys, sc.res)

    def run(k, seed):
        t0 = time.perf_counter()
        r = gps[k].plan(GpuPlanner.make_query(sc.start, sc.goal, sc.env_x, sc.env_y, samples=samples, seed=seed))
        dt = time.perf_counter() - t0
        assert r["status"] in (L.SMP_OK, L.SMP_ERR_NO_SOLUTION), r["status"]
        return r["configs_checked"] / dt, dt / max(r["iterations"], 1) * 1e6, r["iterations"], r["status"]

    for k in gps:
        run(k, 1)  # warm-up
    out = {k: {"configs_per_s": [], "us_per_iteration": [], "iterations": [], "status": []} for k in gps}
    for i in range(reps):
        for k in gps:
            c, u, it, st = run(k, 1 + 1000 * i)
            out[k]["configs_per_s"].append(c); out[k]["us_per_iteration"].append(u)
            out[k]["iterations"].append(int(it)); out[k]["status"].append(int(st))
    res = {}
    for k, v in out.items():
        info = robots[k].self_rounds_info()
        res[k] = {"items": info["n_sph"] + info["n_prim"], "self_rounds": bool(info["qualifies"]),
                  "sphere_pairs": info["n_spairs"], "configs_per_s": stats(v["configs_per_s"]),
                  "us_per_iteration": stats(v["us_per_iteration"]), "iterations": v["iterations"],
                  "status": v["status"]}
    for k in res:
        res[k]["configs_per_s_over_base"] = res[k]["configs_per_s"]["median"] / res["base"]["configs_per_s"]["median"]
        res[k]["us_per_iteration_over_base"] = (res[k]["us_per_iteration"]["median"] /
                                                res["base"]["us_per_iteration"]["median"])
    res["A10"]["note"] = "first measurement of the two-items-per-lane, flat-self-list regime (more than 64 items)"
    return {"scene": sc.name, "samples": samples, "seeds": [1 + 1000 * i for i in range(reps)], "robots": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--samples", type=float, default=1e6)
    a = ap.parse_args()
    res = {"reps": a.reps, "warmup": 1,
           "clocks": {"kernel_ms": "HIP events on the planner's stream (smp_carve_info / smp_scene_build)",
                      "total_ms": "host clock, call entry to return",
                      "planning": "time.perf_counter around GpuPlanner.plan"},
           "carve": [carve_case("C2", scenes.box_room(), a.reps), carve_case("C5", scenes.clutter_cloud(), a.reps)],
           "planning": plan_cases(a.reps, a.samples)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
