"""Clearance of full planner paths: smp_clearance_edges on C2 (scenes.box_room).

The paths are those of tools/repair_probe.py: the planner's own output for a budget of 1e6 collision-checked
configurations (seed 1), not subsampled; that path repaired (smp_repair_path, default options); and the repaired path
shortened (smp_shortcut_path).  For each path and each max_dist (0.1 and 0.3) the adjacent edges go through
smp_clearance_edges and, alternating with it in the same process, through smp_check_edges -- the boolean check of the
same points, the only like-for-like figure there is.  kernel_ms is the library's HIP-event time around the kernel,
total_ms its host clock from call entry to return (for smp_check_edges: time.perf_counter around the call).  One warm-up
call each, then REPS calls; medians.  Recorded per path: the points, both calls' times, points per second, the ratio of
the two kernels, and the path's minimum map and self clearance with their witnesses.  Prints one JSON line.

    python tools/clearance_probe.py [--reps 10] [--samples 1000000] > profiles/clearance.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from squirrel_motion_planner_amd import _lib as L  # noqa: E402
from squirrel_motion_planner_amd import scenes  # noqa: E402
from squirrel_motion_planner_amd.planner import GpuPlanner, Robot, Scene  # noqa: E402


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def call(fn, *args, **kw):
    """(output or None, info)"""
    try:
        return fn(*args, **kw)
    except L.SmpError as e:
        if e.status != L.SMP_ERR_NO_SOLUTION:
            raise
        return None, e.info


def measure(gp, path, D, reps):
    a, b = path[:-1], path[1:]
    edges, summary = gp.path_clearance(path, D)  # warm-up
    first, npts = gp.check_edges(a, b)           # warm-up
    ck, ct, bk, bt = [], [], [], []
    for _ in range(reps):
        e = gp.edge_clearance(a, b, D)
        assert e.tobytes() == edges.tobytes()
        ck.append(gp.clearance_info["kernel_ms"])
        ct.append(gp.clearance_info["total_ms"])
        t0 = time.perf_counter()
        f, _ = gp.check_edges(a, b)
        bt.append((time.perf_counter() - t0) * 1e3)
        bk.append(gp.last_kernel_ms()[0])
        assert np.array_equal(f, first)
    pts = int(edges["n_points"].sum())
    assert np.array_equal(npts, edges["n_points"])
    # an edge is free exactly when both of its minima are positive
    assert np.array_equal(first < 0, (edges["map"] > 0) & (edges["self"] > 0))
    checked = int(np.where(first < 0, npts, first + 1).sum())
    return {"max_dist": D, "edges": int(len(a)), "points": pts,
            "clearance": {"kernel_ms": stats(ck), "total_ms": stats(ct),
                          "points_per_second_kernel": pts / (np.median(ck) * 1e-3)},
            "check_edges": {"kernel_ms": stats(bk), "total_ms": stats(bt), "blocked_edges": int((first >= 0).sum()),
                            "points_up_to_first_collision": checked,
                            "points_per_second_kernel": pts / (np.median(bk) * 1e-3)},
            "ratio_clearance_over_check_kernel": float(np.median(ck) / np.median(bk)),
            "ratio_clearance_over_check_total": float(np.median(ct) / np.median(bt)),
            "minimum": summary}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--samples", type=float, default=1e6)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    sc = scenes.box_room()
    gp = GpuPlanner(Robot())
    gp.set_scene(Scene.from_keys(sc.keys, sc.res))
    r = gp.plan(GpuPlanner.make_query(sc.start, sc.goal, sc.env_x, sc.env_y, samples=a.samples, seed=a.seed))
    if r["status"] != L.SMP_OK:
        raise SystemExit("no path within the budget (status %d)" % r["status"])
    paths = {"planned": r["path"]}
    repaired, _ = call(gp.repair_path, r["path"])
    if repaired is not None:
        paths["repaired"] = repaired
        short, _ = call(gp.shortcut_path, repaired)
        if short is not None:
            paths["shortcut"] = short
    res = {"scene": sc.name, "plan": {"samples": a.samples, "seed": a.seed, "iterations": r["iterations"],
                                      "cost": r["cost_best"][0]},
           "clocks": {"kernel_ms": "smp_clearance_info.kernel_ms / smp_last_kernel_ms (HIP events around the kernel)",
                      "total_ms": "smp_clearance_info.total_ms (host clock, call entry to return) / time.perf_counter "
                                  "around GpuPlanner.check_edges"},
           "reps": a.reps, "warmup": 1, "paths": {}}
    for name, path in paths.items():
        res["paths"][name] = {"waypoints": int(len(path)),
                              "runs": [measure(gp, path, D, a.reps) for D in (0.1, 0.3)]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
