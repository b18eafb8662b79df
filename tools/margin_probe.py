"""The margin passes on a full planner path: C2 (scenes.box_room), the planner's own output for a budget of 1e6
collision-checked configurations (seed 1), not subsampled -- the path of tools/repair_probe.py and clearance_probe.py.

1. The path's adjacent edges at the map margins 0.02 and 0.1 m: the margin check through smp_shortcut_path_margin with
   window = 1, alternating in one process with the boolean check of the same edges (smp_shortcut_path, window = 1) and
   with the clearance query at max_dist = the margin (smp_clearance_edges).  kernel_ms is the library's HIP-event time
   around the kernel, total_ms its host clock from call entry to return.  Recorded: the three calls' times and the
   ratios of the margin check to the other two.  The clearance query never stops early and the two checks stop an edge
   at its first failing tile, so the ratio to the clearance query is a figure for the call a user would otherwise make,
   not for equal work; points_up_to_first_failure says how much each check walked.
2. The pipeline: smp_repair_path_margin at a map margin of 0.02 m (default options), then the all-pairs
   smp_shortcut_path_margin of the result at the same margin, with the outputs of the README's repair and shortcut
   tables and the least map clearance of the result by smp_clearance_edges; the plain pipeline beside it.

One warm-up call each, then REPS calls; medians.  Prints one JSON line.

    python tools/margin_probe.py [--reps 10] [--samples 1000000] > profiles/margin.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from squirrel_motion_planner_amd import _lib as L  # noqa: E402
from squirrel_motion_planner_amd import scenes  # noqa: E402
from squirrel_motion_planner_amd.planner import GpuPlanner, Robot, Scene  # noqa: E402

TIMES = ("kernel_ms", "total_ms")


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def call(fn, *args, **kw):
    """(output or None, info): a blocked path is an answer here, not a failure."""
    try:
        return fn(*args, **kw)
    except L.SmpError as e:
        if e.status not in (L.SMP_ERR_NO_SOLUTION, L.SMP_ERR_START_INVALID, L.SMP_ERR_GOAL_INVALID):
            raise
        return None, dict(e.info, status=e.status)


def timed(fn, reps):
    """The call's info without its times, and the times of `reps` calls after one warm-up; the calls must agree."""
    out, info = fn()
    fixed = {k: v for k, v in info.items() if k not in TIMES}
    t = {k: [] for k in TIMES}
    for _ in range(reps):
        o, i = fn()
        assert {k: v for k, v in i.items() if k not in TIMES} == fixed
        assert (o is None) == (out is None) and (o is None or o.tobytes() == out.tobytes())
        for k in TIMES:
            t[k].append(i[k])
    return out, dict(fixed, **{k: stats(v) for k, v in t.items()})


def adjacent(gp, path, mm, reps):
    """Part 1 at one map margin: the three calls alternate, rep by rep."""
    a, b = path[:-1], path[1:]
    fns = {"margin": lambda: call(gp.shortcut_path, path, window=1, margin=(mm, 0.0))[1],
           "boolean": lambda: call(gp.shortcut_path, path, window=1)[1]}
    for f in fns.values():
        f()
    ref = gp.edge_clearance(a, b, mm)  # warm-up
    t = {n: {k: [] for k in TIMES} for n in ("margin", "boolean", "clearance")}
    info = {}
    for _ in range(reps):
        for n, f in fns.items():
            info[n] = f()
            for k in TIMES:
                t[n][k].append(info[n][k])
        e = gp.edge_clearance(a, b, mm)
        assert e.tobytes() == ref.tobytes()
        for k in TIMES:
            t["clearance"][k].append(gp.clearance_info[k])
    # the margin check and the clearance query agree edge by edge: no clear edge has a map term below the margin (the
    # query caps at max_dist = the margin, so it cannot tell "equal" from "above")
    first, npts = gp.check_edges(a, b, margin=(mm, 0.0))
    plain, _ = gp.check_edges(a, b)
    agree = bool(np.array_equal(first < 0, (plain < 0) & (ref["map"] >= mm)))
    med = {n: {k: float(np.median(t[n][k])) for k in TIMES} for n in t}
    walked = lambda f: int(np.where(f < 0, npts, f + 1).sum())
    return {"margin_map": mm, "edges": int(len(a)), "points": int(npts.sum()), "clear_iff_free_and_map_at_margin": agree,
            "margin": dict({k: stats(t["margin"][k]) for k in TIMES}, n_valid=info["margin"]["n_valid"],
                           points_up_to_first_failure=walked(first)),
            "boolean": dict({k: stats(t["boolean"][k]) for k in TIMES}, n_valid=info["boolean"]["n_valid"],
                            points_up_to_first_failure=walked(plain)),
            "clearance": dict({k: stats(t["clearance"][k]) for k in TIMES}, max_dist=mm,
                              least_map=float(ref["map"].min())),
            "ratio_margin_over_clearance": {k: med["margin"][k] / med["clearance"][k] for k in TIMES},
            "ratio_margin_over_boolean": {k: med["margin"][k] / med["boolean"][k] for k in TIMES}}


def pipeline(gp, path, margin, reps):
    """Part 2: repair, then the all-pairs shortcut of the result, both at `margin` (None: the plain calls)."""
    kw = {} if margin is None else {"margin": margin}
    repaired, rinfo = timed(lambda: call(gp.repair_path, path, **kw), reps)
    res = {"margin": margin, "repair": dict(rinfo, rows=None if repaired is None else int(len(repaired)))}
    if repaired is None:
        return res
    short, sinfo = timed(lambda: call(gp.shortcut_path, repaired, **kw), reps)
    res["shortcut"] = dict(sinfo, rows=None if short is None else int(len(short)))
    if short is not None:
        _, summary = gp.path_clearance(short, 0.3)
        res["result_clearance"] = summary
    return res


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
    path = r["path"]
    res = {"scene": sc.name, "plan": {"samples": a.samples, "seed": a.seed, "iterations": r["iterations"],
                                      "cost": r["cost_best"][0], "waypoints": int(len(path))},
           "clocks": {"kernel_ms": "the info records' kernel_ms (HIP events around the kernels of the call)",
                      "total_ms": "the info records' total_ms (host clock, call entry to return)"},
           "reps": a.reps, "warmup": 1,
           "adjacent_edges": [adjacent(gp, path, mm, a.reps) for mm in (0.02, 0.1)],
           "pipeline": [pipeline(gp, path, (0.02, 0.0), a.reps), pipeline(gp, path, None, a.reps)]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
