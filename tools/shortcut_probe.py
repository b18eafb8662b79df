"""Path shortcutting on a full planner path: smp_shortcut_path on C2 (scenes.box_room), all waypoint pairs.

The path is the planner's own output for a budget of 1e6 collision-checked configurations (seed 1), not subsampled:
every waypoint pair is one candidate edge, checked at the planner's collision density in one edges_kernel launch.
kernel_ms is the library's HIP-event time around that launch, total_ms its host clock from call entry to return (table
build, uploads, the launch, the dynamic program and the output included).  One process, one warm-up call, then REPS
calls; medians.  For comparison the same point set -- every candidate edge's points up to and including its first
colliding one, built with numpy by the density rule of include/smp_gpu.h -- is checked by the CPU oracle's
check_configs on one host core, in chunks, timing only those calls.  Prints one JSON line.

    python tools/shortcut_probe.py [--reps 10] [--window 0] [--samples 1000000] > profiles/shortcut.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import oracle as O  # noqa: E402
from squirrel_motion_planner_amd import _lib as L  # noqa: E402
from squirrel_motion_planner_amd import scenes  # noqa: E402
from squirrel_motion_planner_amd.planner import GpuPlanner, Robot, Scene  # noqa: E402


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def shortcut(gp, path, window):
    """(status, rows of the output, info)"""
    try:
        out, info = gp.shortcut_path(path, window=window)
        return L.SMP_OK, len(out), info
    except L.SmpError as e:
        if e.status != L.SMP_ERR_NO_SOLUTION:
            raise
        return e.status, 0, e.info


def oracle_seconds(gp, orc, path, window, chunk=2048):
    """Seconds of Oracle.check_configs over the point set of the call, and the number of points."""
    k = len(path)
    w = k - 1 if window <= 0 or window > k - 1 else window
    pairs = np.array([(i, j) for j in range(1, k) for i in range(max(0, j - w), j)])
    secs, points = 0.0, 0
    for c0 in range(0, len(pairs), chunk):
        pc = pairs[c0:c0 + chunk]
        a, b = path[pc[:, 0]], path[pc[:, 1]]
        first, npts = gp.check_edges(a, b)
        upto = np.where(first < 0, npts, first + 1)
        pts = []
        for e in range(len(pc)):
            step = (b[e] - a[e]) / float(npts[e] - 1)
            pts.append(a[e][None, :] + np.arange(upto[e], dtype=np.float64)[:, None] * step[None, :])
        pts = np.ascontiguousarray(np.concatenate(pts))
        t = time.perf_counter()
        v = orc.check_configs(pts)
        secs += time.perf_counter() - t
        points += len(pts)
        # the oracle agrees with the kernel on where every edge ends
        off = np.concatenate([[0], np.cumsum(upto)])
        last = v[off[1:] - 1]
        assert np.array_equal(last == 0, first >= 0) and v.sum() == len(v) - int((first >= 0).sum())
    return secs, points


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--window", type=int, default=0)
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
    status, rows, info = shortcut(gp, path, a.window)  # warm-up
    kern, total = [], []
    for _ in range(a.reps):
        s, n, i = shortcut(gp, path, a.window)
        assert (s, n, i["configs_checked"]) == (status, rows, info["configs_checked"])
        kern.append(i["kernel_ms"])
        total.append(i["total_ms"])
    orc = O.Oracle(O.OracleRobot(L.MODEL_JSON), O.OracleScene(sc.keys, sc.res))
    cpu_s, points = oracle_seconds(gp, orc, path, a.window)
    assert points == info["configs_checked"]
    out = {"scene": sc.name, "plan": {"samples": a.samples, "seed": a.seed, "iterations": r["iterations"],
                                      "cost": r["cost_best"][0]},
           "clocks": {"kernel_ms": "smp_shortcut_info.kernel_ms (HIP events around edges_kernel)",
                      "total_ms": "smp_shortcut_info.total_ms (host clock, call entry to return)",
                      "oracle_s": "time.perf_counter around Oracle.check_configs, one host core, the same points"},
           "schedule": "atomic work counter, edges longest first", "reps": a.reps, "warmup": 1, "window": a.window,
           "status": status, "k": int(len(path)), "rows_out": rows, "n_edges": info["n_edges"],
           "n_valid": info["n_valid"], "configs_checked": info["configs_checked"],
           "first_blocked": info["first_blocked"], "cost_in": info["cost_in"], "cost_out": info["cost_out"],
           "kernel_ms": stats(kern), "total_ms": stats(total),
           "configs_per_second_kernel": info["configs_checked"] / (np.median(kern) * 1e-3),
           "configs_per_second_total": info["configs_checked"] / (np.median(total) * 1e-3),
           "oracle_s": cpu_s, "oracle_configs_per_second": points / cpu_s,
           "ratio_oracle_over_total": cpu_s / (np.median(total) * 1e-3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
