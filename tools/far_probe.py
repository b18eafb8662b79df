"""The far-goal stage on C2 (scenes.box_room): the base's free map, the route over it and the staged plan.

1. smp_base_free_map on the lattice over the scene's bounds at pitch = the map's resolution (5 cm) and 16 headings,
   alternating in one process with smp_check_configs on the same configurations formed on the host: each call's
   kernel_ms (HIP events around the kernel) and total_ms (host clock, call entry to return; for smp_check_configs it
   includes the upload of the configurations the free map never makes), and the two answers compared.
2. smp_base_route over that map from the scene's start to its goal: host time of the call.
3. smp_plan_far (the call's defaults: 10 cm, 8 headings, 2 m handover) against plain smp_plan on the C2 bench query
   (bench.py: 1e6 collision-checked samples, path_optimality_threshold = -inf), alternating: host time of the call,
   time to the first path (plain: time_first_solution_host; staged: the stages before the tail plus the tail's), rows,
   cost (the sum of dist over the rows) and each path's verdict by the dense check (smp_shortcut_path, window = 1).

One warm-up call each, then REPS calls; medians.  No thresholds: the ratios are the result.  Prints one JSON line.

    python tools/far_probe.py [--reps 10] [--samples 1000000] > profiles/far.json
"""
import argparse
import ctypes
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
from squirrel_motion_planner_amd.planner import GpuPlanner, Robot, Scene, base_lattice_fit  # noqa: E402

_pd = ctypes.POINTER(ctypes.c_double)


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def node_configs(lat):
    n = np.arange(lat.nx * lat.ny * lat.n_theta, dtype=np.int64)
    ix, iy, t = n % lat.nx, (n // lat.nx) % lat.ny, n // (lat.nx * lat.ny)
    q = np.empty((len(n), 8))
    q[:, 0] = lat.x0 + ix.astype(np.float64) * lat.pitch
    q[:, 1] = lat.y0 + iy.astype(np.float64) * lat.pitch
    q[:, 2] = lat.theta0 + t.astype(np.float64) * lat.dtheta
    q[:, 3:] = np.array(list(lat.arm))[None, :]
    return q


def free_map(gp, sc, reps, n_theta):
    lat = base_lattice_fit(sc.env_x, sc.env_y, sc.res, n_theta)
    q = node_configs(lat)
    t = {n: {"kernel_ms": [], "total_ms": []} for n in ("free_map", "check_configs")}
    free = own = None
    for rep in range(reps + 1):  # (rep 0 is the warm-up)
        free, info = gp.base_free_map(lat)
        t0 = time.perf_counter()
        own = gp.check_configs(q, False, True)
        total = (time.perf_counter() - t0) * 1e3
        if rep:
            t["free_map"]["kernel_ms"].append(info["kernel_ms"])
            t["free_map"]["total_ms"].append(info["total_ms"])
            t["check_configs"]["kernel_ms"].append(gp.last_kernel_ms()[0])
            t["check_configs"]["total_ms"].append(total)
    med = {n: {k: float(np.median(v)) for k, v in t[n].items()} for n in t}
    out = {"lattice": {"pitch": lat.pitch, "nx": lat.nx, "ny": lat.ny, "n_theta": lat.n_theta,
                       "nodes": int(free.size), "free": int(free.sum())},
           "same_answer": bool(np.array_equal(free.reshape(-1), own.astype(bool))),
           "free_map": {k: stats(v) for k, v in t["free_map"].items()},
           "check_configs": dict({k: stats(v) for k, v in t["check_configs"].items()},
                                 total_ms_is="host clock around the Python call: transpose, upload, kernel, download"),
           "ratio_check_configs_over_free_map": {k: med["check_configs"][k] / med["free_map"][k] for k in med["free_map"]}}
    return lat, out


def route(gp, lat, sc, reps):
    """smp_base_route itself over the words the free map left, from the scene's start to its goal."""
    bits = gp.base_map_bits
    a, b = (ctypes.c_double * 3)(*sc.start[:3]), (ctypes.c_double * 3)(*sc.goal[:3])
    ms, info, n_rows = [], L.RouteInfo(), 0
    for rep in range(reps + 1):
        rows, n_out, chain = _pd(), ctypes.c_int64(), ctypes.POINTER(ctypes.c_int32)()
        t0 = time.perf_counter()
        rc = L.lib().smp_base_route(ctypes.byref(lat), bits.ctypes.data_as(ctypes.c_void_p), a, b, 2, ctypes.byref(rows),
                                    ctypes.byref(n_out), ctypes.byref(chain), ctypes.byref(info))
        dt = (time.perf_counter() - t0) * 1e3
        L.lib().smp_buffer_free(rows)
        L.lib().smp_buffer_free(chain)
        L.check(rc, "smp_base_route")
        n_rows = n_out.value
        if rep:
            ms.append(dt)
    return {"host_ms": stats(ms), "n_chain": info.n_chain, "rows": n_rows, "n_settled": info.n_settled, "cost": info.cost,
            "from_node": list(info.from_node), "to_node": list(info.to_node)}


def path_cost(p):
    c = 0.0
    for i in range(len(p) - 1):
        s = 0.0
        for j in range(8):
            d = float(p[i + 1][j]) - float(p[i][j])
            s += d * d
        c += math.sqrt(s)
    return c


def verdict(gp, path):
    """The dense check of the path's adjacent edges: -1 if every edge is free, else the first blocked one."""
    if len(path) < 2:
        return None
    try:
        return gp.shortcut_path(path, window=1)[1]["first_blocked"]
    except L.SmpError as e:
        if e.status != L.SMP_ERR_NO_SOLUTION:
            raise
        return e.info["first_blocked"]


def plans(gp, sc, reps, samples, seed):
    res = {n: {"call_ms": [], "first_path_ms": []} for n in ("plan", "plan_far")}
    last = {}
    for rep in range(reps + 1):
        q = GpuPlanner.make_query(sc.start, sc.goal, sc.env_x, sc.env_y, samples=samples, seed=seed)
        t0 = time.perf_counter()
        p = gp.plan(q)
        tp = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        f = gp.plan_far(q)
        tf = (time.perf_counter() - t0) * 1e3
        last = {"plan": p, "plan_far": f}
        if rep:
            res["plan"]["call_ms"].append(tp)
            res["plan_far"]["call_ms"].append(tf)
            if p["time_first_solution_host"] >= 0:
                res["plan"]["first_path_ms"].append(p["time_first_solution_host"] * 1e3)
            if f["far"]["n_route_rows"] and f["time_first_solution_host"] >= 0:
                # (the tail's own call time is not reported: the stages before it are bounded by the call less the
                #  tail's planning loop)
                before = f["far"]["total_ms"] - f["time_total"] * 1e3
                res["plan_far"]["first_path_ms"].append(before + f["time_first_solution_host"] * 1e3)
    out = {}
    for n, r in last.items():
        path = r["path"]
        out[n] = {"status": r["status"], "rows": int(len(path)), "cost": path_cost(path) if len(path) else None,
                  "iterations": r["iterations"], "configs_checked": r["configs_checked"],
                  "dense_check_first_blocked": verdict(gp, path),
                  "call_ms": stats(res[n]["call_ms"]),
                  "first_path_ms": stats(res[n]["first_path_ms"]) if res[n]["first_path_ms"] else None}
    far = last["plan_far"]["far"]
    out["plan_far"]["far"] = {"stage": far["stage"], "n_route_rows": far["n_route_rows"],
                              "handover_node": list(far["handover_node"]), "map": far["map"],
                              "route": dict(far["route"], from_node=list(far["route"]["from_node"]),
                                            to_node=list(far["route"]["to_node"])),
                              "check": far["check"], "route_ms": far["route_ms"], "total_ms": far["total_ms"]}
    out["ratio_plan_far_over_plan"] = {k: out["plan_far"][k]["median"] / out["plan"][k]["median"]
                                       for k in ("call_ms", "first_path_ms") if out["plan"][k] and out["plan_far"][k]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--samples", type=float, default=1e6)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--headings", type=int, default=16)
    a = ap.parse_args()
    sc = scenes.box_room()
    gp = GpuPlanner(Robot(), path_optimality_threshold=-math.inf)
    gp.set_scene(Scene.from_keys(sc.keys, sc.res))
    lat, fm = free_map(gp, sc, a.reps, a.headings)
    res = {"scene": sc.name, "reps": a.reps, "warmup": 1,
           "clocks": {"kernel_ms": "HIP events around the kernel of the call", "total_ms": "host clock, call entry to return"},
           "free_map": fm, "route": route(gp, lat, sc, a.reps),
           "plans": dict(plans(gp, sc, a.reps, a.samples, a.seed), samples=a.samples, seed=a.seed,
                         far_opts="smp_far_opts_default")}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
