"""The base route on the device against the host route, on C2 (scenes.box_room).

1. For the lattices (5 cm, 16 headings) and (10 cm, 8 headings) over the scene's bounds: smp_base_free_map once, then
   smp_base_route and smp_base_route_gpu on the same words from the scene's start to its goal, alternating in one process:
   host time of each call, the device call's rounds, launches, tile_runs, kernel_ms and total_ms, and whether the two
   answers are equal.  The rounds enqueued between two reads of the changed counters are a build constant: for a sweep,
   run --routes-only on variant builds (make EXTRA=-DSMP_FIELD_BATCH=8 BUILD=build_b8 OUT=lib/libsmp_gpu_b8.so, then
   SMP_LIB=.../libsmp_gpu_b8.so), one JSON line each; `launches` tells them apart.
2. smp_plan_far (the call's defaults: 10 cm, 8 headings, 2 m handover) on the C2 bench query with route_device 0 and 1,
   alternating: host time of the call, time to the first path, route_ms.

One warm-up call each, then REPS calls; medians.  No thresholds: the ratios are the result.  Prints one JSON line.

    python tools/field_probe.py [--reps 10] [--samples 1000000] [--routes-only] > profiles/field.json
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

FIELD_KEYS = ("rounds", "launches", "tile_runs", "fell_back", "n_reached")


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def raw_route(gp, lat, bits, a, b, device):
    """One smp_base_route / smp_base_route_gpu call on packed words: (host ms of the C call, rows, chain, info, field)."""
    fa, fb = (ctypes.c_double * 3)(*a), (ctypes.c_double * 3)(*b)
    rows, n_out, chain = ctypes.POINTER(ctypes.c_double)(), ctypes.c_int64(), ctypes.POINTER(ctypes.c_int32)()
    info, finfo = L.RouteInfo(), L.FieldInfo()
    head = (ctypes.byref(lat), bits.ctypes.data_as(ctypes.c_void_p), fa, fb, 2, ctypes.byref(rows), ctypes.byref(n_out),
            ctypes.byref(chain), ctypes.byref(info))
    t0 = time.perf_counter()
    rc = L.lib().smp_base_route_gpu(gp.h, *head, ctypes.byref(finfo)) if device else L.lib().smp_base_route(*head)
    ms = (time.perf_counter() - t0) * 1e3
    L.check(rc, "route")
    r = np.ctypeslib.as_array(rows, shape=(n_out.value, 8)).copy()
    c = np.ctypeslib.as_array(chain, shape=(info.n_chain, 3)).copy()
    L.lib().smp_buffer_free(rows)
    L.lib().smp_buffer_free(chain)
    d = dict(from_node=list(info.from_node), to_node=list(info.to_node), n_chain=info.n_chain, n_settled=info.n_settled,
             cost=info.cost)
    return ms, r, c, d, {f: getattr(finfo, f) for f, _ in L.FieldInfo._fields_}


def routes(gp, sc, pitch, n_theta, reps):
    lat = base_lattice_fit(sc.env_x, sc.env_y, pitch, n_theta)
    free, minfo = gp.base_free_map(lat)
    bits = gp.base_map_bits.copy()
    a, b = sc.start[:3], sc.goal[:3]
    host, dev, kern, total = [], [], [], []
    h = d = None
    for rep in range(reps + 1):  # (rep 0 is the warm-up)
        h = raw_route(gp, lat, bits, a, b, False)
        d = raw_route(gp, lat, bits, a, b, True)
        if rep:
            host.append(h[0])
            dev.append(d[0])
            kern.append(d[4]["kernel_ms"])
            total.append(d[4]["total_ms"])
    h, d = h[1:], d[1:]
    same = bool(np.array_equal(h[0].view(np.uint64), d[0].view(np.uint64)) and np.array_equal(h[1], d[1]) and h[2] == d[2])
    out = {"lattice": {"pitch": pitch, "nx": lat.nx, "ny": lat.ny, "n_theta": n_theta, "nodes": int(free.size),
                       "free": int(free.sum())},
           "free_map_total_ms": minfo["total_ms"], "same_answer": same,
           "route": {"n_chain": h[2]["n_chain"], "n_settled": h[2]["n_settled"], "cost": h[2]["cost"], "rows": int(len(h[0]))},
           "host_call_ms": stats(host), "device_call_ms": stats(dev),
           "call_ms_is": "host clock around the C call, on the words smp_base_free_map left",
           "device": dict({k: d[3][k] for k in FIELD_KEYS}, kernel_ms=stats(kern), total_ms=stats(total)),
           "ratio_host_over_device_call": float(np.median(host) / np.median(dev))}
    return out


def plans(gp, sc, reps, samples, seed):
    res = {n: {"call_ms": [], "first_path_ms": [], "route_ms": []} for n in ("host_route", "device_route")}
    last = {}
    for rep in range(reps + 1):
        for n, rd in (("host_route", 0), ("device_route", 1)):
            q = GpuPlanner.make_query(sc.start, sc.goal, sc.env_x, sc.env_y, samples=samples, seed=seed)
            f, tf = timed(lambda: gp.plan_far(q, route_device=rd))
            last[n] = f
            if rep:
                res[n]["call_ms"].append(tf)
                res[n]["route_ms"].append(f["far"]["route_ms"])
                if f["far"]["n_route_rows"] and f["time_first_solution_host"] >= 0:
                    before = f["far"]["total_ms"] - f["time_total"] * 1e3
                    res[n]["first_path_ms"].append(before + f["time_first_solution_host"] * 1e3)
    out = {n: {k: stats(v) if v else None for k, v in r.items()} for n, r in res.items()}
    a, b = last["host_route"], last["device_route"]
    out["same_answer"] = bool(a["status"] == b["status"] and np.array_equal(a["path"].view(np.uint64), b["path"].view(np.uint64))
                              and a["far"]["route"] == b["far"]["route"])
    out["status"], out["rows"], out["n_route_rows"] = a["status"], int(len(a["path"])), a["far"]["n_route_rows"]
    out["ratio_host_over_device"] = {k: out["host_route"][k]["median"] / out["device_route"][k]["median"]
                                     for k in ("call_ms", "first_path_ms", "route_ms")
                                     if out["host_route"][k] and out["device_route"][k]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--samples", type=float, default=1e6)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--routes-only", action="store_true")
    a = ap.parse_args()
    sc = scenes.box_room()
    gp = GpuPlanner(Robot(), path_optimality_threshold=-math.inf)
    gp.set_scene(Scene.from_keys(sc.keys, sc.res))
    res = {"scene": sc.name, "reps": a.reps, "warmup": 1, "lib": os.path.basename(L.LIB_PATH),
           "routes": {"5cm_16": routes(gp, sc, sc.res, 16, a.reps), "10cm_8": routes(gp, sc, 0.1, 8, a.reps)}}
    if not a.routes_only:
        res["plan_far"] = dict(plans(gp, sc, a.reps, a.samples, a.seed), samples=a.samples, seed=a.seed,
                               far_opts="smp_far_opts_default")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
