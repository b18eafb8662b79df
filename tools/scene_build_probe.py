"""Scene hand-off latency, host build against device build, on C2 (scenes.box_room) and C5 (scenes.clutter_cloud).

Host path: smp_scene_from_keys + smp_planner_set_scene (every derived array on one host thread, then uploaded), timed
by the host clock from keys in hand to return.  Device path: smp_planner_set_scene_keys; total_ms is the library's
host clock from call entry to return (key upload and the final synchronisation included), kernel_ms the HIP events
around the build kernels on the planner's stream.  One process, one warm-up of each path, then REPS repetitions with
the two paths alternated; the keys are a contiguous uint16 array before any clock starts.  Prints one JSON line.

    python tools/scene_build_probe.py [--reps 10] [--scenes c2,c5] > profiles/scene_build.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from squirrel_motion_planner_amd import scenes  # noqa: E402
from squirrel_motion_planner_amd.planner import GpuPlanner, Robot, Scene  # noqa: E402


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def host_ms(gp, keys, res):
    t = time.perf_counter()
    gp.set_scene(Scene.from_keys(keys, res))
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scenes", default="c2,c5")
    a = ap.parse_args()
    robot = Robot()
    A, B = GpuPlanner(robot), GpuPlanner(robot)
    out = {"clocks": {"host_ms": "time.perf_counter around smp_scene_from_keys + smp_planner_set_scene",
                      "gpu_total_ms": "smp_scene_build.total_ms (host clock, call entry to return)",
                      "gpu_kernel_ms": "smp_scene_build.kernel_ms (HIP events on the planner's stream)"},
           "reps": a.reps, "warmup": 1, "order": "host, gpu alternated per repetition", "scenes": {}}
    for name in a.scenes.split(","):
        sc = {"c2": scenes.box_room, "c5": scenes.clutter_cloud}[name]()
        keys = np.ascontiguousarray(sc.keys, np.uint16)
        host_ms(A, keys, sc.res)
        info = B.set_scene_keys(keys, sc.res)
        equal = all(np.array_equal(x, y) for x, y in zip(A.scene_arrays()[1:], B.scene_arrays()[1:]) if x is not None)
        h, g, k = [], [], []
        for _ in range(a.reps):
            h.append(host_ms(A, keys, sc.res))
            i = B.set_scene_keys(keys, sc.res)
            g.append(i["total_ms"])
            k.append(i["kernel_ms"])
        out["scenes"][name] = {"scene": sc.name, "keys": int(len(keys)), "dims": list(info["dims"]),
                               "cells": int(np.prod(info["dims"])), "n_occupied": info["n_occupied"],
                               "arrays_equal": bool(equal), "host_ms": stats(h), "gpu_total_ms": stats(g),
                               "gpu_kernel_ms": stats(k),
                               "ratio_host_over_gpu_total": float(np.median(h) / np.median(g))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
