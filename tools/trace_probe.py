"""Device timeline of the planner (SMP_TRACE build): thread 0 of the leader and of the scouts log (source site,
device clock) records for a window of iterations of the C2 query; this prints, per role, the mean time between
consecutive trace points (keyed by the two sites, file:line of smp_kernels.hip and the smp_plan_*.h headers it includes) and the raw
timeline of two iterations.

  make -C squirrel_motion_planner_amd EXTRA=-DSMP_TRACE BUILD=build_trace OUT=lib/libsmp_gpu_trace.so
  SMP_LIB=squirrel_motion_planner_amd/lib/libsmp_gpu_trace.so python tools/trace_probe.py [iterations]
"""
import collections
import ctypes
import math
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from squirrel_motion_planner_amd import _lib as L, scenes  # noqa: E402
from squirrel_motion_planner_amd.planner import GpuPlanner, Scene  # noqa: E402

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 3100
lib = L.lib()
lib.smp_debug_tlog.restype = ctypes.c_int
lib.smp_debug_tlog.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.c_int, ctypes.c_int]
sc = scenes.box_room()
gp = GpuPlanner(path_optimality_threshold=-math.inf, scout=int(os.environ.get("SMP_SCOUTS", "1")))
gp.set_scene(Scene.from_keys(sc.keys, sc.res))
buf = (ctypes.c_uint64 * (1 << 18))()
lib.smp_debug_tlog(buf, 1 << 18, 1)  # reset
start, goal = sc.start, sc.goal
if os.environ.get("SMP_TRACE_C3Q"):  # one of C3's random queries (bench.py --workload c3) instead of C2's pair
    pairs = scenes.random_queries(sc, 8, seed=7, check=lambda q: bool(gp.check_configs([q])[0]))
    start, goal = pairs[int(os.environ["SMP_TRACE_C3Q"])]
r = gp.plan(GpuPlanner.make_query(start, goal, sc.env_x, sc.env_y, iterations=iters, seed=1,
                                  query_id=int(os.environ.get("SMP_TRACE_C3Q", "0"))))
n = lib.smp_debug_tlog(buf, 1 << 18, 1)
print("iterations %d, checked %d, first solution iter %d, %d trace records" % (
    r["iterations"], r["configs_checked"], r["first_solution_iter"], n))
a = np.ctypeslib.as_array(buf).astype(np.uint64)
a = a[a != 0]
role = (a >> np.uint64(62)).astype(int)
it = ((a >> np.uint64(54)) & np.uint64(0xff)).astype(int)
# a record (csrc/smp_plan_prof.h TR_RECORD): role << 62 | iteration << 54 | site << 36 | clock; a site (csrc/smp_kernels.h):
# file << SITE_LINE_BITS | line, the file's number being its place in SITE_FILES there
CLOCK_BITS, LINE_BITS, FILE_BITS = 36, 13, 5
line = ((a >> np.uint64(CLOCK_BITS)) & np.uint64((1 << (LINE_BITS + FILE_BITS)) - 1)).astype(int)  # the site word
clk = (a & np.uint64((1 << CLOCK_BITS) - 1)).astype(np.int64)
if len(clk):  # the clock field wraps every 2^36 ticks (11 minutes): times relative to the first record
    clk = ((clk - clk[0] + (1 << (CLOCK_BITS - 1))) % (1 << CLOCK_BITS)) - (1 << (CLOCK_BITS - 1))
TICK_US = 0.01  # wall clock 100 MHz
TR_BAR0 = ((1 << FILE_BITS) - 1) << LINE_BITS  # TR_BARRIERS: file SITE_FILE_BARRIERS, line field = barriers of the iteration
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "squirrel_motion_planner_amd", "csrc")
table = re.search(r"SITE_FILES\[\] = \{(.*?)\};", open(os.path.join(CSRC, "smp_kernels.h")).read(), re.S).group(1)
files = {k: (name, open(os.path.join(CSRC, name)).read().split("\n"))  # file number -> (file name, its lines)
         for k, name in enumerate(re.findall(r'"([^"]+)"', table))}


def site_of(w):
    """file:line of a site word."""
    f, ln = w >> LINE_BITS, w & ((1 << LINE_BITS) - 1)
    return "%s:%d" % (files[f][0].replace("smp_plan_", "").replace("smp_", ""), ln) if f in files else "?%d:%d" % (f, ln)


def func_of(w):
    f, ln = w >> LINE_BITS, w & ((1 << LINE_BITS) - 1)
    src = files[f][1] if f in files else []
    for k in range(min(ln, len(src)) - 1, -1, -1):
        t = src[k]
        if t.startswith("__device__") or t.startswith("__global__"):
            name = t.split("(")[0].split()[-1]
            return name
    return "?"


for rl in sorted(set(role.tolist())):
    m = role == rl
    order = np.argsort(clk[m], kind="stable")
    R_it, R_ln, R_ck = it[m][order], line[m][order], clk[m][order]
    bar = R_ln >= TR_BAR0  # the leader's barrier counts (one record at each iteration's end), not trace points
    if bar.any():
        cnt = collections.Counter((R_ln[bar] - TR_BAR0).tolist())
        print("\n=== role %d: __syncthreads() per iteration: median %d, min %d, max %d; count x iterations: %s" % (
            rl, int(np.median(R_ln[bar] - TR_BAR0)), int(R_ln[bar].min() - TR_BAR0), int(R_ln[bar].max() - TR_BAR0),
            " ".join("%dx%d" % kv for kv in sorted(cnt.items()))))
        R_it, R_ln, R_ck = R_it[~bar], R_ln[~bar], R_ck[~bar]
    trans = collections.OrderedDict()
    its = sorted(set(R_it.tolist()))
    for k in range(len(R_ck) - 1):
        key = (R_ln[k], R_ln[k + 1])
        d = (R_ck[k + 1] - R_ck[k]) * TICK_US
        s = trans.setdefault(key, [0.0, 0])
        s[0] += d
        s[1] += 1
    tot = (R_ck[-1] - R_ck[0]) * TICK_US
    print("\n=== role %d (%s): %d iterations in window, %.1f us per iteration" % (
        rl, "leader" if rl == 0 else "scout %d" % rl, len(its), tot / max(len(its) - 1, 1)))
    rows = sorted(trans.items(), key=lambda kv: -kv[1][0])
    for (l0, l1), (s, c) in rows[:int(os.environ.get("SMP_TRACE_ROWS", "40"))]:
        print("  %5.2f us/iter  %6.2f us x %4d   %18s %-22s -> %18s %-22s" % (
            s / max(len(its), 1), s / c, c, site_of(l0), func_of(l0)[:22], site_of(l1), func_of(l1)[:22]))

# raw timeline of two leader iterations with the scouts' records interleaved
w0 = int(os.environ.get("SMP_TRACE_W0", "20"))
nw = int(os.environ.get("SMP_TRACE_NW", "2"))
sel = (it >= w0) & (it < w0 + nw)
order = np.argsort(clk[sel], kind="stable")
t0 = clk[sel][order][0] if sel.any() else 0
print("\n=== timeline (iterations %d-%d of the window), us from the first record" % (w0, w0 + 1))
for rl_, it_, ln_, ck_ in zip(role[sel][order], it[sel][order], line[sel][order], clk[sel][order]):
    if ln_ >= TR_BAR0:
        print("  %8.2f  L  it+%d  %d barriers in the iteration" % ((ck_ - t0) * TICK_US, it_ - w0, ln_ - TR_BAR0))
        continue
    print("  %8.2f  %s it+%d  %18s %s" % ((ck_ - t0) * TICK_US, "L " if rl_ == 0 else "S%d" % rl_, it_ - w0, site_of(ln_),
                                          func_of(ln_)))
