"""The margin checks restated (include/smp_gpu.h "Margin checks"), shared by test_margin_cpu.py, test_gpu_margin.py and
test_shim_margin.py.

A configuration is clear at the margins (mm, ms) iff it is valid by the CPU oracle, its map clearance by
clearance_restatement.py exceeds mm and its self clearance exceeds ms, each for a positive margin only: the conjunction
of code that exists without the margin kernels.  MarginOracle has the one method the restatements of the path passes
use of their oracle (check_configs), so shortcut_restatement.first_invalid / shortcut and
repair_restatement.sample_detours / repair restate the margin calls as they stand."""
import functools

import numpy as np

import clearance_restatement as C
import repair_restatement as P
import shortcut_restatement as R

SCENES = C.SCENES
POSE_MARGINS = ((0.1, 0.0), (0.05, 0.03), (0.0, 0.02))   # (map, self) of the check_clear cases
EDGE_MARGINS = ((0.02, 0.0), (0.1, 0.0), (0.0, 0.02))    # ... of the check_edges cases
PIPE_MARGIN = (0.02, 0.0)                                # the repair -> shortcut pipeline on the 12-waypoint C2 path
PIPE_SAMPLES = 64


class MarginOracle:
    """check_configs at the margins (mm, ms) in scene `name` (one of shortcut_restatement.scene, or a scene registered
    with clearance_restatement.register_scene whose oracle is passed as `orc`)."""

    def __init__(self, name, mm, ms, map_enabled=None, orc=None):
        self.name, self.mm, self.ms, self.map_enabled = name, float(mm), float(ms), map_enabled
        self.orc = orc if orc is not None else R.oracle_for(name, map_enabled)

    def check_configs(self, q, self_=True, map_=True):
        q = np.asarray(q, np.float64).reshape(-1, 8)
        ok = self.orc.check_configs(q, self_, map_).astype(bool)
        if map_ and self.mm > 0:
            # any admissible D above the margin gives the same comparison
            c = C.clearance(self.name, q, self.mm + 0.01, False, True, self.map_enabled)
            ok &= c["map"] > self.mm
        if self_ and self.ms > 0:
            c = C.clearance(self.name, q, 1.0, True, False)
            ok &= c["self"] > self.ms
        return ok.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def oracle(name, mm, ms, disabled=False):
    if name == "blocked":
        orc, keys, res = P.detour_scene("blocked")
        C.register_scene("blocked", keys, res)
        return MarginOracle(name, mm, ms, orc=orc)
    return MarginOracle(name, mm, ms, C.map_enabled_for(disabled))


@functools.lru_cache(maxsize=None)
def poses_expected(name, mm, ms, self_=True, map_=True, disabled=False):
    """clear per pose of clearance_restatement.poses(name)."""
    return oracle(name, mm, ms, disabled).check_configs(C.poses(name), self_, map_)


@functools.lru_cache(maxsize=None)
def edges_expected(name, mm, ms):
    """(first_invalid, M) of clearance_restatement.edges(name) at the margins."""
    a, b = C.edges(name)
    _, M = R.density(a, b, R.orobot().rev, R.N_SEG, R.STEP)
    return R.first_invalid(oracle(name, mm, ms), a, b, M), M


@functools.lru_cache(maxsize=None)
def edges_plain(name):
    a, b = C.edges(name)
    _, M = R.density(a, b, R.orobot().rev, R.N_SEG, R.STEP)
    return R.first_invalid(R.oracle_for(name), a, b, M)


def shortcut(w, mm, ms, window=0):
    return R.shortcut(oracle("c2", mm, ms), w, R.orobot().rev, R.N_SEG, R.STEP, window=window)


def repair(w, mm, ms, samples=PIPE_SAMPLES, rounds=4, seed=1):
    return P.repair(oracle("c2", mm, ms), w, samples=samples, rounds=rounds, seed=seed)


# The feature's sequence on the 12-waypoint C2 path at PIPE_MARGIN, each step computed once per process.
@functools.lru_cache(maxsize=None)
def pipeline_alone():
    """The margin shortcut of the path as it is (blocked)."""
    return shortcut(C.path12(), *PIPE_MARGIN)


@functools.lru_cache(maxsize=None)
def pipeline_repair():
    return repair(C.path12(), *PIPE_MARGIN)


@functools.lru_cache(maxsize=None)
def pipeline_shortcut(with_margin=True):
    """The all-pairs shortcut of the repaired rows, at the margin or plain."""
    mm, ms = PIPE_MARGIN if with_margin else (0.0, 0.0)
    return shortcut(pipeline_repair()["path"], mm, ms)


@functools.lru_cache(maxsize=None)
def detours_expected(case="a_blocked_gap", mm=0.02, ms=0.0):
    scn, a, b, samples, h, seed, rnd, n, self_, map_ = P.detour_cases()[case]
    return P.sample_detours(oracle(scn, mm, ms), a, b, samples, h, seed, rnd, self_, map_, n=n)
