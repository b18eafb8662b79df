"""Clearance queries, the parts that need no GPU: the C ABI's symbols and records, the numpy restatement
(clearance_restatement.py) against facts it does not build on, and the non-vacuity of the GPU tests' inputs."""
import ctypes
import os
import re

import numpy as np
import pytest

import clearance_restatement as C
import shortcut_restatement as R
from conftest import ROOT
from squirrel_motion_planner_amd import _lib as L

NAMES = ["smp_clearance_configs", "smp_clearance_edges"]
D = 0.3


def header():
    return open(os.path.join(ROOT, "include", "smp_gpu.h")).read()


# ------------------------------------------------------------------------------------------ ABI
def test_lib_and_header_agree():
    bound = {n for n, _, _ in L.EXPORTS}
    for n in NAMES:
        assert n in bound and hasattr(L.lib(), n)
    text = header()
    assert re.search(r"typedef struct smp_clearance \{ double map, self; int32_t map_link, self_a, self_b, pad; \} "
                     r"smp_clearance;", text)
    assert re.search(r"typedef struct smp_edge_clearance \{ double map, self; int32_t map_point, self_point, map_link, "
                     r"self_a, self_b, n_points; \} smp_edge_clearance;", text)
    assert re.search(r"typedef struct smp_clearance_info \{ int64_t n_points; double kernel_ms, total_ms; \} "
                     r"smp_clearance_info;", text)
    assert re.search(r"\bint smp_clearance_configs\(smp_planner\* p, const double\* q_rows, int64_t n, double max_dist, "
                     r"int with_self, int with_map,\s+smp_clearance\* out, smp_clearance_info\* info\);", text)
    assert re.search(r"\bint smp_clearance_edges\(smp_planner\* p, const double\* from_rows, const double\* to_rows, "
                     r"int64_t n, double max_dist,\s+int with_self, int with_map, smp_edge_clearance\* out, "
                     r"smp_clearance_info\* info\);", text)
    for n in NAMES:  # the header's opening list names both, as additions of this library
        assert re.search(r"\*   %s\s[^*]*(\*[^*/][^*]*)*the reference has no counterpart" % n, text), n
    assert ctypes.sizeof(L.Clearance) == 32 and ctypes.sizeof(L.EdgeClearance) == 40
    assert [f for f, _ in L.Clearance._fields_] == ["map", "self", "map_link", "self_a", "self_b", "pad"]
    assert [f for f, _ in L.EdgeClearance._fields_] == ["map", "self", "map_point", "self_point", "map_link", "self_a",
                                                        "self_b", "n_points"]
    assert ctypes.sizeof(L.ClearanceInfo) == 24
    from squirrel_motion_planner_amd import planner
    assert planner.CLEARANCE_DTYPE.itemsize == 32 and planner.EDGE_CLEARANCE_DTYPE.itemsize == 40


def test_null_planner_is_an_argument_error():
    q = np.zeros(8)
    pd = ctypes.POINTER(ctypes.c_double)
    c, e = L.Clearance(), L.EdgeClearance()
    assert L.lib().smp_clearance_configs(None, q.ctypes.data_as(pd), 1, D, 1, 1, ctypes.byref(c), None) == L.SMP_ERR_ARG
    assert L.lib().smp_clearance_edges(None, q.ctypes.data_as(pd), q.ctypes.data_as(pd), 1, D, 1, 1, ctypes.byref(e),
                                       None) == L.SMP_ERR_ARG


# ------------------------------------------------------------------------------------------ restatement against facts
@pytest.fixture(scope="module", params=C.SCENES)
def facts(request):
    """300 random configurations of a scene, their restated clearance and the oracle's flags."""
    name = request.param
    q = R.random_configs(R.scene(name)[0], 300, 11)
    orc = R.oracle_for(name)
    return name, q, C.clearance(name, q, D), orc


def test_model_lists_are_the_checkers():
    m = C.model()
    assert len(m.sp) == 499 and len(m.pp) == 187
    assert (m.sp[:, 2] < m.sp[:, 3]).all() and (m.pp[:, 2] < m.pp[:, 3]).all()


def test_sign_agrees_with_the_oracle(facts):
    name, q, c, orc = facts
    vm = orc.check_configs(q, False, True).astype(bool)
    vs = orc.check_configs(q, True, False).astype(bool)
    print(name, "map capped / in range / zero / negative:", int((c["map"] == D).sum()),
          int(((c["map"] > 0) & (c["map"] < D)).sum()), int((c["map"] == 0).sum()), int((c["map"] < 0).sum()))
    assert vm[c["map"] > 0].all() and not vm[c["map"] < 0].any() and not vm[c["map"] == 0].any()
    assert vs[c["self"] > 0].all() and not vs[c["self"] < 0].any() and not vs[c["self"] == 0].any()
    both = orc.check_configs(q).astype(bool)
    assert np.array_equal(both, (c["map"] > 0) & (c["self"] > 0))


def test_centres_agree_with_the_link_frames(facts):
    """Sphere centres from Oracle.fk's link frames and sph_c, against the body-frame centres: rounding of about 100
    fp64 operations on coordinates below 100 m."""
    name, q, c, orc = facts
    rb = R.orobot()
    wc, _ = C.world(orc, q)
    fr, _ = orc.fk(q)
    F = fr[:, rb.sph_link, :]
    sc = rb.sph_c.reshape(-1, 3)[None, :, :]
    ref = np.stack([F[:, :, 3 * r] * sc[:, :, 0] + F[:, :, 3 * r + 1] * sc[:, :, 1] + F[:, :, 3 * r + 2] * sc[:, :, 2]
                    + F[:, :, 9 + r] for r in range(3)], axis=2)
    err = np.abs(ref - wc).max()
    print(name, "largest centre difference", err)
    assert err <= 1e-12


def test_map_is_one_lipschitz_in_the_base(facts):
    name, q, c, orc = facts
    delta = 0.013
    q2 = q.copy()
    q2[:, 0] += delta
    c2 = C.clearance(name, q2, D, with_self=False)
    step = np.abs(c2["map"] - c["map"]).max()
    print(name, "largest change of map", step)
    assert step <= delta + 1e-12


def test_prefilter_changes_nothing(facts):
    name, q, c, orc = facts
    full = C.clearance(name, q[:24], D, prefilter=False)
    for f in ("map", "self", "map_link", "self_a", "self_b"):
        assert np.array_equal(full[f], c[:24][f]), f


def test_one_voxel_scene():
    """One occupied voxel [0.5, 0.55] x [0, 0.05] x [0.88, 0.93] and the robot at the origin (inside the grid, which is
    padded by 0.55 m around the voxel): the head (an upright cylinder of radius 0.23 around the base's axis, 0.25 m tall
    around z = 0.84 above the base frame) is level with the voxel and 0.5 - 0.23 away from its nearest face; the folded
    arm stays below it."""
    from squirrel_motion_planner_amd import scenes
    keys = np.array([[32768 + 10, 32768, 32768 + 18]])
    C.register_scene("one_voxel", keys, 0.05)
    q = np.array([[0.0, 0.0, 0.0] + scenes.ARM_FOLDED])
    rb = R.orobot()
    c = C.clearance("one_voxel", q, 0.5)
    print("map", c["map"][0], rb.link_names[c["map_link"][0]])
    assert abs(c["map"][0] - 0.27) <= 1e-12
    assert rb.link_names[c["map_link"][0]] == "head_link"
    # a query distance below it: capped, no witness
    c = C.clearance("one_voxel", q, 0.25)
    assert c["map"][0] == 0.25 and c["map_link"][0] == -1
    # turned by 90 degrees about the axis the head is centred on: the same distance
    q[0, 2] = np.pi / 2
    c = C.clearance("one_voxel", q, 0.5)
    assert abs(c["map"][0] - 0.27) <= 1e-12


# ------------------------------------------------------------------------------------------ the GPU tests' inputs
def test_gpu_poses_hold_every_kind():
    """From the restatement and the oracle alone: at least 8 poses of each kind among the GPU tests' configurations."""
    for name in C.SCENES:
        c = C.expected(name, C.N_POSES, D)
        inr = (c["map"] > 0) & (c["map"] < D)
        kinds = {"map == D": c["map"] == D, "in range, sphere link": inr & (c["kind"] == C.SPHERE),
                 "in range, primitive link": inr & (c["kind"] == C.PRIM), "map < 0": c["map"] < 0,
                 "map == 0": c["map"] == 0, "self by a sphere pair": c["self_kind"] == C.SPHERE,
                 "self by a primitive-sphere pair": c["self_kind"] == C.PRIM, "self < 0": c["self"] < 0}
        print(name, {k: int(v.sum()) for k, v in kinds.items()})
        for k, v in kinds.items():
            assert v.sum() >= 8, (name, k)
        assert ((c["map_link"] >= 0) == (c["map"] < D)).all()
        # the booleans of the same poses, by the oracle
        valid = R.oracle_for(name).check_configs(C.poses(name)).astype(bool)
        assert np.array_equal(valid, (c["map"] > 0) & (c["self"] > 0))
        # the narrow and the wide query distance see other things
        assert (C.expected(name, C.N_POSES, 0.05)["map"] == 0.05).sum() > (c["map"] == D).sum()
        wide = C.clearance(name, C.poses(name)[:8], 1.0)
        assert (wide["map"] > D).any()


def test_disabled_link_changes_an_answer():
    rb = R.orobot()
    assert C.DISABLED_LINK.startswith("arm_link") and C.DISABLED_LINK in rb.link_names
    c, d = C.expected("c2", C.N_POSES, D), C.expected("c2", C.N_POSES, D, disabled=True)
    changed = np.flatnonzero((c["map"] != d["map"]) | (c["map_link"] != d["map_link"]))
    print("poses changed by disabling", C.DISABLED_LINK, changed)
    assert len(changed) >= 1
    assert (c["map_link"][changed] == rb.link_names.index(C.DISABLED_LINK)).all()
    assert (d["map"] >= c["map"]).all() and np.array_equal(c["self"], d["self"])


def test_edges_span_tiles():
    for name in C.SCENES:
        e = C.edges_expected(name)
        assert len(e["M"]) == 16 and 2000 <= e["points"] <= C.EDGE_MAX_POINTS_TOTAL
        assert (e["M"] + 1 > R.CT).all() and ((e["M"] + 1) % R.CT != 0).any()
        # a minimum in a later tile than the edge's first, of each kind; a capped edge; an end point as the witness
        assert (e["map_point"] >= R.CT).any() and (e["self_point"] >= R.CT).any()
        assert (e["map_point"] == -1).any() and ((e["map_point"] == -1) == (e["map"] == D)).all()
        assert (e["self_point"] == e["M"]).any() or (e["map_point"] == e["M"]).any()
        assert (e["map"] < 0).any() and (e["map"] > 0).any()


def test_path_of_the_shortcut_tests():
    w = C.path12()
    assert len(w) == 12
    e = C.edge_clearance("c2", w[:-1], w[1:], D)
    assert (e["map"] > 0).all() and (e["self"] > 0).all()  # the path is free at the dense check
    assert len(set(e["map_link"])) > 1 or (e["map"] < D).any()
