"""The device scene build's entry points (smp_planner_set_scene_keys / _bt / _ot / _octomap_msg) as far as a machine
without a GPU can see them: bound in _lib, declared in the header, and a NULL planner is an argument error before
any HIP call."""
import ctypes
import os
import re

from conftest import ROOT
from squirrel_motion_planner_amd import _lib as L

NAMES = ["smp_planner_set_scene_keys", "smp_planner_set_scene_bt", "smp_planner_set_scene_ot",
         "smp_planner_set_scene_octomap_msg"]


def test_lib_exposes_the_symbols():
    bound = {n for n, _, _ in L.EXPORTS}
    for n in NAMES:
        assert n in bound and hasattr(L.lib(), n)
    fields = [f for f, _ in L.SceneBuild._fields_]
    assert fields == ["dims", "origin", "resolution", "n_occupied", "bbox_min", "bbox_max", "kernel_ms", "total_ms"]


def test_header_declares_them():
    text = open(os.path.join(ROOT, "include", "smp_gpu.h")).read()
    for n in NAMES:
        assert re.search(r"\bint %s\(smp_planner\*" % n, text), n
    assert "typedef struct smp_scene_build" in text


def test_null_planner_is_an_argument_error():
    lib = L.lib()
    o = L.SceneOpts()
    lib.smp_scene_opts_default(ctypes.byref(o))
    keys = (ctypes.c_uint16 * 3)(32768, 32768, 32768)
    info = L.SceneBuild()
    data = ctypes.create_string_buffer(b"# Octomap OcTree binary file\nid OcTree\nsize 0\nres 0.05\ndata\n")
    assert lib.smp_planner_set_scene_keys(None, keys, 1, ctypes.byref(o), ctypes.byref(info)) == L.SMP_ERR_ARG
    assert lib.smp_planner_set_scene_bt(None, data, len(data.raw), ctypes.byref(o), None) == L.SMP_ERR_ARG
    assert lib.smp_planner_set_scene_ot(None, data, len(data.raw), ctypes.byref(o), None) == L.SMP_ERR_ARG
    assert lib.smp_planner_set_scene_octomap_msg(None, b"OcTree", 0.05, 1, data, 0, ctypes.byref(o), None) == L.SMP_ERR_ARG
