"""ctypes binding of the C ABI (include/smp_gpu.h) of libsmp_gpu.so.

This is the reference-side binding a maintainer would add: every call goes through the C ABI into the HIP
kernels.  There is no CPU fallback -- if the library is missing the import fails loudly, and without a GPU
smp_planner_create returns SMP_ERR_NO_DEVICE.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SMP_LIB") or os.path.join(HERE, "lib", "libsmp_gpu.so")  # SMP_LIB: experiment builds
MODEL_JSON = os.path.join(HERE, "data", "robotino_model.json")
SPHERES_JSON = os.path.join(HERE, "data", "robotino_spheres.json")

SMP_OK = 0
SMP_ERR_ARG = -1
SMP_ERR_START_INVALID = -2
SMP_ERR_GOAL_INVALID = -3
SMP_ERR_NO_SOLUTION = -4
SMP_ERR_HIP = -5
SMP_ERR_PARSE = -6
SMP_ERR_CAPACITY = -7
SMP_ERR_NO_DEVICE = -8

BUDGET_ITERATIONS = 0
BUDGET_SECONDS = 1
BUDGET_SAMPLES = 2

_d = ctypes.c_double
_i = ctypes.c_int
_i64 = ctypes.c_int64
_p = ctypes.c_void_p
_pd = ctypes.POINTER(ctypes.c_double)


class SceneOpts(ctypes.Structure):
    _fields_ = [("resolution", _d), ("z_offset", _d), ("insert_floor", _i), ("floor_center", _d * 2),
                ("floor_distance", _d)]


class Params(ctypes.Structure):
    _fields_ = [("near_threshold", _d), ("step_factor", _d), ("num_traj_segments", _i), ("max_near_nodes", _i),
                ("path_optimality_threshold", _d), ("tree_optimization", _i), ("informed_sampling", _i),
                ("node_capacity", _i64), ("helpers", _i), ("scout", _i)]


class Query(ctypes.Structure):
    _fields_ = [("start", _d * 8), ("goal", _d * 8), ("env_x", _d * 2), ("env_y", _d * 2), ("check_self", _i),
                ("check_map", _i), ("budget_kind", _i), ("budget", _d), ("seed", ctypes.c_uint64),
                ("query_id", ctypes.c_uint32)]


class Stats(ctypes.Structure):
    _fields_ = [("iterations", _i64), ("first_solution_iter", _i64), ("last_solution_iter", _i64),
                ("configs_checked", _i64), ("configs_valid", _i64), ("time_first_solution", _d), ("time_total", _d),
                ("cost_best", _d * 3), ("cost_theoretical", _d * 3), ("nodes_start", _i64), ("nodes_goal", _i64),
                ("edges_start", _i64), ("edges_goal", _i64), ("rewires_start", _i64), ("rewires_goal", _i64),
                ("connected_tree_is_start", ctypes.c_int32), ("conn_node_b", ctypes.c_int32),
                ("conn_node_a", ctypes.c_int32), ("nn_nodes_scanned", _i64), ("near_nodes_scanned", _i64),
                ("samples_precomputed", _i64), ("phase_seconds", _d * 32), ("scout_nn_hits", _i64),
                ("scout_near_hits", _i64), ("scout_edge_hits", _i64), ("scout_edge_misses", _i64),
                ("scout_wait_seconds", _d), ("scout_phase_seconds", _d * 32), ("helpers", ctypes.c_int32),
                ("scout", ctypes.c_int32), ("time_first_solution_host", _d), ("scout_conn_row_hits", _i64),
                ("scout_conn_batch_hits", _i64), ("scout_conn_ov_hits", _i64)]


class Result(ctypes.Structure):
    _fields_ = [("status", _i), ("n_waypoints", _i64), ("waypoints", _pd), ("stats", Stats), ("n_cost_rows", _i64),
                ("cost_rows", _pd)]


class IkRequest(ctypes.Structure):
    _fields_ = [("ee_pose", _d * 6), ("deviation", (_d * 2) * 6), ("q_init", _d * 8), ("max_iter", _i)]


class IkResult(ctypes.Structure):
    _fields_ = [("reached", _i), ("iterations", _i), ("fallback_iterations", _i), ("q", _d * 8), ("error", _d * 6),
                ("manipulability", _d)]


class GoalSearch(ctypes.Structure):
    _fields_ = [("n_candidates", _i), ("n_reached", _i), ("chosen", _i), ("downward", _i), ("kernel_ms", _d)]


class SceneDevice(ctypes.Structure):
    """smp_scene_device: a planner's device-resident scene (geometry, sizes, device pointers)."""
    _fields_ = [("dims", _i * 3), ("origin", _d * 3), ("resolution", _d), ("n_bricks", _i64), ("n_cells", _i64),
                ("n_prim", _i), ("has_d2b", _i), ("bricks", _p), ("d2", _p), ("d2b", _p), ("slab", _p)]


class SceneBuild(ctypes.Structure):
    """smp_scene_build: geometry, occupied cells and timing of a device scene build."""
    _fields_ = [("dims", _i * 3), ("origin", _d * 3), ("resolution", _d), ("n_occupied", _i64), ("bbox_min", _d * 3),
                ("bbox_max", _d * 3), ("kernel_ms", _d), ("total_ms", _d)]


class Attach(ctypes.Structure):
    """smp_attach: a grasped object as spheres in the frame of the link it is fixed to."""
    _fields_ = [("link", ctypes.c_char_p), ("name", ctypes.c_char_p), ("n_spheres", _i), ("centres", _pd),
                ("radii", _pd), ("touch_links", ctypes.POINTER(ctypes.c_char_p)), ("n_touch", _i)]


class Carve(ctypes.Structure):
    """smp_carve: the self filter -- the pose the map was taken at, the pad, the collision links to carve."""
    _fields_ = [("q", _d * 8), ("pad", _d), ("links", ctypes.POINTER(ctypes.c_char_p)), ("n_links", _i)]


class CarveInfo(ctypes.Structure):
    """smp_carve_info: carved keys and timing of the last carve."""
    _fields_ = [("n_carved", _i64), ("kernel_ms", _d), ("total_ms", _d)]


class ShortcutInfo(ctypes.Structure):
    """smp_shortcut_info: counts, costs and timing of one smp_shortcut_path call."""
    _fields_ = [("n_edges", _i64), ("n_valid", _i64), ("configs_checked", _i64), ("cost_in", _d), ("cost_out", _d),
                ("first_blocked", _i64), ("kernel_ms", _d), ("total_ms", _d)]


class Detour(ctypes.Structure):
    """smp_detour: one item (gap, sample) of smp_sample_detours."""
    _fields_ = [("v", _d * 8), ("M1", ctypes.c_int32), ("M2", ctypes.c_int32), ("free", ctypes.c_int32),
                ("pad", ctypes.c_int32)]


class RepairOpts(ctypes.Structure):
    """smp_repair_opts: samples per gap and round, rounds, Philox seed."""
    _fields_ = [("samples", _i), ("rounds", _i), ("seed", ctypes.c_uint64)]


class RepairInfo(ctypes.Structure):
    """smp_repair_info: counts, costs and timing of one smp_repair_path call."""
    _fields_ = [("n_blocked_edges", _i64), ("n_gaps", _i64), ("n_repaired", _i64), ("n_items", _i64), ("n_free", _i64),
                ("rounds_used", ctypes.c_int32), ("cost_in", _d), ("cost_out", _d), ("first_blocked", _i64),
                ("kernel_ms", _d), ("total_ms", _d)]


class Margin(ctypes.Structure):
    """smp_margin: the distances (metres) a margin check keeps from the map and from self-collision."""
    _fields_ = [("map", _d), ("self", _d)]


class Clearance(ctypes.Structure):
    """smp_clearance: map and self clearance of one configuration with the witness links."""
    _fields_ = [("map", _d), ("self", _d), ("map_link", ctypes.c_int32), ("self_a", ctypes.c_int32),
                ("self_b", ctypes.c_int32), ("pad", ctypes.c_int32)]


class EdgeClearance(ctypes.Structure):
    """smp_edge_clearance: the minima over a dense edge, the points and links attaining them."""
    _fields_ = [("map", _d), ("self", _d), ("map_point", ctypes.c_int32), ("self_point", ctypes.c_int32),
                ("map_link", ctypes.c_int32), ("self_a", ctypes.c_int32), ("self_b", ctypes.c_int32),
                ("n_points", ctypes.c_int32)]


class ClearanceInfo(ctypes.Structure):
    """smp_clearance_info: configurations evaluated and timing of one clearance call."""
    _fields_ = [("n_points", _i64), ("kernel_ms", _d), ("total_ms", _d)]


class BaseLattice(ctypes.Structure):
    """smp_base_lattice: the base's lattice (x, y, heading) with the arm joints held on it."""
    _fields_ = [("x0", _d), ("y0", _d), ("pitch", _d), ("nx", _i), ("ny", _i), ("theta0", _d), ("dtheta", _d),
                ("n_theta", _i), ("wrap_theta", _i), ("arm", _d * 5)]


class BaseMapInfo(ctypes.Structure):
    """smp_base_map_info: nodes, free nodes and timing of one smp_base_free_map call."""
    _fields_ = [("n_nodes", _i64), ("n_free", _i64), ("kernel_ms", _d), ("total_ms", _d)]


class RouteInfo(ctypes.Structure):
    """smp_route_info: the snapped end nodes (ix, iy, t), chain length, settled nodes and cost of one route search."""
    _fields_ = [("from_node", ctypes.c_int32 * 3), ("to_node", ctypes.c_int32 * 3), ("n_chain", _i64),
                ("n_settled", _i64), ("cost", _d)]


class FarOpts(ctypes.Structure):
    """smp_far_opts: lattice, handover distance, map margin, shortcut window and snapping of smp_plan_far."""
    _fields_ = [("pitch", _d), ("n_theta", _i), ("arm", _d * 5), ("handover_distance", _d), ("map_margin", _d),
                ("window", _i), ("snap_cells", _i), ("route_device", _i)]


class FieldInfo(ctypes.Structure):
    """smp_field_info: reached nodes, rounds, launches and timing of one cost-field solve on the device."""
    _fields_ = [("n_nodes", _i64), ("n_reached", _i64), ("rounds", _i), ("launches", _i), ("fell_back", _i),
                ("tile_runs", _i64), ("kernel_ms", _d), ("total_ms", _d)]


class FarInfo(ctypes.Structure):
    """smp_far_info: where smp_plan_far ended and what its stages reported."""
    _fields_ = [("stage", _i), ("map", BaseMapInfo), ("route", RouteInfo), ("handover_node", ctypes.c_int32 * 3),
                ("n_route_rows", _i64), ("check", ShortcutInfo), ("route_ms", _d), ("total_ms", _d)]


SMP_LATTICE_MAX_NODES = 1 << 26
FIELD_TILE = (16, 16, 8)  # smp_field_tile_shape: the nodes (ix, iy, t) one tile of the cost field owns
SMP_EDGE_MAX_POINTS = 1 << 20
SMP_EDGE_TABLE_MAX = 1 << 20

# (name, restype, argtypes) of every symbol declared in include/smp_gpu.h
EXPORTS = [
    ("smp_params_default", None, [ctypes.POINTER(Params)]),
    ("smp_scene_opts_default", None, [ctypes.POINTER(SceneOpts)]),
    ("smp_robot_create_json", _i, [ctypes.c_char_p, ctypes.POINTER(_p)]),
    ("smp_robot_create_urdf", _i, [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(_p)]),
    ("smp_robot_destroy", None, [_p]),
    ("smp_robot_num_links", _i, [_p]),
    ("smp_robot_link_name", ctypes.c_char_p, [_p, _i]),
    ("smp_robot_self_rounds", _i, [_p, _p, _p, _p, _p, _p, _p, _p]),
    ("smp_robot_attach", _i, [_p, ctypes.POINTER(Attach), ctypes.POINTER(_p)]),
    ("smp_cover_box", _i, [_pd, _pd, _d, _i, _pd, _pd, ctypes.POINTER(_i)]),
    ("smp_cover_cylinder", _i, [_d, _d, _pd, _d, _i, _pd, _pd, ctypes.POINTER(_i)]),
    ("smp_planner_set_robot", _i, [_p, _p]),
    ("smp_planner_set_carve", _i, [_p, ctypes.POINTER(Carve)]),
    ("smp_planner_last_carve", _i, [_p, ctypes.POINTER(CarveInfo)]),
    ("smp_carve_keys", _i, [_p, _p, _i64, ctypes.POINTER(SceneOpts), ctypes.POINTER(Carve), _p,
                            ctypes.POINTER(CarveInfo)]),
    ("smp_scene_from_keys", _i, [_p, _i64, ctypes.POINTER(SceneOpts), ctypes.POINTER(_p)]),
    ("smp_scene_from_bt", _i, [_p, ctypes.c_size_t, ctypes.POINTER(SceneOpts), ctypes.POINTER(_p)]),
    ("smp_scene_from_ot", _i, [_p, ctypes.c_size_t, ctypes.POINTER(SceneOpts), ctypes.POINTER(_p)]),
    ("smp_scene_from_octomap_msg", _i, [ctypes.c_char_p, _d, _i, _p, ctypes.c_size_t, ctypes.POINTER(SceneOpts),
                                        ctypes.POINTER(_p)]),
    ("smp_scene_from_grid", _i, [_p, _p, ctypes.POINTER(_i), _pd, _d, ctypes.POINTER(_p)]),
    ("smp_scene_destroy", None, [_p]),
    ("smp_scene_info", _i, [_p, ctypes.POINTER(_i), _pd, _pd, ctypes.POINTER(_i64), _pd, _pd]),
    ("smp_scene_export", _i, [_p, _p, _p]),
    ("smp_planner_create", _i, [_i, _p, ctypes.POINTER(Params), ctypes.POINTER(_p)]),
    ("smp_planner_destroy", None, [_p]),
    ("smp_planner_set_scene", _i, [_p, _p]),
    ("smp_planner_set_scene_keys", _i, [_p, _p, _i64, ctypes.POINTER(SceneOpts), ctypes.POINTER(SceneBuild)]),
    ("smp_planner_set_scene_bt", _i, [_p, _p, ctypes.c_size_t, ctypes.POINTER(SceneOpts), ctypes.POINTER(SceneBuild)]),
    ("smp_planner_set_scene_ot", _i, [_p, _p, ctypes.c_size_t, ctypes.POINTER(SceneOpts), ctypes.POINTER(SceneBuild)]),
    ("smp_planner_set_scene_octomap_msg", _i, [_p, ctypes.c_char_p, _d, _i, _p, ctypes.c_size_t,
                                               ctypes.POINTER(SceneOpts), ctypes.POINTER(SceneBuild)]),
    ("smp_planner_set_params", _i, [_p, ctypes.POINTER(Params)]),
    ("smp_planner_get_params", _i, [_p, ctypes.POINTER(Params)]),
    ("smp_set_disabled_map_links", _i, [_p, ctypes.POINTER(ctypes.c_char_p), _i]),
    ("smp_plan", _i, [_p, ctypes.POINTER(Query), ctypes.POINTER(Result)]),
    ("smp_plan_batch", _i, [_p, ctypes.POINTER(Query), _i, ctypes.POINTER(Result)]),
    ("smp_plan_multi", _i, [ctypes.POINTER(_p), _i, ctypes.POINTER(Query), _i, ctypes.POINTER(Result)]),
    ("smp_planner_scene_device", _i, [_p, ctypes.POINTER(SceneDevice)]),
    ("smp_planner_set_scene_device", _i, [_p, ctypes.POINTER(SceneDevice)]),
    ("smp_planners_share_scene", _i, [ctypes.POINTER(_p), _i, _i]),
    ("smp_result_free", None, [ctypes.POINTER(Result)]),
    ("smp_get_tree", _i64, [_p, _i, _p, _p, _p]),
    ("smp_check_configs", _i, [_p, _pd, _i64, _i, _i, _p]),
    ("smp_is_config_valid", _i, [_p, _pd, _i, _i, ctypes.POINTER(_i)]),
    ("smp_check_sequence", _i, [_p, _pd, _i64, _i, _i, ctypes.POINTER(_i64)]),
    ("smp_get_collisions", _i, [_p, _pd, ctypes.POINTER(ctypes.c_int32), _i, ctypes.POINTER(_i),
                                ctypes.POINTER(ctypes.c_int32), _i, ctypes.POINTER(_i)]),
    ("smp_check_edges", _i, [_p, _pd, _pd, _i64, _i, _i, ctypes.POINTER(_i64), ctypes.POINTER(ctypes.c_int32)]),
    ("smp_shortcut_path", _i, [_p, _pd, _i64, _i, _i, _i, ctypes.POINTER(_pd), ctypes.POINTER(_i64),
                               ctypes.POINTER(ShortcutInfo)]),
    ("smp_sample_detours", _i, [_p, _pd, _pd, _i64, _i, _d, ctypes.c_uint64, ctypes.c_uint32, _i, _i,
                                ctypes.POINTER(Detour)]),
    ("smp_repair_opts_default", None, [ctypes.POINTER(RepairOpts)]),
    ("smp_repair_path", _i, [_p, _pd, _i64, _i, _i, ctypes.POINTER(RepairOpts), ctypes.POINTER(_pd),
                             ctypes.POINTER(_i64), ctypes.POINTER(RepairInfo)]),
    ("smp_buffer_free", None, [_p]),
    ("smp_clearance_configs", _i, [_p, _pd, _i64, _d, _i, _i, ctypes.POINTER(Clearance),
                                   ctypes.POINTER(ClearanceInfo)]),
    ("smp_clearance_edges", _i, [_p, _pd, _pd, _i64, _d, _i, _i, ctypes.POINTER(EdgeClearance),
                                 ctypes.POINTER(ClearanceInfo)]),
    ("smp_check_configs_margin", _i, [_p, _pd, _i64, _i, _i, ctypes.POINTER(Margin), _p]),
    ("smp_check_edges_margin", _i, [_p, _pd, _pd, _i64, _i, _i, ctypes.POINTER(Margin), ctypes.POINTER(_i64),
                                    ctypes.POINTER(ctypes.c_int32)]),
    ("smp_sample_detours_margin", _i, [_p, _pd, _pd, _i64, _i, _d, ctypes.c_uint64, ctypes.c_uint32, _i, _i,
                                       ctypes.POINTER(Margin), ctypes.POINTER(Detour)]),
    ("smp_shortcut_path_margin", _i, [_p, _pd, _i64, _i, _i, _i, ctypes.POINTER(Margin), ctypes.POINTER(_pd),
                                      ctypes.POINTER(_i64), ctypes.POINTER(ShortcutInfo)]),
    ("smp_repair_path_margin", _i, [_p, _pd, _i64, _i, _i, ctypes.POINTER(RepairOpts), ctypes.POINTER(Margin),
                                    ctypes.POINTER(_pd), ctypes.POINTER(_i64), ctypes.POINTER(RepairInfo)]),
    ("smp_base_lattice_fit", _i, [_pd, _pd, _d, _i, _d, _pd, ctypes.POINTER(BaseLattice)]),
    ("smp_base_free_map", _i, [_p, ctypes.POINTER(BaseLattice), ctypes.POINTER(Margin), _p,
                               ctypes.POINTER(BaseMapInfo)]),
    ("smp_base_route", _i, [ctypes.POINTER(BaseLattice), _p, _pd, _pd, _i, ctypes.POINTER(_pd), ctypes.POINTER(_i64),
                            ctypes.POINTER(ctypes.POINTER(ctypes.c_int32)), ctypes.POINTER(RouteInfo)]),
    ("smp_base_cost_field", _i, [_p, ctypes.POINTER(BaseLattice), _p, ctypes.POINTER(ctypes.c_int32), _pd,
                                 ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(FieldInfo)]),
    ("smp_base_route_gpu", _i, [_p, ctypes.POINTER(BaseLattice), _p, _pd, _pd, _i, ctypes.POINTER(_pd),
                                ctypes.POINTER(_i64), ctypes.POINTER(ctypes.POINTER(ctypes.c_int32)),
                                ctypes.POINTER(RouteInfo), ctypes.POINTER(FieldInfo)]),
    ("smp_field_tile_shape", None, [ctypes.POINTER(ctypes.c_int)]),
    ("smp_far_opts_default", None, [ctypes.POINTER(FarOpts)]),
    ("smp_plan_far", _i, [_p, ctypes.POINTER(Query), ctypes.POINTER(FarOpts), ctypes.POINTER(Result),
                          ctypes.POINTER(FarInfo)]),
    ("smp_normalize_trajectory", _i, [_pd, _i64, _i, _pd, _pd, _i64, ctypes.POINTER(_i64)]),
    ("smp_ik_solve", _i, [_p, ctypes.POINTER(IkRequest), _i, ctypes.POINTER(IkResult)]),
    ("smp_find_goal_pose", _i, [_p, _pd, _pd, _d, _i, _i, _pd, ctypes.POINTER(_i), ctypes.POINTER(GoalSearch)]),
    ("smp_last_kernel_ms", _i, [_p, _pd, _pd, ctypes.POINTER(_i64)]),
    ("smp_strerror", ctypes.c_char_p, [_i]),
]

PROBES = [
    ("smp_probe_sincos", _i, [_i, _pd, _i, _pd, _pd]),
    ("smp_probe_u01", _i, [_i, ctypes.c_uint64, ctypes.c_uint32, _p, _i, _pd]),
    ("smp_probe_fk", _i, [_p, _pd, _i, _pd, _pd]),
    ("smp_probe_sqrt_div", _i, [_i, _pd, _pd, _i, _pd, _pd]),
    ("smp_probe_near", _i, [_i, _pd, _pd, _i, _pd, _p, _i, ctypes.c_double, _i, _p, _p, _p, _p,
                            ctypes.POINTER(ctypes.c_uint64), _pd]),
    ("smp_probe_check_latency", _i, [_p, _pd, _i64, _i, _i, _i, _i, _pd, ctypes.POINTER(ctypes.c_uint64), _pd]),
    ("smp_probe_check_shape", _i, [_p, _pd, _i64, _i, _i, _i, _i, _p]),
    ("smp_probe_export_tree", _i, [_p, _i, _p, _p, _pd, _pd]),
    ("smp_probe_export_state", _i, [_p, _p, _pd]),
    ("smp_probe_robot_dev", _i64, [_p, _p, _i64]),
    ("smp_probe_scene_slabs", _i64, [_p, _p, _p, _i64]),
]

_lib = None


def lib():
    """Load libsmp_gpu.so (build it with `make -C squirrel_motion_planner_amd` / __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libsmp_gpu.so not built at %s -- run __graft_entry__.build(); there is no CPU fallback"
                              % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        for name, res, args in EXPORTS + PROBES:
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


class SmpError(RuntimeError):
    def __init__(self, status, what=""):
        self.status = status
        msg = lib().smp_strerror(status).decode()
        super().__init__("%s%s (status %d)" % (what + ": " if what else "", msg, status))


def check(status, what=""):
    if status != SMP_OK:
        raise SmpError(status, what)
    return status
