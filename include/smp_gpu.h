/* smp_gpu.h -- C ABI of the MI355X BiRRT* sampling / collision hot path.
 *
 * Drop-in boundary for the planner core that squirrel_8dof_planner drives
 * (tpatten/squirrel_motion_planner).  Each entry point replaces one interface of the reference:
 *
 *   smp_robot_create_json      KDLRobotModel + CollisionChecker construction
 *                              (birrt_star.cpp:61-73, kdl_kuka_model.cpp:12-236, collision_checker.hpp:65-74)
 *   smp_robot_create_urdf      the same from robot_description / SRDF text (collision_checker.hpp:176-393)
 *   smp_robot_attach           a grasped object as one more collision link of a robot (the reference keeps "Planning
 *   smp_cover_box / _cylinder  with Attached Objects" as a commented-out stub, birrt_star.h:411-414), and sphere
 *   smp_planner_set_robot      covers of a bounding box / cylinder; the planner's robot swapped in place, scene kept
 *   smp_planner_set_carve      the self filter the node's octomap needs before setOctree (the fetched map holds the
 *   smp_carve_keys             arm's and the grasped object's voxels): the robot's volume at the pose the map was
 *   smp_planner_last_carve     taken carved out of the key list inside the device scene build, or as a mask
 *   smp_scene_from_keys        BiRRTstarPlanner::setOctree -> CollisionChecker::setOcTree
 *                              (birrt_star.cpp:1621-1624, collision_checker.hpp:76-88) for occupied leaf keys
 *   smp_scene_from_bt          the same from an octomap binary (.bt / binary octomap_msgs payload), with the
 *                              node's floor insertion (squirrel_8dof_planner.cpp:862-917)
 *   smp_scene_from_ot          the same from an octomap full-format file (.ot, the octomap_server's input,
 *                              launch/simulation.launch:51)
 *   smp_scene_from_octomap_msg the same from an octomap_msgs/Octomap payload (id, resolution, binary flag, data):
 *                              binaryMsgToMap / fullMsgToMap (squirrel_8dof_planner.cpp:875-883)
 *   smp_scene_from_grid        the same from a broadcast grid (multi-GPU: one RCCL broadcast per scene)
 *   smp_planner_create         BiRRTstarPlanner::initialize (birrt_star.cpp:11-326) on one GPU
 *   smp_planner_set_scene      BiRRTstarPlanner::setOctree (copies; caller keeps ownership)
 *   smp_planner_set_scene_keys the node's map hand-off per request -- fetch the octomap, insert the floor, setOctree
 *   smp_planner_set_scene_bt   (squirrel_8dof_planner.cpp:862-917, collision_checker.hpp:76-88) -- with the scene built
 *   smp_planner_set_scene_ot   on the GPU: the keys (decoded on the host) are uploaded and every derived array is
 *   smp_planner_set_scene_octomap_msg  computed by kernels, bit for bit what smp_scene_from_* + smp_planner_set_scene give
 *   smp_set_disabled_map_links BiRRTstarPlanner::setDisabledLinkMapCollisions (birrt_star.cpp:6916-6919)
 *   smp_plan                   reset_planner_and_config + setPlanningSceneInfo + init_planner + run_planner
 *                              + getJointTrajectoryRef (squirrel_8dof_planner.cpp:1221-1248,
 *                              birrt_star.cpp:335-536, 983-1407, 1688-1691)
 *   smp_plan_batch             independent queries against one scene (one workgroup each)
 *   smp_plan_multi             the same over several planners / GPUs of one process (the node is one process:
 *                              squirrel_8dof_planner_node.cpp:6-15), queries dealt round-robin
 *   smp_planner_scene_device   setOctree's copy of the map for further GPUs: the planner's device-resident scene
 *   smp_planner_set_scene_device  (RCCL broadcast between ranks, xGMI peer copies between planners) instead of a
 *   smp_planners_share_scene   host rebuild per GPU
 *   smp_check_configs          batched isConfigValid (birrt_star.cpp:6897-6908) -> valid flags
 *   smp_is_config_valid        BiRRTstarPlanner::isConfigValid for one configuration
 *   smp_get_collisions         BiRRTstarPlanner::getCollisions (birrt_star.cpp:6910-6914 -> collision_checker.hpp:
 *                              123-132, 594-630): colliding self pairs and map-colliding links of one configuration
 *   smp_check_sequence         the node's keyframe loops over isConfigValid (fold / unfold arm,
 *                              squirrel_8dof_planner.cpp:759-784, 814-823): first invalid pose, one kernel launch
 *   smp_check_edges            batched BiRRTstarPlanner::isEdgeValid (birrt_star.h:103-104, birrt_star.cpp:6864-6895):
 *                              every edge interpolated as connectNodesInterpolation does (birrt_star.cpp:4443-4526),
 *                              hop by hop of at most one planner step -> index of the first colliding point
 *   smp_shortcut_path          a simplification pass over a finished path (the reference has none: the node resamples
 *                              getJointTrajectoryRef as it is, squirrel_8dof_planner.cpp:1238-1248): every waypoint
 *                              pair as one dense edge check, then the cheapest route (edge cost as DH:128-156)
 *   smp_sample_detours         one-via detours a -> v -> b for a table of gaps: samples drawn and both legs checked
 *                              densely on the device, one launch (the reference has no counterpart)
 *   smp_repair_path            a repair pass over a path that fails the dense check: blocked stretches gathered into
 *                              gaps between valid waypoints, each bridged by the cheapest free detour
 *   smp_buffer_free            releases smp_shortcut_path's and smp_repair_path's output
 *   smp_clearance_configs      distance of a batch of configurations to the map and to self-collision, with the
 *                              witness links, one launch (the reference has no counterpart: getCollisions lists
 *                              contacts only once they exist)
 *   smp_clearance_edges        the same along dense edges of the density rule: each edge's minima, the points and the
 *                              links attaining them, one launch (the reference has no counterpart)
 *   smp_base_free_map          the first stage of the node's two-stage planner (squirrel_8dof_planner.h:50), a 2-D base
 *   smp_base_route             path with the arm folded and 8 DoF only for the last distance_birrt_star_planning metres.
 *   smp_plan_far               In the reference that branch is dead: both service callbacks print "COMBINED 2DOF AND
 *                              8DOF PLANNING NOT IMPLEMENTED!" and return false (squirrel_8dof_planner.cpp:505-508,
 *                              595-598).  Here: the base's free space as a slice of C-space, every lattice node
 *                              (x, y, theta, folded arm) answered by the real checker in one launch; a Dijkstra route
 *                              over the bit grid on the host; the route checked densely, then smp_plan for the tail
 *                              (the pop-back loop of squirrel_8dof_planner.cpp:1209-1215 chooses the handover)
 *   smp_normalize_trajectory   Planner::normalizeTrajectory (squirrel_8dof_planner.cpp:1557-1637), host only
 *   smp_ik_solve               BiRRTstarPlanner::getFullPoseFromEEPose (birrt_star.cpp:1627-1686) ->
 *                              RobotController::run_VDLS_Control_Connector (control_laws.cpp:3283-3712):
 *                              n independent controller runs, one wavefront each
 *   smp_find_goal_pose         Planner::findGoalPose (squirrel_8dof_planner.cpp:1129-1201): every candidate base
 *                              angle's controller run at once, each REACHED pose checked in the same kernel, the
 *                              first valid one in the reference's order (later candidates stop once it is known)
 *   smp_result_free            releases library-owned result buffers
 *   smp_strerror               text of a status code
 *
 * Conventions: the caller owns every input buffer; results are library-allocated and released with
 * smp_result_free.  Every function returns SMP_OK (0) or a negative status.  One smp_planner per host
 * thread (the reference planner is not thread-safe either, squirrel_8dof_planner_node.cpp:12).
 * Configurations are 8 fp64 values in chain order [x, y, theta, arm1..arm5].
 */
#ifndef SMP_GPU_H
#define SMP_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  SMP_OK = 0,
  SMP_ERR_ARG = -1,           /* bad argument / dimension mismatch (birrt_star.cpp:338-342) */
  SMP_ERR_START_INVALID = -2, /* start configuration in collision (birrt_star.cpp:353-357) */
  SMP_ERR_GOAL_INVALID = -3,  /* goal configuration in collision (birrt_star.cpp:358-362) */
  SMP_ERR_NO_SOLUTION = -4,   /* budget exhausted without a path (birrt_star.cpp:1405) */
  SMP_ERR_HIP = -5,           /* HIP runtime error, or a launch the call gave up waiting for (a seconds budget's
                                 4x + 60 s): the planner then sets its abort word, which every leader polls each 64
                                 iterations, and answers SMP_ERR_HIP to every call until that launch has drained */
  SMP_ERR_PARSE = -6,         /* model / octomap parse error */
  SMP_ERR_CAPACITY = -7,      /* tree capacity exceeded (raise smp_params.node_capacity) */
  SMP_ERR_NO_DEVICE = -8      /* no usable GPU: the library never falls back to the CPU */
};

enum { SMP_BUDGET_ITERATIONS = 0, SMP_BUDGET_SECONDS = 1, SMP_BUDGET_SAMPLES = 2 };

typedef struct smp_robot smp_robot;
typedef struct smp_scene smp_scene;
typedef struct smp_planner smp_planner;

typedef struct smp_scene_opts {
  double resolution;      /* metres per voxel (used by smp_scene_from_keys) */
  double z_offset;        /* octree transform z (collision_checker.hpp:87: -0.02) */
  int insert_floor;       /* 1: insert the node's floor square (squirrel_8dof_planner.cpp:889-902) */
  double floor_center[2]; /* robot x, y at planning time */
  double floor_distance;  /* floor_collision_distance (parameters.yaml:24: 3.0) */
} smp_scene_opts;

typedef struct smp_params {
  double near_threshold;   /* near_threshold_interpolation (birrt_star.cpp:183, default 4.0) */
  double step_factor;      /* unconstraint_extend_step_factor (birrt_star.cpp:189, default 0.5) */
  int num_traj_segments;   /* num_traj_segments_interp (birrt_star.cpp:186, default 20) */
  int max_near_nodes;      /* max_near_nodes (birrt_star.cpp:195, default 20) */
  double path_optimality_threshold; /* birrt_star.cpp:201 (default 1.0) */
  int tree_optimization;   /* m_tree_optimization_active (default 1) */
  int informed_sampling;   /* m_informed_sampling_active (default 1) */
  int64_t node_capacity;   /* per-tree node capacity on the device (0: derived from the budget) */
  int helpers;             /* helper workgroups per query that share its collision tiles across CUs
                              (0: automatic, up to 200 with scouts / 63 without; -1: none, the query runs on
                              its own workgroup) */
  int scout;               /* 1 (default): scout workgroups compute the coming iterations' scans and collision jobs
                              ahead of the leader -- 4 when a query has 64 CUs or more, 2 from 18 CUs, 1 from 6
                              (before the first solution they take the iterations in turn; after it scouts 0 and 1
                              alternate, two ahead, and the others retire); 2..8: that many (with >= 4 helpers);
                              0: off.  Results are identical either way */
} smp_params;

typedef struct smp_query {
  double start[8];
  double goal[8];
  double env_x[2];         /* setPlanningSceneInfo size_x (0,0 = unconfined) */
  double env_y[2];
  int check_self;
  int check_map;
  int budget_kind;         /* SMP_BUDGET_*: iterations (flag_iter_or_time = 0), seconds (= 1), or
                              collision-checked configurations (checked before each iteration) */
  double budget;
  uint64_t seed;
  uint32_t query_id;       /* RNG stream of this query */
} smp_query;

typedef struct smp_stats {
  int64_t iterations;
  int64_t first_solution_iter;   /* -1 if none */
  int64_t last_solution_iter;
  int64_t configs_checked;       /* isInCollision calls of the reference semantics */
  int64_t configs_valid;         /* ... of which collision free */
  double time_first_solution;    /* seconds from the kernel's planning start (device clock; see also
                                    time_first_solution_host) */
  double time_total;             /* seconds of the planning loop (device clock) */
  double cost_best[3];           /* total, revolute, prismatic.  The total is the value the reference commits
                                    (birrt_star.cpp:2651-2668, 3267): the cost of the straight edge x_connect -> x_new
                                    on top of the two tree costs, plus later reductions, while the nodes it inserts are
                                    the stepped via chain, which advances the revolute and the prismatic part at
                                    different rates and is bent in the 8-D norm.  It may therefore be less than the
                                    length of the returned path (measured: 10.4524 for a path of 10.5609, box room,
                                    seed 5, 3000 iterations).  The revolute and prismatic parts are the path's own. */
  double cost_theoretical[3];
  int64_t nodes_start, nodes_goal, edges_start, edges_goal, rewires_start, rewires_goal;
  int32_t connected_tree_is_start;
  int32_t conn_node_b, conn_node_a;
  int64_t nn_nodes_scanned;      /* nodes streamed by nearest-neighbour scans (64 B each) */
  int64_t near_nodes_scanned;    /* nodes streamed by near-vertex scans (72 B each) */
  int64_t samples_precomputed;   /* iterations whose sample came from the run-ahead sampler workgroup */
  double phase_seconds[32];      /* device time per planner phase (sample, nn, expand, near, choose-parent,
                                    rewire, connect, collision tiles, #tiles, edge costs, via chains, #via,
                                    tile stages, tile time per calling phase, then counts of checked
                                    configurations and of tile slots per calling phase) */
  int64_t scout_nn_hits;         /* nearest-neighbour scans answered from the scout's record */
  int64_t scout_near_hits;       /* near-vertex scans answered from the scout's record */
  int64_t scout_edge_hits;       /* needed edges whose collision check the scout had done */
  int64_t scout_edge_misses;     /* needed edges checked by the leader's own jobs while the scout was asked */
  double scout_wait_seconds;     /* time the leader waited for the scout */
  double scout_phase_seconds[32]; /* the scout's time per stage (0 sample, 1 nearest, 2 expand, 3 near, 4 choose,
                                    5 via chain, 6 rewire, 28 idle, 29 publishing, 31 busy; 30 = iterations) */
  int32_t helpers;               /* helper workgroups per query used */
  int32_t scout;                 /* scout workgroups per query used (0: none) */
  double time_first_solution_host; /* seconds from smp_plan entry until the host saw the first feasible path (host
                                    clock: start / goal checks, allocation, uploads and launch included; SURVEY 8d
                                    counts from run_planner entry, birrt_star.cpp:1075-1081); -1 if none */
  int64_t scout_conn_row_hits;   /* connects whose nearest node's row came from the scout's connect record */
  int64_t scout_conn_batch_hits; /* connects whose near candidates' rows came from the scout's connect record */
  int64_t scout_conn_ov_hits;    /* scout passes whose connect scan of tree_B ran under the rewire job
                                    (SMP_SCOUT_CONN_OV_MAX) */
} smp_stats;

typedef struct smp_result {
  int status;               /* SMP_OK or a negative code */
  int64_t n_waypoints;
  double* waypoints;        /* n_waypoints x 8, row-major (library-owned).  The first row is the start.  The last row is
                               the goal unless start and goal were connected before the first iteration: that path is
                               the start tree's via chain and, as the reference builds it (birrt_star.cpp:6246-6273),
                               ends one interpolation point before the goal */
  smp_stats stats;
  int64_t n_cost_rows;
  double* cost_rows;        /* n_cost_rows x 5: [iteration, time, c_best, c_rev, c_prism] (birrt_star.cpp:1325-1331) */
} smp_result;

void smp_params_default(smp_params* p);
void smp_scene_opts_default(smp_scene_opts* o);

int smp_robot_create_json(const char* model_json, smp_robot** out);
int smp_robot_create_urdf(const char* urdf_xml, const char* srdf_xml, const char* spheres_json, smp_robot** out);
void smp_robot_destroy(smp_robot* r);
int smp_robot_num_links(const smp_robot* r);
const char* smp_robot_link_name(const smp_robot* r, int i);
/* The model's self-collision lists and the round schedule of the job tiles' self test (read only).
 * info: n_sph, n_prim, n_spairs, n_ppairs, qualifies (1: the job tiles run the rounds, 0: the flat lists), rounds,
 * lanes, max_rounds.  Every array may be NULL: sp_ab[n_spairs] (a | b << 8) and sp_rr2[n_spairs], the flat sphere
 * pairs and their thresholds; pp_ps[n_ppairs] (primitive | sphere << 8); partner / rr2 [lanes * max_rounds], slot
 * lane * max_rounds + round: the other sphere of the pair that sphere `lane` owns in that round (-1: none) and the
 * threshold the tile forms for it, (r_lane + r_partner)^2; prim_mask[n_sph]: bit p set iff sphere s is paired with primitive p. */
int smp_robot_self_rounds(const smp_robot* r, int32_t info[8], uint16_t* sp_ab, double* sp_rr2, uint16_t* pp_ps,
                          int32_t* partner, double* rr2, uint32_t* prim_mask);

/* Attached objects (not in the reference: birrt_star.h:411-414 keeps "Planning with Attached Objects" as a stub).
 * A grasped object is one more collision link of the model, rigidly fixed to an existing link and covered by spheres
 * given in that link's frame.  smp_robot_attach leaves `base` untouched and returns a new robot (release it with
 * smp_robot_destroy); it composes, so a second object is attached to the result of the first.  The result is the
 * robot smp_robot_create_json builds from base's model with these additions, byte for byte in the device model:
 *   one link `name` after all links (parent `link`, fixed joint, identity frame); its spheres after all spheres, on
 *   the parent's body, centres carried into the body frame by the model generator's own arithmetic; one link bound
 *   (centre: componentwise mean, radius: max(distance + r) + 1e-6); one self pair (i, new) for every collision link i
 *   on another body than the parent's that is not a touch link, the pair list kept in lexicographic order.  Links on
 *   the parent's body are rigid to the object and get no pair, as everywhere else in the model.
 * SMP_ERR_ARG: a NULL argument, an unknown `link`, a `name` some link already has, a touch link that is unknown or
 * has no collision geometry, n_spheres < 1, a non-finite value, a radius <= 0 or > 0.45 m (the scene grids' padding),
 * a base model without its link tree.  SMP_ERR_CAPACITY: more spheres, collision links, link pairs, sphere pairs or
 * (primitive, sphere) pairs than the device model holds (72, 32, 256, 768, 320); for the committed robotino model
 * that is reached beyond 16 spheres on the hand.  Past 64 spheres and primitives together the job tiles run two items
 * per lane and the flat self lists instead of the self rounds (smp_robot_self_rounds, info[4] = 0): slower, same
 * results. */
typedef struct smp_attach {
  const char* link;        /* existing link the object is rigidly fixed to, e.g. "hand_palm_link" */
  const char* name;        /* name of the new collision link; must differ from every link name */
  int n_spheres;           /* >= 1 */
  const double* centres;   /* n x 3, in `link`'s frame */
  const double* radii;     /* n, each finite, > 0 and <= 0.45 */
  const char* const* touch_links; int n_touch;  /* collision links the object may overlap: no self pair with them */
} smp_attach;
int smp_robot_attach(const smp_robot* base, const smp_attach* a, smp_robot** out);
/* Conservative cover of a box (half extents) or of a cylinder upright in its own frame (radius, half length along z)
 * by at most max_spheres equal spheres on its longest axis (box: the lowest such axis; cylinder: z), for callers that
 * hold a bounding volume.  With ha the half length on that axis and rho the square root of the sum of squares of the
 * other two half extents (cylinder: the radius): m = min(max_spheres, max(1, ceil(ha / sqrt((rho + tol)^2 - rho^2))));
 * centre k sits at -ha + (2k + 1) * (ha / m) on the axis; every radius is sqrt((ha / m)^2 + rho^2), so the spheres
 * contain the volume for every m and overshoot it sideways by at most tol unless max_spheres caps m.  Every operation
 * is rounded on its own.  The centres are then mapped by pose (R row-major, then p; NULL: identity) into the link's
 * frame.  centres / radii hold max_spheres entries; *n receives m.  SMP_ERR_ARG: a NULL output, max_spheres < 1, a
 * non-finite value, an extent, radius or tol <= 0. */
int smp_cover_box(const double half[3], const double pose[12], double tol, int max_spheres,
                  double* centres, double* radii, int* n);
int smp_cover_cylinder(double radius, double half_length, const double pose[12], double tol, int max_spheres,
                       double* centres, double* radii, int* n);

int smp_scene_from_keys(const uint16_t* keys_xyz, int64_t n, const smp_scene_opts* opts, smp_scene** out);
int smp_scene_from_bt(const uint8_t* data, size_t size, const smp_scene_opts* opts, smp_scene** out);
/* Octomap full format (.ot): per node a float log-odds and a child-existence byte; leaves with log-odds >= 0 are
 * occupied.  Floor insertion (opts->insert_floor) leaves cells of free leaves free when one hit does not make them
 * occupied, as updateNode(key, true) does. */
int smp_scene_from_ot(const uint8_t* data, size_t size, const smp_scene_opts* opts, smp_scene** out);
/* octomap_msgs/Octomap fields: id must be "OcTree" (other tree types: SMP_ERR_PARSE, the node's "empty octomap"),
 * binary != 0: writeBinaryData payload, else writeData payload; neither carries a text header. */
int smp_scene_from_octomap_msg(const char* id, double resolution, int binary, const uint8_t* data, size_t size,
                               const smp_scene_opts* opts, smp_scene** out);
/* A scene from an exported grid (bitset + d2), e.g. after the RCCL broadcast of rank 0's scene. */
int smp_scene_from_grid(const uint64_t* bits, const uint16_t* d2, const int dims[3], const double origin[3],
                        double resolution, smp_scene** out);
void smp_scene_destroy(smp_scene* s);
/* Grid geometry of a scene: dims[3], origin[3], resolution; bitset/d2 copies for inspection (may be NULL). */
int smp_scene_info(const smp_scene* s, int dims[3], double origin[3], double* resolution,
                   int64_t* n_occupied, double bbox_min[3], double bbox_max[3]);
int smp_scene_export(const smp_scene* s, uint64_t* bits, uint16_t* d2);

int smp_planner_create(int device, const smp_robot* robot, const smp_params* params, smp_planner** out);
void smp_planner_destroy(smp_planner* p);
int smp_planner_set_scene(smp_planner* p, const smp_scene* s);
/* The same scene as smp_scene_from_keys / _bt / _ot / _octomap_msg followed by smp_planner_set_scene, built on the
 * planner's GPU (dilation, exact squared distance transform, bricks, byte field, slab fields as kernels on the
 * planner's stream); the resulting device arrays are identical.  Arguments, floor insertion and status codes are
 * those of the smp_scene_from_* call of the same name; on an argument or parse error the planner keeps its previous
 * scene.  Grids with a line of more than 32768 cells along y or z are left to the host path (SMP_ERR_ARG). */
typedef struct smp_scene_build {   /* may be NULL */
  int dims[3];
  double origin[3];
  double resolution;
  int64_t n_occupied;      /* distinct occupied cells, as smp_scene_info reports */
  double bbox_min[3], bbox_max[3];
  double kernel_ms;        /* HIP events around the build kernels on the planner's stream */
  double total_ms;         /* host clock, call entry to return (upload and final sync included) */
} smp_scene_build;
int smp_planner_set_scene_keys(smp_planner* p, const uint16_t* keys_xyz, int64_t n, const smp_scene_opts* opts,
                               smp_scene_build* info);
int smp_planner_set_scene_bt(smp_planner* p, const uint8_t* data, size_t size, const smp_scene_opts* opts,
                             smp_scene_build* info);
int smp_planner_set_scene_ot(smp_planner* p, const uint8_t* data, size_t size, const smp_scene_opts* opts,
                             smp_scene_build* info);
int smp_planner_set_scene_octomap_msg(smp_planner* p, const char* id, double resolution, int binary,
                                      const uint8_t* data, size_t size, const smp_scene_opts* opts,
                                      smp_scene_build* info);
/* Self filter (not in the reference): the robot's own volume carved out of an occupied key list on the GPU.  The
 * octomap the node fetches holds the arm's voxels and those of a grasped object, so the start pose is "in collision"
 * against its own image.  Definition: take the key list after floor insertion; its grid geometry (key of cell
 * (0, 0, 0), dims, origin o) is exactly what smp_planner_set_scene_keys computes for that list before any carving.
 * Key k sits at cell i = k - kmin, the box [o + i * res, o + (i + 1) * res] per axis.  With the world items of the
 * selected collision links at q formed as the checker forms them, k is carved iff some item's "Clearance queries" map
 * term against that single cell is <= pad: fl(fl(sqrt(gx^2 + gy^2 + gz^2)) - r) <= pad for a sphere, that section's
 * box or cylinder term for a primitive.  The comparison is non-strict, the exact complement of the margin checks'
 * strict >: after carving every link at (q, pad), smp_check_configs_margin(q, {pad, 0}) is clear of the map and
 * smp_clearance_configs(q, D).map > pad.  The link selection is independent of smp_set_disabled_map_links; links =
 * NULL / n_links = 0 selects every collision link, attached ones included.
 *   smp_carve_keys        one flag per caller key (1: carved).  Floor keys (opts->insert_floor) take part in the
 *                         geometry only.  n = 0: SMP_OK.
 *   smp_planner_set_carve the sticky form (copied; NULL turns it off): smp_planner_set_scene_keys, _bt, _ot and
 *                         _octomap_msg then clear the bits of the carved keys (floor keys included) between the
 *                         scatter of the keys and everything derived from the bit grid, so bricks, n_occupied,
 *                         dilation, distance fields and slabs see the carved occupancy; bbox_min / bbox_max stay
 *                         those of the full list.  The links are resolved by name at every build (the robot may
 *                         have been swapped since); on an error the planner keeps its previous scene.
 *                         smp_planner_set_scene and smp_planner_set_scene_device do not carve.
 *   smp_planner_last_carve  carved keys and timing of the last carving build or smp_carve_keys call.
 * SMP_ERR_ARG: a NULL planner or carve (smp_carve_keys), a non-finite q, a pad that is not finite or negative, a link
 * that is unknown or has no collision geometry, a non-positive resolution. */
typedef struct smp_carve {
  double q[8];                                /* the robot's pose when the map was taken */
  double pad;                                 /* metres; finite, >= 0 */
  const char* const* links; int n_links;      /* collision links to carve; 0 = every collision link, attached ones too */
} smp_carve;
typedef struct smp_carve_info { int64_t n_carved; double kernel_ms, total_ms; } smp_carve_info;  /* may be NULL */
int smp_planner_set_carve(smp_planner* p, const smp_carve* c);
int smp_planner_last_carve(const smp_planner* p, smp_carve_info* info);
int smp_carve_keys(smp_planner* p, const uint16_t* keys_xyz, int64_t n, const smp_scene_opts* opts,
                   const smp_carve* c, uint8_t* carved, smp_carve_info* info);
/* Planner parameters for subsequent smp_plan calls (activate/deactivateTreeOptimization,
 * activate/deactivateInformedSampling, birrt_star.h:57-63; setEdgeCostWeights keeps weights 1). */
int smp_planner_set_params(smp_planner* p, const smp_params* params);
int smp_planner_get_params(const smp_planner* p, smp_params* params);
int smp_set_disabled_map_links(smp_planner* p, const char* const* link_names, int n);
/* Swaps the planner's robot in place (not in the reference): after a grasp smp_planner_set_robot(p, attached), after
 * the release smp_planner_set_robot(p, base).  The device model is uploaded again (the SMP_SELF_FLAT override
 * included), the disabled-link set is kept by name (the object's own name may be in it) and the scene stays: its
 * byte field exists only while every sphere threshold is below 255, so it is derived from the box-gap field by one
 * kernel, or dropped, when the new spheres change that.  Trees and query buffers are untouched.  SMP_ERR_ARG: a NULL
 * argument, or a scene is set and the new robot's primitive tables (count, types, bodies, frames, extents) differ
 * from the current ones -- the slab fields belong to the primitives; attaching never changes them. */
int smp_planner_set_robot(smp_planner* p, const smp_robot* r);

/* Multi-GPU (queries shard, the scene is sent once per scene, no per-iteration collective).
 * The device-resident form of a planner's scene: the arrays smp_planner_set_scene derived for the planner's robot
 * (4x4x4 occupancy bricks, the box-gap field, its byte copy when every sphere threshold is below 255, one 2-D slab field
 * per exact primitive).  They move device to device: between ranks by an RCCL broadcast into caller buffers
 * (squirrel_motion_planner_amd/distributed.py), between the planners of one process by peer copies over xGMI
 * (smp_planners_share_scene).  The sender's and the receiver's robot must be the same model. */
typedef struct smp_scene_device {
  int dims[3];             /* cells x, y, z */
  double origin[3];
  double resolution;
  int64_t n_bricks;        /* uint64 words: ceil(x/4) * ceil(y/4) * ceil(z/4) */
  int64_t n_cells;         /* x * y * z: uint16 box-gap values (and bytes of the byte copy) */
  int n_prim;              /* slab planes of x * y uint16 values */
  int has_d2b;             /* the byte copy is part of the scene */
  uint64_t* bricks;        /* device pointers (any GPU of this process, or caller-owned buffers on the planner's GPU) */
  uint16_t* d2;
  uint8_t* d2b;
  uint16_t* slab;
} smp_scene_device;
/* Geometry and sizes of the planner's device scene; each non-NULL pointer of *io receives a device-to-device copy of
 * that array (caller-allocated, on any GPU).  SMP_ERR_ARG if the planner has no scene. */
int smp_planner_scene_device(const smp_planner* p, smp_scene_device* io);
/* Sets the planner's scene from device arrays laid out as above (copied: the caller keeps ownership); the robot-derived
 * parts must match this planner's robot (SMP_ERR_ARG otherwise).  Replaces smp_planner_set_scene on receiving ranks. */
int smp_planner_set_scene_device(smp_planner* p, const smp_scene_device* in);
/* ps[src]'s scene to every other planner of the array (peer copies over xGMI for planners on other GPUs). */
int smp_planners_share_scene(smp_planner* const* ps, int n, int src);

int smp_plan(smp_planner* p, const smp_query* q, smp_result* out);
int smp_plan_batch(smp_planner* p, const smp_query* q, int n, smp_result* out);
/* Independent queries over several planners (typically one per GPU, sharing a scene): query i runs on planner
 * i % n_planners, all planners concurrently (one host thread each); out[i] is query i's result, identical to what
 * smp_plan on that planner returns.  Each planner may appear once; planners on one GPU split that GPU's co-resident
 * workgroups among them for the call (each query's workgroups must all be resident).  Scenes set from grids
 * (smp_planner_set_scene / _device) must keep every occupied cell 0.45 m plus one cell from the grid's faces
 * (SMP_ERR_ARG otherwise): a sphere or primitive centred outside the grid is taken as free of the map. */
int smp_plan_multi(smp_planner* const* planners, int n_planners, const smp_query* q, int n, smp_result* out);
void smp_result_free(smp_result* r);

/* Tree dump of the last smp_plan (which: 0 start tree, 1 goal tree) for parity checks; arrays may be NULL. */
int64_t smp_get_tree(smp_planner* p, int which, int32_t* parent, double* conf, double* cost);

int smp_check_configs(smp_planner* p, const double* q_soa, int64_t n, int check_self, int check_map, uint8_t* valid);
int smp_is_config_valid(smp_planner* p, const double q[8], int check_self, int check_map, int* valid);
/* Every self pair that collides (2 link indices each, smp_robot_link_name, in the model's pair order -- the SRDF-enabled
 * link pairs i < j in link order, CC:378-388) and every collision link that touches the map (link indices in name
 * order, as the reference's std::map; disabled links included, CC:610-630).  Writes at most max_self pairs /
 * max_map links; *n_self / *n_map receive the full counts (the caller compares them with its capacity).
 * Rigid pairs are left out, here as in every validity check: the 65 SRDF-enabled pairs of links on one rigid body
 * (the reference's getSelfCollisions, CC:594-608, tests all 230) have the same relative pose in every configuration,
 * so their outcome does not depend on it; an overlapping one would make every configuration invalid in the
 * reference, and 7 of them overlap only under the conservative sphere covers (hand couplers / cranks against the
 * hand base and finger links, door against shell) -- tests/test_host_cpu.py pins both facts. */
int smp_get_collisions(smp_planner* p, const double q[8], int32_t* self_pairs, int max_self, int* n_self,
                       int32_t* map_links, int max_map, int* n_map);
/* n poses, row-major n x 8: *first_invalid = index of the first pose in collision, -1 if all are valid. */
int smp_check_sequence(smp_planner* p, const double* q_rows, int64_t n, int check_self, int check_map,
                       int64_t* first_invalid);
/* Dense edge checks.  The density rule, for an edge a -> b (8 values each), the planner's num_traj_segments n and
 * step_factor f: d[j] = b[j] - a[j]; L_rev = sqrt(sum of d[j]^2 over the revolute joints), L_pr the same over the
 * prismatic ones (each summed for j ascending); m = max(1, ceil(max(L_rev, L_pr) / f)) hops of at most one planner
 * step; M = n * m; point k (0..M) is a[j] + k * (d[j] / M), the quotient formed first, without contraction.  For m = 1
 * these are bit for bit the n + 1 configurations of the reference's edge trajectory (birrt_star.cpp:4443-4526); the via
 * nodes of an edge are its points n, 2n, ..., (m - 1) n.  Coordinates must be finite and an edge may have at most
 * SMP_EDGE_MAX_POINTS points (SMP_ERR_ARG otherwise). */
enum {
  SMP_EDGE_MAX_POINTS = 1 << 20,  /* points of one edge, M + 1 */
  SMP_EDGE_TABLE_MAX = 1 << 20    /* edges of one smp_check_edges call; waypoints and candidate pairs of one
                                     smp_shortcut_path call (all pairs: k <= 1448) */
};
/* Batched isEdgeValid (birrt_star.cpp:6864-6895): n edges from_rows[i] -> to_rows[i] (row-major n x 8), one kernel
 * launch.  first_invalid[i] = index of edge i's first colliding point, -1 if the edge is free (the reference's
 * last_valid_node_idx is then M, else max(first_invalid - 1, 0)); n_points[i] = M + 1 (may be NULL).  Honours
 * smp_set_disabled_map_links.  n = 0: SMP_OK.  check_map without a scene: SMP_ERR_ARG (a caller asking whether a
 * trajectory is free of the map must not be answered by the self test alone; smp_check_configs does answer so).
 * n > SMP_EDGE_TABLE_MAX: SMP_ERR_CAPACITY. */
int smp_check_edges(smp_planner* p, const double* from_rows, const double* to_rows, int64_t n, int check_self,
                    int check_map, int64_t* first_invalid, int32_t* n_points);

typedef struct smp_shortcut_info {   /* may be NULL */
  int64_t n_edges;          /* candidate pairs checked */
  int64_t n_valid;          /* ... of which free */
  int64_t configs_checked;  /* points up to and including the first colliding one per edge (smp_stats' convention) */
  double cost_in;           /* sum of dist(w_i, w_i+1), i ascending */
  double cost_out;          /* the dynamic program's cost of the chosen route (0 when blocked) */
  int64_t first_blocked;    /* blocked: the smallest i whose edge (i, i + 1) is invalid; else -1 */
  double kernel_ms;         /* HIP events around the edge kernel */
  double total_ms;          /* host clock, call entry to return */
} smp_shortcut_info;
/* Shortens a path of k waypoints (row-major k x 8).
 *  1. Candidates are all pairs (i, j), i < j, j - i <= window (window <= 0: all pairs), adjacent pairs included (the
 *     scene may have changed since the path was planned); each is one edge of the density rule and all are checked in
 *     one launch.
 *  2. dp[0] = 0; for j ascending and i ascending over the valid (i, j): c = dp[i] + dist(w_i, w_j), dist the 8-term sum
 *     for joints ascending followed by a square root (DH:128-156); the first strict minimum wins.
 *  3. Output: the chosen waypoints with the via nodes of each chosen edge between them, so every hop is at most one
 *     planner step and every row is a configuration that was collision-checked (the last waypoint as point M of its
 *     edges, a + M * (d / M), which can differ from it in the last bit).  *out_waypoints (n_out x 8) is allocated by the
 *     library: release it with smp_buffer_free.
 *  4. Waypoint k - 1 not reachable: SMP_ERR_NO_SOLUTION, info->first_blocked set, *out_waypoints = NULL, *n_out = 0.
 * k < 2: SMP_ERR_ARG (k = 2 is one candidate).  More than SMP_EDGE_TABLE_MAX waypoints or candidates:
 * SMP_ERR_CAPACITY (bound them with window).  check_map without a scene: SMP_ERR_ARG. */
int smp_shortcut_path(smp_planner* p, const double* waypoints, int64_t k, int check_self, int check_map, int window,
                      double** out_waypoints, int64_t* n_out, smp_shortcut_info* info);
void smp_buffer_free(void* buffer);  /* NULL is allowed */

/* Path repair: one-via detours around the blocked stretches of a path (the planner's own full paths can fail the dense
 * check, and the scene can change between planning and execution; smp_shortcut_path then only answers "blocked").
 *
 * One detour item (gap g, sample s) of a round: with the gap's anchors a and b, the half width h, the arm's joint limits
 * q_min / q_max and the planner's Philox draw u01 (seed, query = g, iteration = round, outer = s, inner = 0, index = j),
 *   c[j] = 0.5 * (a[j] + b[j]);  t = 2.0 * u01 - 1.0;  v[j] = c[j] + t * h;  v[j] clamped to [q_min[j], q_max[j]] for
 *   j >= 2 (x and y are not clamped: environment bounds belong to a query), every operation rounded on its own.
 * The legs a -> v and v -> b are edges of the density rule above (M1 and M2 segments, formed on the device); the item is
 * free if every point of both legs is.  A leg of more than SMP_EDGE_MAX_POINTS points makes the item blocked and is
 * reported with 0 segments. */
typedef struct smp_detour { double v[8]; int32_t M1, M2; int32_t free; int32_t pad; } smp_detour;
/* n_gaps pairs from_rows[g] -> to_rows[g]; out[g * samples + s]. One launch.  g in the Philox stream is the row index.
 * Honours smp_set_disabled_map_links.  n_gaps = 0: SMP_OK.  samples < 1, a non-finite coordinate or half width:
 * SMP_ERR_ARG.  check_map without a scene: SMP_ERR_ARG.  n_gaps * samples > SMP_EDGE_TABLE_MAX: SMP_ERR_CAPACITY. */
int smp_sample_detours(smp_planner* p, const double* from_rows, const double* to_rows, int64_t n_gaps,
                       int samples, double half_width, uint64_t seed, uint32_t round,
                       int check_self, int check_map, smp_detour* out);

typedef struct smp_repair_opts { int samples; int rounds; uint64_t seed; } smp_repair_opts;  /* NULL: defaults */
void smp_repair_opts_default(smp_repair_opts*);   /* samples 256, rounds 4, seed 1 */
typedef struct smp_repair_info {   /* may be NULL */
  int64_t n_blocked_edges, n_gaps, n_repaired, n_items, n_free;  /* blocked adjacent edges; gaps, of which closed;
                                                                     detour items checked over all rounds, of which free */
  int32_t rounds_used;      /* detour launches made (0 without a gap) */
  double cost_in, cost_out; /* sums of dist, i ascending, over the input rows / the route's rows (via nodes excluded);
                               cost_out is 0 when gaps stay open */
  int64_t first_blocked;    /* gaps stay open: the smallest blocked edge index of the first open gap; else -1 */
  double kernel_ms, total_ms;  /* HIP events around the check, edge and detour kernels; host clock, entry to return */
} smp_repair_info;
/* Repairs a path of k waypoints (row-major k x 8).
 *  1. Validity: the k waypoints through the batch checker (smp_check_configs), the k - 1 adjacent edges through the edge
 *     kernel (smp_check_edges).  w_0 invalid: SMP_ERR_START_INVALID; w_k-1 invalid: SMP_ERR_GOAL_INVALID.
 *  2. Gaps: for every blocked adjacent edge i, ascending, l = the largest index <= i whose waypoint is valid, r = the
 *     smallest index >= i + 1 whose waypoint is valid; gaps whose index ranges overlap (l' < r) are merged, so the gaps
 *     are disjoint and ordered.  Without a blocked edge the output is the input route with via nodes inserted.
 *  3. Rounds rho = 0 .. rounds - 1: one launch of detour items over the gaps still open (anchors w_l, w_r, g = the gap's
 *     index among all gaps, round = rho, h = step_factor * 2^rho).  Per gap the chosen sample is the first strict minimum,
 *     s ascending, of dist(a, v) + dist(v, b) over the free items (dist as in smp_shortcut_path, formed on the host from
 *     the returned v); a gap with a chosen sample is closed.
 *  4. Gaps open after the last round: SMP_ERR_NO_SOLUTION, info->first_blocked set, *out_waypoints = NULL, *n_out = 0.
 *  5. Output: the route w_0 ... w_l, v, w_r, ... (waypoints strictly inside a gap dropped) with the via nodes of every
 *     route edge between its rows, as smp_shortcut_path writes them: every row was collision-checked and every hop is at
 *     most one planner step.  Release *out_waypoints with smp_buffer_free.
 * k < 2, a non-finite coordinate, an edge of more than SMP_EDGE_MAX_POINTS points, samples < 1, rounds < 1 (or more than
 * 32): SMP_ERR_ARG.  check_map without a scene: SMP_ERR_ARG.  k or n_gaps * samples > SMP_EDGE_TABLE_MAX:
 * SMP_ERR_CAPACITY. */
int smp_repair_path(smp_planner* p, const double* waypoints, int64_t k, int check_self, int check_map,
                    const smp_repair_opts* opts, double** out_waypoints, int64_t* n_out, smp_repair_info* info);

/* Clearance queries: how far a configuration is from the map and from self-collision, and which links are nearest.
 * Every validity check above ends in a yes or no; these return the minimum behind it, with its witness.
 *
 * Definition, for a configuration q, a query distance D = max_dist and the planner's scene.  Body frames, sphere world
 * centres wc and primitive world centres / x axes pw are the checker's (KDL Frame * Frame, Frame * Vector).  Every
 * operation below is rounded on its own (no contraction), sums run left to right, and a minimum does not depend on the
 * order of the sweep: ties are settled on link indices (smp_robot_link_name), never on item order.
 *   gap(c, lo, hi) = c < lo ? lo - c : (c > hi ? c - hi : 0.0); cell (i, j, k) is the box lo = o + i * res,
 *   hi = o + (i + 1) * res per axis.
 *   Map term of sphere s (map-enabled link): min over the occupied cells of sqrt(gx*gx + gy*gy + gz*gz) - r_s, g the
 *     gaps of wc_s to the cell; negative = penetration depth.  A centre whose cell floor((wc - o) / res) lies outside
 *     the grid gives D (the boolean check takes such a sphere as free).
 *   Map term of primitive p (upright; half height hz, centre (px, py, pz), x axis (c, s)): min over the occupied cells of
 *     sqrt(dxy2 + dz*dz) with dz = max(zlo - (pz + hz), (pz - hz) - zhi, 0) and
 *       cylinder (radius h0): dxy = max(sqrt(qx*qx + qy*qy) - h0, 0), qx = gap(px, xlo, xhi), qy = gap(py, ylo, yhi);
 *         dxy2 = dxy*dxy;
 *       box (half extents h0, h1): dxy2 = 0 if none of the cell test's four separating-axis comparisons holds
 *         (|dx| > hw + (|c|*h0 + |s|*h1), |dy| > hw + (|s|*h0 + |c|*h1), |c*dx + s*dy| > h0 + hw*(|c| + |s|),
 *         |c*dy - s*dx| > h1 + hw*(|c| + |s|); hw = 0.5*res, dx = 0.5*(xlo + xhi) - px, dy likewise); else the least of
 *         eight squared distances: each corner (X, Y) of the cell's square to the solid rectangle, ex = X - px,
 *         ey = Y - py, lx = |c*ex + s*ey|, ly = |c*ey - s*ex|, qx = max(lx - h0, 0), qy = max(ly - h1, 0),
 *         qx*qx + qy*qy; and each corner ((px + sx*(c*h0)) - sy*(s*h1), (py + sx*(s*h0)) + sy*(c*h1)), sx, sy = +-1, of
 *         the rectangle to the square, gx*gx + gy*gy of its gaps.  (Two disjoint convex polygons attain their distance
 *         at a vertex of one of them.)
 *     A primitive overlapping a cell has term 0: primitives have no penetration depth.  A centre column outside the grid
 *     gives D.
 *   map = min(D, all map terms); map_link = the link of a term equal to it, the smallest link index among several,
 *     -1 when map == D.
 *   self = min over the model's self pairs (the flat lists of every validity check: sphere pairs and (primitive, sphere)
 *     pairs of the enabled, non-rigid link pairs) of
 *       sphere pair (a, b): sqrt(ex*ex + ey*ey + ez*ez) - (r_a + r_b), e = wc_a - wc_b;
 *       (primitive, sphere): sqrt(q2) - r_s, q2 the squared distance of the sphere's centre to the solid primitive as
 *         the validity check forms it (box: qx*qx + qy*qy + qz*qz; cylinder: qr*qr + qz*qz);
 *     uncapped.  self_a < self_b are the link indices of a pair attaining it, the lexicographically smallest (a, b)
 *     among equal minima.
 * sqrt is monotone and sqrt(fl(r * r)) == r, so a term > 0 means the boolean test of that item is free and a term < 0
 * that it collides; map == 0 arises from a primitive overlapping a cell and means colliding.
 * An edge is the points 0..M of the density rule (smp_check_edges): map and self are the minima over its points,
 * map_point / self_point the lowest point index attaining each (map_point = -1 when map == D), and the link fields are
 * those of that point.
 * Exactness of map against the true distance to the occupied cells: exact while every item centre is inside the grid,
 * or max_dist + reach <= the pad (reach: the item's radius, or the radius of the ball about a primitive's centre that
 * holds it; the pad: ceil(0.45 / res) + 2 cells around the occupied keys); otherwise an upper bound that may overstate,
 * because an item centred outside the grid gives D whatever its distance.  self has no such limit. */
typedef struct smp_clearance { double map, self; int32_t map_link, self_a, self_b, pad; } smp_clearance;            /* 32 B */
typedef struct smp_edge_clearance { double map, self; int32_t map_point, self_point, map_link, self_a, self_b, n_points; } smp_edge_clearance;  /* 40 B */
typedef struct smp_clearance_info { int64_t n_points; double kernel_ms, total_ms; } smp_clearance_info;             /* may be NULL */
/* n configurations (row-major n x 8), resp. n edges from_rows[i] -> to_rows[i]; one kernel launch each.  Both honour
 * smp_set_disabled_map_links.  A part not asked for reports map = max_dist, map_link = -1, resp. self = +inf,
 * self_a = self_b = -1 (and the point fields -1).  info->n_points: configurations evaluated (for edges the sum of
 * M + 1).  n = 0: SMP_OK.  SMP_ERR_ARG: a NULL planner or output, a non-finite coordinate, max_dist not finite or
 * <= 0, a max_dist whose largest prefilter threshold floor(((r + max_dist + 1e-6) / res)^2) reaches the clamp of the
 * box-gap field (65535; about 12.5 m at 5 cm), an edge of more than SMP_EDGE_MAX_POINTS points, with_map without a
 * scene (as smp_check_edges).  n > SMP_EDGE_TABLE_MAX: SMP_ERR_CAPACITY. */
int smp_clearance_configs(smp_planner* p, const double* q_rows, int64_t n, double max_dist, int with_self, int with_map,
                          smp_clearance* out, smp_clearance_info* info);
int smp_clearance_edges(smp_planner* p, const double* from_rows, const double* to_rows, int64_t n, double max_dist,
                        int with_self, int with_map, smp_edge_clearance* out, smp_clearance_info* info);

/* Margin checks: the path passes with a safety margin.  The validity checks answer "does it touch?", the clearance
 * queries "how far is it?"; these answer "is every point farther than the margin?", with the early exits of the former,
 * and carry that predicate through the dense edge check, the shortcut and the repair.
 *
 * Definition.  A configuration q is clear at the margins (mm, ms) = (margin->map, margin->self) under the flags
 * (check_self, check_map) iff all of
 *   1. it is valid by smp_check_configs with the same flags;
 *   2. if check_map and mm > 0: every map term of the "Clearance queries" definition above is > mm -- the same
 *      expressions in the same order, the same disabled links, a centre outside the grid is free; equivalently
 *      smp_clearance_configs(q, D).map > mm for any admissible D > mm;
 *   3. if check_self and ms > 0: every self term of that definition is > ms, i.e. .self > ms.
 * The comparison is made on the term as that definition rounds it, e.g. fl(fl(sqrt(s)) - r) > mm, and it is strict.  A
 * part whose margin is 0 is the boolean test of that part, untouched.  By the monotonicity note above (sqrt is monotone
 * and sqrt(fl(r * r)) == r) 2 and 3 imply 1 for a part whose margin is positive, so the kernel skips the boolean test of
 * that part; the tests compare against the conjunction.
 * An edge is clear iff all points 0..M of the density rule are; first_invalid is the lowest point that is not clear.
 * Exactness of the map part against the true distance to the occupied cells: exact while every item centre is inside
 * the grid, or margin + reach <= the pad (as under "Clearance queries"); otherwise an upper bound that may overstate:
 * an item centred outside the grid is clear whatever its distance.  The boolean checks are exact everywhere.
 * SMP_ERR_ARG: a margin that is not finite or is negative; a map margin whose largest prefilter threshold
 * floor(((r + mm + 1e-6) / res)^2) reaches the clamp of the box-gap field (the rule of smp_clearance_* for max_dist); a
 * positive map margin with check_map and no scene.  A NULL margin or {0, 0} gives results identical to the plain entry
 * point in every output field (a margin of a part not asked for counts as 0).
 *
 * Each entry point takes the plain call's arguments plus the margin; semantics, errors, capacities, info records and
 * output rows are those of the plain call with "valid / free" read as "clear" (smp_repair_path_margin: an unclear first
 * or last waypoint gives SMP_ERR_START_INVALID / SMP_ERR_GOAL_INVALID).  smp_check_configs_margin takes its
 * configurations row-major (n x 8) and writes clear[i] = 1 iff configuration i is clear. */
typedef struct smp_margin { double map, self; } smp_margin;   /* metres; NULL means {0, 0} */
int smp_check_configs_margin(smp_planner* p, const double* q_rows, int64_t n, int check_self, int check_map,
                             const smp_margin* margin, uint8_t* clear);
int smp_check_edges_margin(smp_planner* p, const double* from_rows, const double* to_rows, int64_t n, int check_self,
                           int check_map, const smp_margin* margin, int64_t* first_invalid, int32_t* n_points);
int smp_sample_detours_margin(smp_planner* p, const double* from_rows, const double* to_rows, int64_t n_gaps,
                              int samples, double half_width, uint64_t seed, uint32_t round, int check_self,
                              int check_map, const smp_margin* margin, smp_detour* out);
int smp_shortcut_path_margin(smp_planner* p, const double* waypoints, int64_t k, int check_self, int check_map,
                             int window, const smp_margin* margin, double** out_waypoints, int64_t* n_out,
                             smp_shortcut_info* info);
int smp_repair_path_margin(smp_planner* p, const double* waypoints, int64_t k, int check_self, int check_map,
                           const smp_repair_opts* opts, const smp_margin* margin, double** out_waypoints,
                           int64_t* n_out, smp_repair_info* info);

/* Far goals: the base lattice, the route over it and the staged plan (the reference's two-stage planner,
 * squirrel_8dof_planner.h:50, whose branch is dead there: squirrel_8dof_planner.cpp:505-508, 595-598).
 *
 * The lattice.  Node (ix, iy, t) is the configuration [x0 + ix * pitch, y0 + iy * pitch, theta0 + t * dtheta, arm[0..4]]:
 * the integer converted to double, then the product, then the sum, each rounded on its own (formed on the device; no
 * table of configurations is uploaded).  Node number n = (t * ny + iy) * nx + ix, N = nx * ny * n_theta.
 * smp_base_lattice_fit (host only): x0 = env_x[0], nx = (int)floor((env_x[1] - env_x[0]) / pitch) + 1, y likewise,
 * dtheta = (2.0 * M_PI) / n_theta, wrap_theta = 1.  SMP_ERR_ARG: a NULL argument, a non-finite value, pitch <= 0,
 * n_theta < 1, a reversed interval; SMP_ERR_CAPACITY: more than SMP_LATTICE_MAX_NODES nodes.
 *
 * smp_base_free_map.  Bit n % 32 of word n / 32 of free_bits (ceil(N / 32) words; the unused bits of the last word are
 * 0) is 1 iff smp_check_configs(q_n, check_self = 0, check_map = 1) says valid, or, with margin->map > 0, iff
 * smp_check_configs_margin(q_n, 0, 1, {margin->map, 0}) says clear (margin->self is ignored; NULL means no margin) --
 * bit for bit those calls' answers: the same tile on the same values, the disabled links of smp_set_disabled_map_links
 * honoured, an item centred outside the grid free.  The arm's self test is not part of the map: the route's dense
 * check in smp_plan_far carries it.  One launch, one workgroup per 32 consecutive nodes, each storing its own word.
 * SMP_ERR_ARG: a NULL planner, lattice or output, a non-finite field, pitch <= 0, a count < 1, no scene, a margin that
 * smp_check_configs_margin refuses.  SMP_ERR_CAPACITY: N > SMP_LATTICE_MAX_NODES. */
enum { SMP_LATTICE_MAX_NODES = 1 << 26 };
typedef struct smp_base_lattice {
  double x0, y0, pitch;     /* node (ix, iy): x = x0 + ix * pitch, y = y0 + iy * pitch; pitch finite, > 0 */
  int nx, ny;               /* >= 1 */
  double theta0, dtheta;    /* heading t: theta0 + t * dtheta */
  int n_theta;              /* >= 1 */
  int wrap_theta;           /* 1: headings 0 and n_theta - 1 are neighbours (a full circle) */
  double arm[5];            /* arm joints held on the lattice (pose_folded_arm) */
} smp_base_lattice;
typedef struct smp_base_map_info { int64_t n_nodes, n_free; double kernel_ms, total_ms; } smp_base_map_info; /* may be NULL */
int smp_base_lattice_fit(const double env_x[2], const double env_y[2], double pitch, int n_theta, double theta0,
                         const double arm[5], smp_base_lattice* out);
int smp_base_free_map(smp_planner* p, const smp_base_lattice* lat, const smp_margin* margin, uint32_t* free_bits,
                      smp_base_map_info* info);

/* smp_base_route (host only): the cheapest route over the free nodes of a lattice.
 *  Snapping of from / to (x, y, theta): ix = (int)floor((x - x0) / pitch + 0.5), iy likewise,
 *   t = (int)floor((theta - theta0) / dtheta + 0.5), taken modulo n_theta with wrap_theta; an index outside the lattice:
 *   SMP_ERR_ARG.  A blocked node is replaced from the square rings r = 1 .. snap_cells of its heading layer, ascending:
 *   within a ring the free node with the least (ix - ix0)^2 + (iy - iy0)^2, ties to the smaller node number.  None:
 *   SMP_ERR_START_INVALID for from, SMP_ERR_GOAL_INVALID for to.
 *  Graph: the 4 axis steps (weight pitch); the 4 diagonal steps (weight sqrt(pitch * pitch + pitch * pitch)) only where
 *   both axis cells between the two nodes are free in that layer; the heading steps t - 1, t + 1 at the same (ix, iy)
 *   (weight fabs(dtheta)), wrapping iff wrap_theta and n_theta > 1 -- the reference's dist with weights 1.
 *  Search: Dijkstra.  The priority is the pair (cost, node number), ascending; a node is settled at its first pop;
 *   dp starts at +inf and is relaxed with dp[u] + w < dp[v], strict; neighbours are tried in the order -y, -x, +x, +y,
 *   (-x,-y), (+x,-y), (-x,+y), (+x,+y), t - 1, t + 1.  The search stops when to_node is settled; to_node never
 *   settled: SMP_ERR_NO_SOLUTION (from_node, to_node and n_settled are still reported).
 *  Output: *out_chain (n_chain x 3: ix, iy, t; may be NULL) holds every node from from_node to to_node; *out_rows
 *   (n_out x 8) the chain with runs of equal step (dix, diy, dt) merged -- a node is kept where the step changes, plus
 *   both ends -- each row the node's configuration as above; from_node == to_node gives one row.  Both are released
 *   with smp_buffer_free. */
typedef struct smp_route_info { int32_t from_node[3], to_node[3]; int64_t n_chain, n_settled; double cost; } smp_route_info;
int smp_base_route(const smp_base_lattice* lat, const uint32_t* free_bits, const double from[3], const double to[3],
                   int snap_cells, double** out_rows, int64_t* n_out, int32_t** out_chain, smp_route_info* info);

/* The cost field of a lattice: every node's cheapest cost from one source, on the device.
 * smp_base_cost_field.  cost[n] (N doubles): the least left-to-right fp64 sum of step weights over routes source -> n in
 *  smp_base_route's graph; +inf for a blocked or unreachable node.  parent[n] (N values): -1 for the source and for +inf
 *  nodes, else the neighbour u with cost[u] + w == cost[n] and the least (cost[u], u).  Either output may be NULL.  Equal
 *  bit for bit to smp_base_route's search run until its heap is empty: the field is the one solution of
 *  cost[v] = min_u fl(cost[u] + w) while every weight still moves the largest finite cost; a field where the least
 *  weight does not (fl(cost_max + w_min) == cost_max) is computed by the host search instead, fell_back = 1.
 *  The free bits (ceil(N / 32) words) are uploaded; rounds of a tile-resident relaxation run as separate launches until
 *  one changes nothing.  No scene is needed: the planner gives its device and stream.
 *  SMP_ERR_ARG: a NULL planner, lattice, map or source, what smp_base_route refuses in a lattice, a source outside the
 *  lattice or on a blocked node.  SMP_ERR_CAPACITY: N > SMP_LATTICE_MAX_NODES, or the device buffers cannot be had.
 *  SMP_ERR_HIP: a failing runtime call, or more than n_free + 1 rounds.
 * smp_base_route_gpu.  smp_base_route with the search on the device: the same snapping, statuses, chain, rows, cost and
 *  n_settled (the nodes n with (cost[n], n) <= (cost[to], to); every reachable node where to is not reached).  Only the
 *  chain, the cost and the counts are downloaded.  A NULL planner: SMP_ERR_ARG. */
typedef struct smp_field_info {
  int64_t n_nodes, n_reached;      /* reachable nodes, the source included */
  int rounds, launches, fell_back; /* rounds up to and including the one that changed nothing; round launches enqueued */
  int64_t tile_runs;               /* tile runs that did work */
  double kernel_ms, total_ms;
} smp_field_info;                  /* may be NULL */
int smp_base_cost_field(smp_planner* p, const smp_base_lattice* lat, const uint32_t* free_bits,
                        const int32_t source[3], double* cost, int32_t* parent, smp_field_info* info);
int smp_base_route_gpu(smp_planner* p, const smp_base_lattice* lat, const uint32_t* free_bits, const double from[3],
                       const double to[3], int snap_cells, double** out_rows, int64_t* n_out, int32_t** out_chain,
                       smp_route_info* info, smp_field_info* finfo);
/* The field's tile: FIELD_BX x FIELD_BY x FIELD_BT nodes into tile[3] (host only; what the tests size their maps by). */
void smp_field_tile_shape(int tile[3]);

/* smp_plan_far: the staged call.
 *  1. The lattice smp_base_lattice_fit(q->env_x, q->env_y, pitch, n_theta, 0, arm) and its free map at the margin
 *     {map_margin, 0}.  An unconfined query (env_x or env_y of (0, 0)): SMP_ERR_ARG.
 *  2. smp_base_route from q->start[0..2] to q->goal[0..2]; with route_device = 1 smp_base_route_gpu, whose answer is
 *     the same (every output of the call but its times is).
 *  3. Handover: with the chain c_0 .. c_m, acc = 0 and j = m; while j > 0 and acc < handover_distance, the planar length
 *     of the step c_j -> c_j-1 (pitch, the diagonal weight, or 0 for a heading step) is added to acc and j decremented
 *     (squirrel_8dof_planner.cpp:1209-1215).  j == 0: no base stage, the call is smp_plan(p, q, out), n_route_rows = 0.
 *  4. The route rows -- q->start, then the merged rows of the chain c_0 .. c_j -- validated and shortened in one
 *     smp_shortcut_path_margin call with the query's check_self / check_map, the margin {map_margin, 0} and `window`
 *     (the first edge folds the arm if the caller has not).  Blocked: SMP_ERR_NO_SOLUTION, stage 3, check.first_blocked.
 *  5. smp_plan on q with start replaced by the last row of step 4's output, bit for bit.  out is that call's result with
 *     its waypoints prefixed by step 4's rows (the plan's own first row, equal to the last route row, dropped); stats
 *     and cost_rows are the tail's.  A failing tail returns its status with stage 4; out->waypoints then holds the route
 *     rows alone. */
typedef struct smp_far_opts {
  double pitch; int n_theta; double arm[5];
  double handover_distance;   /* distance_birrt_star_planning: metres of base route left to the 8-DoF planner */
  double map_margin;          /* astar_safety_distance's role: margin of the free map and of the route's dense check; 0: boolean */
  int window;                 /* smp_shortcut_path's window over the route rows; <= 0: all pairs */
  int snap_cells;
  int route_device;           /* 0: step 2 on the host (smp_base_route); 1: on the device (smp_base_route_gpu) */
} smp_far_opts;
void smp_far_opts_default(smp_far_opts*);
    /* pitch 0.1, n_theta 8, arm = pose_folded_arm, handover 2.0, margin 0, window 0, snap 2, route on the host */
typedef struct smp_far_info {
  int stage;                  /* where the call ended: 0 complete, 1 free map, 2 route search, 3 route check, 4 tail plan */
  smp_base_map_info map; smp_route_info route; int32_t handover_node[3];
  int64_t n_route_rows;       /* leading rows of out->waypoints that belong to the base stage; 0: planned directly */
  smp_shortcut_info check;    /* the route's dense check */
  double route_ms, total_ms;  /* host clock */
} smp_far_info;
int smp_plan_far(smp_planner* p, const smp_query* q, const smp_far_opts* o, smp_result* out, smp_far_info* info);

/* n poses of `dim` values, row-major.  *n_out = rows of the normalized trajectory; with out == NULL only counts,
 * else writes them (SMP_ERR_CAPACITY if out_cap < *n_out).  For dim < 1 or n <= 1 the reference leaves its output
 * untouched: *n_out = 0.  Host only (no GPU needed). */
int smp_normalize_trajectory(const double* raw, int64_t n, int dim, const double* normalized_pose, double* out,
                             int64_t out_cap, int64_t* n_out);

/* End-effector goal -> 8-DoF pose (IK of the node's goal search). */
typedef struct smp_ik_request {
  double ee_pose[6];        /* x, y, z, roll, pitch, yaw: getFullPoseFromEEPose's endEffectorPose (birrt_star.cpp:1627) */
  double deviation[6][2];   /* (lower, upper) permitted error per task coordinate: endEffectorDeviations
                               (setVariableConstraints, control_laws.cpp:1740-1761) */
  double q_init[8];         /* poseInit (setStartConf, control_laws.cpp:1464-1495) */
  int max_iter;             /* controller iterations, >= 1 (the reference passes 1000, birrt_star.cpp:1670) */
} smp_ik_request;

typedef struct smp_ik_result {
  int reached;              /* 1: REACHED -- getFullPoseFromEEPose returns true; 0: ADVANCED (control_laws.cpp:3691-3710) */
  int iterations;           /* controller iterations run */
  int fallback_iterations;  /* iterations whose manipulability needed the Jacobi eigenvalue path (near-singular J) */
  double q[8];              /* poseSolution = joint_trajectory.back() (birrt_star.cpp:1675) */
  double error[6];          /* last task-space error (zero inside the deviation band) */
  double manipulability;    /* last manipulability measure (control_laws.cpp:6050-6089) */
} smp_ik_result;

/* Parity: bit for bit against the oracle (oracle/smp_oracle.cpp), which is unpinned against the reference here:
 * the reference's manipulability (float Eigen::JacobiSVD, CL:6061-6084) and damped pseudo-inverse (fp64 SVD,
 * CL:5574-5596) are restated as det / Gauss-Jordan with a Jacobi eigen-decomposition fallback (DESIGN.md "IK goal
 * search"), equal in exact arithmetic; near singular Jacobians the iteration counts and REACHED / ADVANCED can
 * differ from the reference binaries.  fallback_iterations counts the fallback branch; tests/test_gpu_ik.py checks
 * that kernel and oracle take the same branch on singular starts. */
int smp_ik_solve(smp_planner* p, const smp_ik_request* reqs, int n, smp_ik_result* out);

typedef struct smp_goal_search {
  int n_candidates;         /* base angles of the search (17 at the default 20 degrees) */
  int n_reached;            /* candidates whose controller run REACHED the pose; candidates after the chosen one may
                               have stopped early (they can no longer be chosen), so this counts the ones that ran */
  int chosen;               /* candidate index of pose_goal, -1 if none */
  int downward;             /* 1 if the hand points downward (squirrel_8dof_planner.cpp:1140) */
  double kernel_ms;         /* IK + validity kernels, HIP events */
} smp_goal_search;

/* findGoalPose for end-effector pose ee_pose (x, y, z, roll, pitch, yaw in the planning frame) from the robot's
 * current pose, candidate spacing in degrees (goal_pose_search_discretization, default 20; values < 1 count as 1).
 * *result: 0 = pose found (pose_goal written), 1 = every pose the controller reached collides (COLLISION_GOAL_POSE),
 * 2 = the controller reached no pose (INVALID_END_EFFECTOR_POSE) -- the reference's return codes.  info may be NULL. */
/* (Unpinned against the reference near singular Jacobians as smp_ik_solve.) */
int smp_find_goal_pose(smp_planner* p, const double ee_pose[6], const double pose_current[8], double discretization_deg,
                       int check_self, int check_map, double pose_goal[8], int* result, smp_goal_search* info);

/* Kernel timing of the last smp_check_configs / smp_plan call: milliseconds on the launch stream. */
int smp_last_kernel_ms(const smp_planner* p, double* check_ms, double* plan_ms, int64_t* plan_launches);

const char* smp_strerror(int status);

#ifdef __cplusplus
}
#endif
#endif /* SMP_GPU_H */
