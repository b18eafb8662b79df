// C ABI implementation (include/smp_gpu.h): status strings and defaults, robot / scene / planner lifecycle, the scene
// setters, the configuration checks and IK.  Planning is smp_api_plan.cpp, the dense edge checks, shortcutting and
// repair smp_api_paths.cpp, the test hooks smp_api_probe.cpp; smp_planner.h holds the handles they share.
// No CPU fallback: without a usable GPU every compute entry point returns SMP_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "smp_attach.h"
#include "smp_kernels.h"
#include "smp_math.h"
#include "smp_planner.h"
#include "smp_scene.h"

namespace smp {
size_t ik_kernels_private_bytes();
void launch_ik(bool search, int n, hipStream_t st, const RobotDev* rb, const IkTaskDev* tasks, IkOutDev* out,
               SceneDev sc, const MapCfg* mc, int self, int map, int* best);
}  // namespace smp

using namespace smp;

static int update_mapcfg(smp_planner* p) {
  const RobotDev& d = p->robot.dev;
  std::memset(&p->mc_host, 0, sizeof(MapCfg));
  p->mc_host.has_map = p->have_scene ? 1 : 0;
  for (int s = 0; s < d.n_sph; ++s) {
    p->mc_host.T[s] = p->have_scene ? sphere_threshold(d.sph_r[s], p->scene_res) : 0;
    int link = d.cl_link[d.sph_clink[s]];
    p->mc_host.map_on[s] = p->disabled.count(p->robot.link_names[link]) ? 0 : 1;
  }
  for (int k = 0; k < d.n_prim; ++k) {
    p->mc_host.pT[k] = p->have_scene ? sphere_threshold(d.prim_rxy[k], p->scene_res) : 0;
    p->mc_host.p_map_on[k] = p->disabled.count(p->robot.link_names[d.cl_link[d.prim_clink[k]]]) ? 0 : 1;
  }
  HIPCHK(hipMemcpyAsync(p->d_mc, &p->mc_host, sizeof(MapCfg), hipMemcpyHostToDevice, p->stream));
  HIPCHK(hipStreamSynchronize(p->stream));
  return SMP_OK;
}

// The self filter's link selection as a mask over the robot's collision links (n = 0: all of them); SMP_ERR_ARG for a
// link that is unknown or has no collision geometry.
static int carve_link_mask(const RobotHost& h, const char* const* links, int n, uint32_t* mask) {
  if (n < 0 || (n > 0 && !links)) return SMP_ERR_ARG;
  if (n == 0) {
    *mask = (uint32_t)((1ull << h.dev.n_clink) - 1ull);
    return SMP_OK;
  }
  uint32_t m = 0;
  for (int i = 0; i < n; ++i) {
    if (!links[i]) return SMP_ERR_ARG;
    int c = -1;
    for (size_t l = 0; l < h.link_names.size(); ++l)
      if (h.link_names[l] == links[i]) c = h.clink_of_link[l];
    if (c < 0) return SMP_ERR_ARG;
    m |= 1u << c;
  }
  *mask = m;
  return SMP_OK;
}

static bool carve_values_ok(const smp_carve* c) {
  for (int j = 0; j < NJ; ++j)
    if (!std::isfinite(c->q[j])) return false;
  return std::isfinite(c->pad) && c->pad >= 0.0;
}

// Scratch and events of the carve launches, created on first use.
static hipError_t carve_scratch(smp_planner* p) {
  hipError_t e;
  if ((e = p->d_citems.reserve(1)) != hipSuccess || (e = p->d_ccount.reserve(1)) != hipSuccess) return e;
  if (!p->ev2 && (e = hipEventCreate(&p->ev2)) != hipSuccess) return e;
  if (!p->ev3 && (e = hipEventCreate(&p->ev3)) != hipSuccess) return e;
  return hipSuccess;
}

static void self_flat_override(RobotDev* d) {
  if (const char* e = std::getenv("SMP_SELF_FLAT"))
    if (std::atoi(e) != 0) d->sr_ok = 0;
}

extern "C" {

void smp_params_default(smp_params* p) {
  p->near_threshold = 4.0;
  p->step_factor = 0.5;
  p->num_traj_segments = 20;
  p->max_near_nodes = 20;
  p->path_optimality_threshold = 1.0;
  p->tree_optimization = 1;
  p->informed_sampling = 1;
  p->node_capacity = 0;
  p->helpers = 0;
  p->scout = 1;
}

void smp_scene_opts_default(smp_scene_opts* o) {
  o->resolution = 0.05;
  o->z_offset = -0.02;
  o->insert_floor = 0;
  o->floor_center[0] = o->floor_center[1] = 0.0;
  o->floor_distance = 3.0;
}

const char* smp_strerror(int s) {
  switch (s) {
    case SMP_OK: return "ok";
    case SMP_ERR_ARG: return "invalid argument";
    case SMP_ERR_START_INVALID: return "start configuration is invalid";
    case SMP_ERR_GOAL_INVALID: return "goal configuration is invalid";
    case SMP_ERR_NO_SOLUTION: return "no solution found within the budget";
    case SMP_ERR_HIP: return "HIP runtime error";
    case SMP_ERR_PARSE: return "parse error";
    case SMP_ERR_CAPACITY: return "tree capacity exceeded";
    case SMP_ERR_NO_DEVICE: return "no usable GPU (the library has no CPU fallback)";
    default: return "unknown status";
  }
}

int smp_robot_create_json(const char* model_json, smp_robot** out) {
  if (!model_json || !out) return SMP_ERR_ARG;
  smp_robot* r = new smp_robot();
  try {
    robot_from_json(model_json, &r->h);
  } catch (const std::exception& e) {
    fprintf(stderr, "smp_gpu: %s\n", e.what());
    delete r;
    return SMP_ERR_PARSE;
  }
  *out = r;
  return SMP_OK;
}

int smp_robot_create_urdf(const char* urdf_xml, const char* srdf_xml, const char* spheres_json, smp_robot** out) {
  if (!urdf_xml || !srdf_xml || !spheres_json || !out) return SMP_ERR_ARG;
  smp_robot* r = new smp_robot();
  try {
    robot_from_urdf(urdf_xml, srdf_xml, spheres_json, &r->h);
  } catch (const std::exception& e) {
    fprintf(stderr, "smp_gpu: %s\n", e.what());
    delete r;
    return SMP_ERR_PARSE;
  }
  *out = r;
  return SMP_OK;
}

int smp_robot_attach(const smp_robot* base, const smp_attach* a, smp_robot** out) {
  if (!base || !a || !out) return SMP_ERR_ARG;
  smp_robot* r = new smp_robot();
  const int st = robot_attach(base->h, *a, &r->h);
  if (st != SMP_OK) {
    delete r;
    return st;
  }
  *out = r;
  return SMP_OK;
}

void smp_robot_destroy(smp_robot* r) { delete r; }
int smp_robot_num_links(const smp_robot* r) { return r ? (int)r->h.link_names.size() : 0; }
const char* smp_robot_link_name(const smp_robot* r, int i) {
  if (!r || i < 0 || i >= (int)r->h.link_names.size()) return nullptr;
  return r->h.link_names[i].c_str();
}
int smp_robot_self_rounds(const smp_robot* r, int32_t info[8], uint16_t* sp_ab, double* sp_rr2, uint16_t* pp_ps,
                          int32_t* partner, double* rr2, uint32_t* prim_mask) {
  if (!r || !info) return SMP_ERR_ARG;
  const RobotDev& d = r->h.dev;
  const int32_t v[8] = {d.n_sph, d.n_prim, d.n_spairs, d.n_ppairs, d.sr_ok, d.sr_rounds, SR_LANES, MAX_SROUNDS};
  std::memcpy(info, v, sizeof(v));
  if (sp_ab) std::memcpy(sp_ab, d.sp_ab, d.n_spairs * sizeof(uint16_t));
  if (sp_rr2) std::memcpy(sp_rr2, d.sp_rr2, d.n_spairs * sizeof(double));
  if (pp_ps) std::memcpy(pp_ps, d.pp_ps, d.n_ppairs * sizeof(uint16_t));
  for (int l = 0; l < SR_LANES; ++l)
    for (int k = 0; k < MAX_SROUNDS; ++k) {
      // (an empty slot holds the lane itself; the threshold is what the tile forms: the two radii's sum, squared)
      const int o = d.sr_partner[l][k];
      const bool used = d.sr_ok && o != l;
      volatile double rs = used ? d.sph_r[l] + d.sph_r[o] : 0.0;
      if (partner) partner[l * MAX_SROUNDS + k] = used ? o : -1;
      if (rr2) rr2[l * MAX_SROUNDS + k] = used ? rs * rs : -1.0;
    }
  if (prim_mask)
    for (int s = 0; s < d.n_sph; ++s) prim_mask[s] = d.sph_pmask[s];
  return SMP_OK;
}

int smp_scene_from_keys(const uint16_t* keys, int64_t n, const smp_scene_opts* o, smp_scene** out) {
  if (!o || !out || (n > 0 && !keys) || !(o->resolution > 0)) return SMP_ERR_ARG;
  std::vector<uint16_t> k(keys, keys + 3 * std::max<int64_t>(n, 0));
  if (o->insert_floor) floor_keys(o->floor_center[0], o->floor_center[1], o->resolution, o->floor_distance, &k);
  smp_scene* s = new smp_scene();
  scene_from_keys(k.data(), (int64_t)k.size() / 3, o->resolution, o->z_offset, &s->h);
  *out = s;
  return SMP_OK;
}

// Occupied keys + free leaves of an octomap stream -> scene (with the node's floor insertion when asked).
static int scene_from_octomap(bool full, bool header, const uint8_t* data, size_t size, double res,
                              const smp_scene_opts* o, smp_scene** out) {
  std::vector<uint16_t> k;
  std::vector<FreeLeaf> fl;
  try {
    if (full) octomap_ot_keys(data, size, &res, &k, &fl, header);
    else octomap_bt_keys(data, size, &res, &k, &fl, header);
  } catch (const std::exception& e) {
    fprintf(stderr, "smp_gpu: %s\n", e.what());
    return SMP_ERR_PARSE;
  }
  if (!(res > 0)) return SMP_ERR_ARG;
  if (o->insert_floor) floor_keys(o->floor_center[0], o->floor_center[1], res, o->floor_distance, &k, &fl);
  smp_scene* s = new smp_scene();
  scene_from_keys(k.data(), (int64_t)k.size() / 3, res, o->z_offset, &s->h);
  *out = s;
  return SMP_OK;
}

int smp_scene_from_bt(const uint8_t* data, size_t size, const smp_scene_opts* o, smp_scene** out) {
  if (!data || !o || !out) return SMP_ERR_ARG;
  return scene_from_octomap(false, true, data, size, 0.0, o, out);
}

int smp_scene_from_ot(const uint8_t* data, size_t size, const smp_scene_opts* o, smp_scene** out) {
  if (!data || !o || !out) return SMP_ERR_ARG;
  return scene_from_octomap(true, true, data, size, 0.0, o, out);
}

int smp_scene_from_octomap_msg(const char* id, double resolution, int binary, const uint8_t* data, size_t size,
                               const smp_scene_opts* o, smp_scene** out) {
  if (!id || !o || !out || (size > 0 && !data) || !(resolution > 0)) return SMP_ERR_ARG;
  // binaryMsgToMap / fullMsgToMap + dynamic_cast<octomap::OcTree*> (squirrel_8dof_planner.cpp:875-883): any
  // other tree type is an empty octomap for the node
  if (std::strcmp(id, "OcTree") != 0) return SMP_ERR_PARSE;
  return scene_from_octomap(binary == 0, false, data, size, resolution, o, out);
}

int smp_scene_from_grid(const uint64_t* bits, const uint16_t* d2, const int dims[3], const double origin[3],
                        double res, smp_scene** out) {
  if (!bits || !d2 || !dims || !origin || !out || !(res > 0) || dims[0] <= 0 || dims[1] <= 0 || dims[2] <= 0)
    return SMP_ERR_ARG;
  smp_scene* s = new smp_scene();
  SceneHost& h = s->h;
  h.nx = dims[0]; h.ny = dims[1]; h.nz = dims[2]; h.wx = (h.nx + 63) / 64;
  h.ox = origin[0]; h.oy = origin[1]; h.oz = origin[2]; h.res = res;
  size_t nw = (size_t)h.wx * h.ny * h.nz, nc = (size_t)h.nx * h.ny * h.nz;
  h.bits.assign(bits, bits + nw);
  h.d2.assign(d2, d2 + nc);
  h.n_occupied = 0;
  for (uint64_t w : h.bits) h.n_occupied += __builtin_popcountll(w);
  build_bricks(&h);
  *out = s;
  return SMP_OK;
}

void smp_scene_destroy(smp_scene* s) { delete s; }

int smp_scene_info(const smp_scene* s, int dims[3], double origin[3], double* resolution, int64_t* n_occupied,
                   double bbox_min[3], double bbox_max[3]) {
  if (!s) return SMP_ERR_ARG;
  if (dims) { dims[0] = s->h.nx; dims[1] = s->h.ny; dims[2] = s->h.nz; }
  if (origin) { origin[0] = s->h.ox; origin[1] = s->h.oy; origin[2] = s->h.oz; }
  if (resolution) *resolution = s->h.res;
  if (n_occupied) *n_occupied = s->h.n_occupied;
  for (int d = 0; d < 3; ++d) {
    if (bbox_min) bbox_min[d] = s->h.bbox_min[d];
    if (bbox_max) bbox_max[d] = s->h.bbox_max[d];
  }
  return SMP_OK;
}

int smp_scene_export(const smp_scene* s, uint64_t* bits, uint16_t* d2) {
  if (!s) return SMP_ERR_ARG;
  if (bits) std::memcpy(bits, s->h.bits.data(), s->h.bits.size() * sizeof(uint64_t));
  if (d2) std::memcpy(d2, s->h.d2.data(), s->h.d2.size() * sizeof(uint16_t));
  return SMP_OK;
}

static bool params_ok(const smp_params& q) {
  return q.max_near_nodes >= 1 && q.max_near_nodes <= 20 && q.num_traj_segments >= 1 && q.num_traj_segments <= MAX_PTS &&
         q.near_threshold > 0 && q.step_factor > 0 && q.node_capacity >= 0 && q.scout >= 0 && q.scout <= MAX_SCOUTS;
}

int smp_planner_set_params(smp_planner* p, const smp_params* params) {
  if (!p || !params || !params_ok(*params)) return SMP_ERR_ARG;
  p->params = *params;
  return SMP_OK;
}

int smp_planner_get_params(const smp_planner* p, smp_params* params) {
  if (!p || !params) return SMP_ERR_ARG;
  *params = p->params;
  return SMP_OK;
}

int smp_planner_create(int device, const smp_robot* robot, const smp_params* params, smp_planner** out) {
  if (!robot || !out) return SMP_ERR_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return SMP_ERR_NO_DEVICE;
  HIPCHK(hipSetDevice(device));
  smp_planner* p = new smp_planner();
  p->device = device;
  p->robot = robot->h;
  if (params) p->params = *params; else smp_params_default(&p->params);
  if (!params_ok(p->params)) {
    delete p;
    return SMP_ERR_ARG;
  }
  // The runtime sizes a dispatch's scratch from the device stack limit (hipLimitStackSize, 1 KB per work-item by
  // default), not from the kernel's private segment: a kernel whose fixed private segment exceeds the limit reads
  // and writes scratch beyond its allocation (HSA_STATUS_ERROR_MEMORY_APERTURE_VIOLATION).  Raise the limit to the
  // largest private segment of the planner's kernels.
  {
    size_t need = 0;
    hipFuncAttributes fa;
    const void* ks[] = {reinterpret_cast<const void*>(&plan_kernel), reinterpret_cast<const void*>(&path_kernel)};
    for (const void* k : ks)
      if (hipFuncGetAttributes(&fa, k) == hipSuccess) need = std::max(need, (size_t)fa.localSizeBytes);
    need = std::max(need, check_kernels_private_bytes());
    need = std::max(need, ik_kernels_private_bytes());
    need = std::max(need, scene_kernels_private_bytes());
    need = std::max(need, edges_kernels_private_bytes());
    need = std::max(need, repair_kernels_private_bytes());
    need = std::max(need, clearance_kernels_private_bytes());
    need = std::max(need, margin_kernels_private_bytes());
    need = std::max(need, carve_kernels_private_bytes());
    need = std::max(need, lattice_kernels_private_bytes());
    need = std::max(need, field_kernels_private_bytes());
    size_t cur = 0;
    if (hipDeviceGetLimit(&cur, hipLimitStackSize) == hipSuccess && cur < need) {
      need = (need + 255) / 256 * 256;
      if (hipDeviceSetLimit(hipLimitStackSize, need) != hipSuccess) {
        delete p;
        return SMP_ERR_HIP;
      }
    }
  }
  // SMP_SELF_FLAT: the job tiles of this planner run the flat self-pair lists, as for a model that does not qualify
  // for the rounds (experiments, and the parity test of the two forms); the planner's copy of the model only
  self_flat_override(&p->robot.dev);
  // every failure from here on releases what was created so far (smp_planner_destroy skips null handles)
  if (hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking) != hipSuccess ||
      hipMalloc(&p->d_rb, sizeof(RobotDev)) != hipSuccess || hipMalloc(&p->d_mc, sizeof(MapCfg)) != hipSuccess ||
      hipMemcpy(p->d_rb, &p->robot.dev, sizeof(RobotDev), hipMemcpyHostToDevice) != hipSuccess ||
      hipEventCreate(&p->ev0) != hipSuccess || hipEventCreate(&p->ev1) != hipSuccess) {
    smp_planner_destroy(p);
    return SMP_ERR_HIP;
  }
  int khz = 0;
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) == hipSuccess && khz > 0)
    p->wall_rate_hz = khz * 1000.0;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
    p->num_cus = cus;
  if (const char* e = std::getenv("SMP_SLOT_SHARE")) p->proc_share = std::max(1, std::atoi(e));
  p->slot_share = p->proc_share;
  int xcc = 0;
  if (hipDeviceGetAttribute(&xcc, hipDeviceAttributeNumberOfXccs, device) == hipSuccess && xcc > 0) p->num_xcd = xcc;
  else (void)hipGetLastError();
  std::memset(&p->sc, 0, sizeof(p->sc));
  int st = update_mapcfg(p);
  if (st) { smp_planner_destroy(p); return st; }
  *out = p;
  return SMP_OK;
}

void smp_planner_destroy(smp_planner* p) {
  if (!p) return;
  (void)hipSetDevice(p->device);
  if (busy_check(p) != SMP_OK) {  // a kernel still runs on the buffers: leak them rather than free them under it
    fprintf(stderr, "smp_gpu: planner destroyed while a planning launch still runs; its device memory is leaked\n");
    return;
  }
  if (p->stream) (void)hipStreamSynchronize(p->stream);
  for (auto& q : p->qb) q.release();
  p->d_qdev.release(); p->d_counts.release(); p->d_lfin.release(); p->d_cq.release(); p->d_valid.release();
  p->d_ik_tasks.release(); p->d_ik_out.release(); p->d_ik_best.release(); p->d_path_edges.release();
  p->d_edges.release(); p->d_eorder.release(); p->d_efirst.release(); p->d_ecounter.release();
  p->d_gaps.release(); p->d_detours.release();
  p->d_clq.release(); p->d_clc.release(); p->d_cle.release(); p->d_mclear.release(); p->d_lbits.release();
  p->d_fbits.release(); p->d_fcost.release(); p->d_factive.release(); p->d_fchanged.release(); p->d_fparent.release();
  p->d_fchain.release(); p->d_fstats.release();
  p->d_bricks.release(); p->d_d2.release(); p->d_d2b.release(); p->d_slab.release();
  p->d_keys.release(); p->d_sbits.release(); p->d_sdil.release(); p->d_scount.release(); p->d_sk01.release();
  if (p->d_rb) (void)hipFree(p->d_rb);
  if (p->d_mc) (void)hipFree(p->d_mc);
  if (p->ev0) (void)hipEventDestroy(p->ev0);
  if (p->ev1) (void)hipEventDestroy(p->ev1);
  p->d_citems.release(); p->d_cflags.release(); p->d_ccount.release();
  if (p->ev2) (void)hipEventDestroy(p->ev2);
  if (p->ev3) (void)hipEventDestroy(p->ev3);
  if (p->stream) (void)hipStreamDestroy(p->stream);
  if (p->h_ttff) (void)hipHostFree(p->h_ttff);
  if (p->h_trace) (void)hipHostFree(p->h_trace);
  if (p->h_abort) (void)hipHostFree(p->h_abort);
  if (p->h_st) (void)hipHostFree(p->h_st);
  delete p;
}

// The collision tests treat a sphere or primitive whose centre lies outside the grid as free of the map (centre_cell,
// prim_candidate): exact only while every occupied cell keeps GRID_REACH (+ one cell of rounding margin) from every
// face of the grid, which scene_from_keys' padding guarantees.  Grids from elsewhere (smp_scene_from_grid, a device
// scene) are checked here: false if an occupied cell of the 4x4x4 bricks lies closer to a face.
static bool occupancy_clear_of_faces(const uint64_t* bricks, int nx, int ny, int nz, double res) {
  const int m = (int)std::ceil(GRID_REACH / res) + 1;
  const int bnx = (nx + 3) / 4, bny = (ny + 3) / 4, bnz = (nz + 3) / 4;
  const int lo[3] = {m, m, m}, hi[3] = {nx - 1 - m, ny - 1 - m, nz - 1 - m};
  for (int bk = 0; bk < bnz; ++bk)
    for (int bj = 0; bj < bny; ++bj)
      for (int bi = 0; bi < bnx; ++bi) {
        uint64_t w = bricks[((size_t)bk * bny + bj) * bnx + bi];
        if (!w) continue;
        if (4 * bi >= lo[0] && 4 * bi + 3 <= hi[0] && 4 * bj >= lo[1] && 4 * bj + 3 <= hi[1] && 4 * bk >= lo[2] &&
            4 * bk + 3 <= hi[2])
          continue;
        for (; w; w &= w - 1) {
          const int bit = __builtin_ctzll(w);
          const int c[3] = {4 * bi + (bit & 3), 4 * bj + ((bit >> 2) & 3), 4 * bk + (bit >> 4)};
          for (int d = 0; d < 3; ++d)
            if (c[d] < lo[d] || c[d] > hi[d]) return false;
        }
      }
  return true;
}

int smp_planner_set_scene(smp_planner* p, const smp_scene* s) {
  if (!p || !s) return SMP_ERR_ARG;
  if (int b_ = busy_check(const_cast<smp_planner*>(p))) return b_;
  if (!occupancy_clear_of_faces(s->h.bricks.data(), s->h.nx, s->h.ny, s->h.nz, s->h.res)) {
    fprintf(stderr, "smp_gpu: an occupied cell lies within %.2f m of the grid's faces (pad the grid)\n", GRID_REACH);
    return SMP_ERR_ARG;
  }
  HIPCHK(hipSetDevice(p->device));
  HIPCHK(p->d_bricks.reserve(s->h.bricks.size()));
  HIPCHK(p->d_d2.reserve(s->h.d2.size()));
  HIPCHK(hipMemcpyAsync(p->d_bricks.p, s->h.bricks.data(), s->h.bricks.size() * sizeof(uint64_t), hipMemcpyHostToDevice, p->stream));
  HIPCHK(hipMemcpyAsync(p->d_d2.p, s->h.d2.data(), s->h.d2.size() * sizeof(uint16_t), hipMemcpyHostToDevice, p->stream));
  p->sc.nx = s->h.nx; p->sc.ny = s->h.ny; p->sc.nz = s->h.nz;
  p->sc.bnx = s->h.bnx; p->sc.bny = s->h.bny;
  p->sc.ox = s->h.ox; p->sc.oy = s->h.oy; p->sc.oz = s->h.oz; p->sc.res = s->h.res; p->sc.inv_res = 1.0 / s->h.res;
  p->sc.bricks = p->d_bricks.p;
  p->sc.d2 = p->d_d2.p;
  {
    const RobotDev& d = p->robot.dev;
    for (int k = 0; k < d.n_prim; ++k)
      if (d.prim_rxy[k] > GRID_REACH) {  // the padding would not keep a primitive outside the grid free
        fprintf(stderr, "smp_gpu: primitive reach %.3f m exceeds the grid padding\n", d.prim_rxy[k]);
        return SMP_ERR_ARG;
      }
    for (int k = 0; k < MAX_PRIM; ++k) p->sc.slab[k] = nullptr;
    if (d.n_prim > 0) {
      std::vector<std::vector<uint16_t>> slabs;
      prim_slabs(d, s->h, &slabs);
      const size_t plane = (size_t)s->h.nx * s->h.ny;
      std::vector<uint16_t> all(plane * d.n_prim);
      for (int k = 0; k < d.n_prim; ++k) std::memcpy(all.data() + k * plane, slabs[k].data(), plane * sizeof(uint16_t));
      HIPCHK(p->d_slab.reserve(all.size()));
      HIPCHK(hipMemcpyAsync(p->d_slab.p, all.data(), all.size() * sizeof(uint16_t), hipMemcpyHostToDevice, p->stream));
      HIPCHK(hipStreamSynchronize(p->stream));  // `all` is released on return
      for (int k = 0; k < d.n_prim; ++k) p->sc.slab[k] = p->d_slab.p + k * plane;
    }
  }
  // byte copy of the field when every sphere's threshold is below 255 (SceneDev.d2b)
  uint32_t tmax = 0;
  for (int k = 0; k < p->robot.dev.n_sph; ++k) tmax = std::max(tmax, sphere_threshold(p->robot.dev.sph_r[k], s->h.res));
  p->sc.d2b = nullptr;
  if (tmax < 255) {
    std::vector<uint8_t> b(s->h.d2.size());
    for (size_t i = 0; i < b.size(); ++i) b[i] = (uint8_t)std::min<uint16_t>(s->h.d2[i], 255);
    HIPCHK(p->d_d2b.reserve(b.size()));
    HIPCHK(hipMemcpyAsync(p->d_d2b.p, b.data(), b.size(), hipMemcpyHostToDevice, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));  // b is released on return
    p->sc.d2b = p->d_d2b.p;
  }
  p->have_scene = true;
  p->scene_res = s->h.res;
  return update_mapcfg(p);
}

// The planner's scene built on the device from occupied keys (DESIGN.md "Scene build", smp_scene.hip): the arrays
// scene_from_keys + smp_planner_set_scene derive on the host, bit for bit.  The grid geometry is scene_from_keys' own
// arithmetic on the key list (O(n), and it carries the double rounding of the origin); everything per cell runs in
// kernels on the planner's stream.
static int set_scene_keys_device(smp_planner* p, const uint16_t* keys, int64_t n, double res, double z_offset,
                                 smp_scene_build* info, std::chrono::steady_clock::time_point t0) {
  if (int b_ = busy_check(p)) return b_;
  const RobotDev& d = p->robot.dev;
  for (int k = 0; k < d.n_prim; ++k)
    if (d.prim_rxy[k] > GRID_REACH) {  // the padding would not keep a primitive outside the grid free
      fprintf(stderr, "smp_gpu: primitive reach %.3f m exceeds the grid padding\n", d.prim_rxy[k]);
      return SMP_ERR_ARG;
    }
  // the self filter's links, by name against the robot of this build (before anything of the old scene is touched)
  uint32_t carve_mask = 0;
  if (p->carve_on) {
    std::vector<const char*> names;
    for (const std::string& s : p->carve_links) names.push_back(s.c_str());
    if (carve_link_mask(p->robot, names.data(), (int)names.size(), &carve_mask) != SMP_OK) {
      fprintf(stderr, "smp_gpu: the self filter names a link the planner's robot does not have (smp_planner_set_carve)\n");
      return SMP_ERR_ARG;
    }
  }
  int nx = 1, ny = 1, nz = 1, kmin[3] = {0, 0, 0};
  double org[3] = {0.0, 0.0, 0.0 + z_offset}, bmin[3] = {0, 0, 0}, bmax[3] = {0, 0, 0};
  if (n > 0) {
    int kmax[3] = {-1, -1, -1};
    kmin[0] = kmin[1] = kmin[2] = 1 << 30;
    for (int64_t i = 0; i < n; ++i)
      for (int a = 0; a < 3; ++a) {
        const int k = keys[i * 3 + a];
        kmin[a] = std::min(kmin[a], k);
        kmax[a] = std::max(kmax[a], k);
      }
    const int pad = grid_pad_cells(res);
    for (int a = 0; a < 3; ++a) {
      bmin[a] = (double)(kmin[a] - KEY_OFFSET) * res;
      bmax[a] = (double)(kmax[a] - KEY_OFFSET + 1) * res;
      kmin[a] -= pad;
      kmax[a] += pad;
    }
    nx = kmax[0] - kmin[0] + 1;
    ny = kmax[1] - kmin[1] + 1;
    nz = kmax[2] - kmin[2] + 1;
    org[0] = (double)(kmin[0] - KEY_OFFSET) * res;
    org[1] = (double)(kmin[1] - KEY_OFFSET) * res;
    org[2] = (double)(kmin[2] - KEY_OFFSET) * res + z_offset;
  } else {
    n = 0;
  }
  if (!scene_build_fits(nx, ny, nz, d.n_prim)) {
    fprintf(stderr, "smp_gpu: a %d x %d x %d grid is beyond the device scene build (use smp_planner_set_scene)\n", nx, ny, nz);
    return SMP_ERR_ARG;
  }
  const int bnx = (nx + 3) / 4, bny = (ny + 3) / 4, bnz = (nz + 3) / 4;
  const size_t nc = (size_t)nx * ny * nz, plane = (size_t)nx * ny, words = scene_words(nx, ny, nz, d.n_prim);
  uint32_t tmax = 0;  // byte copy of the field when every sphere's threshold is below 255 (SceneDev.d2b)
  for (int k = 0; k < d.n_sph; ++k) tmax = std::max(tmax, sphere_threshold(d.sph_r[k], res));
  const bool bytes = tmax < 255;
  int k01[2 * MAX_PRIM] = {0};
  {
    int k0[MAX_PRIM], k1[MAX_PRIM];
    prim_slab_layers(d, org[2], res, nz, k0, k1);
    for (int k = 0; k < d.n_prim; ++k) { k01[2 * k] = k0[k]; k01[2 * k + 1] = k1[k]; }
  }
  HIPCHK(hipSetDevice(p->device));
  HIPCHK(p->d_keys.reserve((size_t)n * 3));
  HIPCHK(p->d_sbits.reserve(words));
  HIPCHK(p->d_sdil.reserve(words));
  HIPCHK(p->d_scount.reserve(1));
  HIPCHK(p->d_sk01.reserve(2 * MAX_PRIM));
  HIPCHK(p->d_bricks.reserve((size_t)bnx * bny * bnz));
  HIPCHK(p->d_d2.reserve(nc));
  if (bytes) HIPCHK(p->d_d2b.reserve(nc));
  if (d.n_prim > 0) HIPCHK(p->d_slab.reserve(plane * d.n_prim));
  if (n > 0) HIPCHK(hipMemcpyAsync(p->d_keys.p, keys, (size_t)n * 3 * sizeof(uint16_t), hipMemcpyHostToDevice, p->stream));
  HIPCHK(hipMemcpyAsync(p->d_sk01.p, k01, sizeof(k01), hipMemcpyHostToDevice, p->stream));
  SceneBuildArgs a{};
  a.keys = p->d_keys.p; a.n_keys = n;
  for (int c = 0; c < 3; ++c) a.kmin[c] = kmin[c];
  a.nx = nx; a.ny = ny; a.nz = nz;
  a.bits = p->d_sbits.p; a.dil = p->d_sdil.p; a.count = p->d_scount.p;
  a.bricks = reinterpret_cast<unsigned long long*>(p->d_bricks.p);
  a.d2 = p->d_d2.p;
  a.d2b = bytes ? p->d_d2b.p : nullptr;
  a.n_prim = d.n_prim; a.k01 = p->d_sk01.p; a.slab = p->d_slab.p;
  CarveArgs ca{};
  const bool carving = p->carve_on && n > 0;
  if (carving) {
    HIPCHK(carve_scratch(p));
    ca.rb = p->d_rb;
    for (int j = 0; j < NJ; ++j) ca.q[j] = p->carve_q[j];
    ca.pad = p->carve_pad;
    ca.links = carve_mask;
    ca.items = p->d_citems.p;
    ca.keys = p->d_keys.p; ca.n_keys = n;
    for (int c = 0; c < 3; ++c) { ca.kmin[c] = kmin[c]; ca.org[c] = org[c]; }
    ca.res = res;
    ca.flags = nullptr;
    ca.bits = p->d_sbits.p;
    ca.nx = nx; ca.ny = ny; ca.nz = nz;
    ca.count = p->d_ccount.p;
    a.carve = &ca;
    a.carve_ev[0] = p->ev2; a.carve_ev[1] = p->ev3;
  }
  HIPCHK(hipEventRecord(p->ev0, p->stream));
  HIPCHK(launch_scene_build(p->stream, a));
  HIPCHK(hipEventRecord(p->ev1, p->stream));
  unsigned long long n_occ = 0, n_carved = 0;
  HIPCHK(hipMemcpyAsync(&n_occ, p->d_scount.p, sizeof(n_occ), hipMemcpyDeviceToHost, p->stream));
  if (carving) HIPCHK(hipMemcpyAsync(&n_carved, p->d_ccount.p, sizeof(n_carved), hipMemcpyDeviceToHost, p->stream));
  p->sc.nx = nx; p->sc.ny = ny; p->sc.nz = nz;
  p->sc.bnx = bnx; p->sc.bny = bny;
  p->sc.ox = org[0]; p->sc.oy = org[1]; p->sc.oz = org[2]; p->sc.res = res; p->sc.inv_res = 1.0 / res;
  p->sc.bricks = p->d_bricks.p;
  p->sc.d2 = p->d_d2.p;
  p->sc.d2b = bytes ? p->d_d2b.p : nullptr;
  for (int k = 0; k < MAX_PRIM; ++k) p->sc.slab[k] = k < d.n_prim ? p->d_slab.p + k * plane : nullptr;
  p->have_scene = true;
  p->scene_res = res;
  // The one synchronisation of this path: update_mapcfg waits for the stream after its own small upload, which
  // covers the kernels (kernel_ms, the occupied-cell count) and the key upload (the caller's buffer, k01).
  if (int st = update_mapcfg(p)) return st;
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, p->ev0, p->ev1));
  if (p->carve_on) {
    float cms = 0.f;
    if (carving) HIPCHK(hipEventElapsedTime(&cms, p->ev2, p->ev3));
    p->last_carve.n_carved = (int64_t)n_carved;
    p->last_carve.kernel_ms = cms;
    p->last_carve.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  if (info) {
    info->dims[0] = nx; info->dims[1] = ny; info->dims[2] = nz;
    for (int c = 0; c < 3; ++c) { info->origin[c] = org[c]; info->bbox_min[c] = bmin[c]; info->bbox_max[c] = bmax[c]; }
    info->resolution = res;
    info->n_occupied = (int64_t)n_occ;
    info->kernel_ms = ms;
    info->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  return SMP_OK;
}

int smp_planner_set_scene_keys(smp_planner* p, const uint16_t* keys, int64_t n, const smp_scene_opts* o,
                               smp_scene_build* info) {
  const auto t0 = std::chrono::steady_clock::now();
  if (!p || !o || (n > 0 && !keys) || !(o->resolution > 0)) return SMP_ERR_ARG;
  if (!o->insert_floor) return set_scene_keys_device(p, keys, n, o->resolution, o->z_offset, info, t0);
  std::vector<uint16_t> k(keys, keys + 3 * std::max<int64_t>(n, 0));
  floor_keys(o->floor_center[0], o->floor_center[1], o->resolution, o->floor_distance, &k);
  return set_scene_keys_device(p, k.data(), (int64_t)k.size() / 3, o->resolution, o->z_offset, info, t0);
}

int smp_planner_set_carve(smp_planner* p, const smp_carve* c) {
  if (!p) return SMP_ERR_ARG;
  if (int b_ = busy_check(p)) return b_;
  if (!c) {
    p->carve_on = false;
    p->carve_links.clear();
    return SMP_OK;
  }
  uint32_t mask = 0;
  if (!carve_values_ok(c) || carve_link_mask(p->robot, c->links, c->n_links, &mask) != SMP_OK) return SMP_ERR_ARG;
  p->carve_on = true;
  for (int j = 0; j < NJ; ++j) p->carve_q[j] = c->q[j];
  p->carve_pad = c->pad;
  p->carve_links.clear();
  for (int i = 0; i < c->n_links; ++i) p->carve_links.push_back(c->links[i]);
  return SMP_OK;
}

int smp_planner_last_carve(const smp_planner* p, smp_carve_info* info) {
  if (!p || !info) return SMP_ERR_ARG;
  *info = p->last_carve;
  return SMP_OK;
}

// The self filter as a mask over the caller's keys.  The grid geometry is set_scene_keys_device's own arithmetic on the
// list after floor insertion; the planner's scene is not touched (the keys share the build's upload buffer, which holds
// nothing between builds).
int smp_carve_keys(smp_planner* p, const uint16_t* keys, int64_t n, const smp_scene_opts* o, const smp_carve* c,
                   uint8_t* carved, smp_carve_info* info) {
  const auto t0 = std::chrono::steady_clock::now();
  if (!p || !o || !c || n < 0 || (n > 0 && (!keys || !carved)) || !(o->resolution > 0)) return SMP_ERR_ARG;
  if (int b_ = busy_check(p)) return b_;
  uint32_t mask = 0;
  if (!carve_values_ok(c) || carve_link_mask(p->robot, c->links, c->n_links, &mask) != SMP_OK) return SMP_ERR_ARG;
  p->last_carve = smp_carve_info{0, 0.0, 0.0};
  if (info) *info = p->last_carve;
  if (n == 0) return SMP_OK;
  const double res = o->resolution;
  std::vector<uint16_t> fk;
  if (o->insert_floor) floor_keys(o->floor_center[0], o->floor_center[1], res, o->floor_distance, &fk);
  int kmin[3] = {1 << 30, 1 << 30, 1 << 30}, kmax[3] = {-1, -1, -1};
  for (int64_t i = 0; i < n; ++i)
    for (int a = 0; a < 3; ++a) {
      const int k = keys[i * 3 + a];
      kmin[a] = std::min(kmin[a], k);
      kmax[a] = std::max(kmax[a], k);
    }
  for (size_t i = 0; i < fk.size() / 3; ++i)
    for (int a = 0; a < 3; ++a) {
      const int k = fk[i * 3 + a];
      kmin[a] = std::min(kmin[a], k);
      kmax[a] = std::max(kmax[a], k);
    }
  const int pad = grid_pad_cells(res);
  CarveArgs ca{};
  for (int a = 0; a < 3; ++a) {
    kmin[a] -= pad;
    kmax[a] += pad;
    ca.kmin[a] = kmin[a];
  }
  ca.org[0] = (double)(kmin[0] - KEY_OFFSET) * res;
  ca.org[1] = (double)(kmin[1] - KEY_OFFSET) * res;
  ca.org[2] = (double)(kmin[2] - KEY_OFFSET) * res + o->z_offset;
  ca.nx = kmax[0] - kmin[0] + 1; ca.ny = kmax[1] - kmin[1] + 1; ca.nz = kmax[2] - kmin[2] + 1;
  ca.res = res;
  HIPCHK(hipSetDevice(p->device));
  HIPCHK(carve_scratch(p));
  HIPCHK(p->d_keys.reserve((size_t)n * 3));
  HIPCHK(p->d_cflags.reserve((size_t)n));
  HIPCHK(hipMemcpyAsync(p->d_keys.p, keys, (size_t)n * 3 * sizeof(uint16_t), hipMemcpyHostToDevice, p->stream));
  ca.rb = p->d_rb;
  for (int j = 0; j < NJ; ++j) ca.q[j] = c->q[j];
  ca.pad = c->pad;
  ca.links = mask;
  ca.items = p->d_citems.p;
  ca.keys = p->d_keys.p; ca.n_keys = n;
  ca.flags = p->d_cflags.p;
  ca.bits = nullptr;
  ca.count = p->d_ccount.p;
  HIPCHK(hipEventRecord(p->ev2, p->stream));
  HIPCHK(launch_carve(p->stream, ca));
  HIPCHK(hipEventRecord(p->ev3, p->stream));
  unsigned long long n_carved = 0;
  HIPCHK(hipMemcpyAsync(carved, p->d_cflags.p, (size_t)n, hipMemcpyDeviceToHost, p->stream));
  HIPCHK(hipMemcpyAsync(&n_carved, p->d_ccount.p, sizeof(n_carved), hipMemcpyDeviceToHost, p->stream));
  HIPCHK(hipStreamSynchronize(p->stream));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, p->ev2, p->ev3));
  p->last_carve.n_carved = (int64_t)n_carved;
  p->last_carve.kernel_ms = ms;
  p->last_carve.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (info) *info = p->last_carve;
  return SMP_OK;
}

// Occupied keys + free leaves of an octomap stream (the host decoders: the octree walk is sequential and small, and
// the floor rule depends on the free leaves), then the keys path.
static int set_scene_octomap_device(smp_planner* p, bool full, bool header, const uint8_t* data, size_t size,
                                    double res, const smp_scene_opts* o, smp_scene_build* info,
                                    std::chrono::steady_clock::time_point t0) {
  std::vector<uint16_t> k;
  std::vector<FreeLeaf> fl;
  try {
    if (full) octomap_ot_keys(data, size, &res, &k, &fl, header);
    else octomap_bt_keys(data, size, &res, &k, &fl, header);
  } catch (const std::exception& e) {
    fprintf(stderr, "smp_gpu: %s\n", e.what());
    return SMP_ERR_PARSE;
  }
  if (!(res > 0)) return SMP_ERR_ARG;
  if (o->insert_floor) floor_keys(o->floor_center[0], o->floor_center[1], res, o->floor_distance, &k, &fl);
  return set_scene_keys_device(p, k.data(), (int64_t)k.size() / 3, res, o->z_offset, info, t0);
}

int smp_planner_set_scene_bt(smp_planner* p, const uint8_t* data, size_t size, const smp_scene_opts* o,
                             smp_scene_build* info) {
  const auto t0 = std::chrono::steady_clock::now();
  if (!p || !data || !o) return SMP_ERR_ARG;
  return set_scene_octomap_device(p, false, true, data, size, 0.0, o, info, t0);
}

int smp_planner_set_scene_ot(smp_planner* p, const uint8_t* data, size_t size, const smp_scene_opts* o,
                             smp_scene_build* info) {
  const auto t0 = std::chrono::steady_clock::now();
  if (!p || !data || !o) return SMP_ERR_ARG;
  return set_scene_octomap_device(p, true, true, data, size, 0.0, o, info, t0);
}

int smp_planner_set_scene_octomap_msg(smp_planner* p, const char* id, double resolution, int binary,
                                      const uint8_t* data, size_t size, const smp_scene_opts* o,
                                      smp_scene_build* info) {
  const auto t0 = std::chrono::steady_clock::now();
  if (!p || !id || !o || (size > 0 && !data) || !(resolution > 0)) return SMP_ERR_ARG;
  if (std::strcmp(id, "OcTree") != 0) return SMP_ERR_PARSE;  // as smp_scene_from_octomap_msg
  return set_scene_octomap_device(p, binary == 0, false, data, size, resolution, o, info, t0);
}

// Device-resident scene of a planner (multi-GPU): the arrays smp_planner_set_scene derived for
// this robot (bricks, box-gap field, its byte copy, the primitives' slab fields) travel device to device -- an RCCL
// broadcast between ranks, or peer copies over xGMI between the planners of one process -- instead of being rebuilt
// from a host scene on every GPU.
static void scene_layout(const smp_planner* p, smp_scene_device* o) {
  o->dims[0] = p->sc.nx; o->dims[1] = p->sc.ny; o->dims[2] = p->sc.nz;
  o->origin[0] = p->sc.ox; o->origin[1] = p->sc.oy; o->origin[2] = p->sc.oz;
  o->resolution = p->sc.res;
  o->n_bricks = (int64_t)p->sc.bnx * p->sc.bny * (((int64_t)p->sc.nz + 3) / 4);
  o->n_cells = (int64_t)p->sc.nx * p->sc.ny * p->sc.nz;
  o->n_prim = p->robot.dev.n_prim;
  o->has_d2b = p->sc.d2b != nullptr;
}

int smp_planner_scene_device(const smp_planner* p, smp_scene_device* io) {
  if (!p || !io) return SMP_ERR_ARG;
  if (int b_ = busy_check(const_cast<smp_planner*>(p))) return b_;
  if (!p->have_scene) return SMP_ERR_ARG;
  HIPCHK(hipSetDevice(p->device));
  uint64_t* bricks = io->bricks;
  uint16_t* d2 = io->d2;
  uint8_t* d2b = io->d2b;
  uint16_t* slab = io->slab;
  scene_layout(p, io);
  io->bricks = bricks; io->d2 = d2; io->d2b = d2b; io->slab = slab;
  const size_t plane = (size_t)p->sc.nx * p->sc.ny;
  if (bricks) HIPCHK(hipMemcpyAsync(bricks, p->sc.bricks, io->n_bricks * sizeof(uint64_t), hipMemcpyDefault, p->stream));
  if (d2) HIPCHK(hipMemcpyAsync(d2, p->sc.d2, io->n_cells * sizeof(uint16_t), hipMemcpyDefault, p->stream));
  if (d2b && io->has_d2b) HIPCHK(hipMemcpyAsync(d2b, p->sc.d2b, io->n_cells, hipMemcpyDefault, p->stream));
  if (slab && io->n_prim > 0)
    HIPCHK(hipMemcpyAsync(slab, p->d_slab.p, plane * io->n_prim * sizeof(uint16_t), hipMemcpyDefault, p->stream));
  HIPCHK(hipStreamSynchronize(p->stream));
  return SMP_OK;
}

int smp_planner_set_scene_device(smp_planner* p, const smp_scene_device* in) {
  if (!p || !in || !in->bricks || !in->d2) return SMP_ERR_ARG;
  if (int b_ = busy_check(const_cast<smp_planner*>(p))) return b_;
  const int nx = in->dims[0], ny = in->dims[1], nz = in->dims[2];
  if (nx <= 0 || ny <= 0 || nz <= 0 || !(in->resolution > 0)) return SMP_ERR_ARG;
  const RobotDev& d = p->robot.dev;
  const int bnx = (nx + 3) / 4, bny = (ny + 3) / 4, bnz = (nz + 3) / 4;
  const size_t nb = (size_t)bnx * bny * bnz, nc = (size_t)nx * ny * nz, plane = (size_t)nx * ny;
  // the derived arrays depend on the robot (slab z ranges, the byte field's threshold condition): the sender's
  // robot must be this one's
  uint32_t tmax = 0;
  for (int k = 0; k < d.n_sph; ++k) tmax = std::max(tmax, sphere_threshold(d.sph_r[k], in->resolution));
  if (in->n_bricks != (int64_t)nb || in->n_cells != (int64_t)nc || in->n_prim != d.n_prim ||
      (in->has_d2b != 0) != (tmax < 255) || (in->has_d2b && !in->d2b) || (d.n_prim > 0 && !in->slab))
    return SMP_ERR_ARG;
  for (int k = 0; k < d.n_prim; ++k)
    if (d.prim_rxy[k] > GRID_REACH) return SMP_ERR_ARG;
  HIPCHK(hipSetDevice(p->device));
  {  // the occupancy must keep the collision tests' reach from the grid's faces (occupancy_clear_of_faces)
    std::vector<uint64_t> hb(nb);
    HIPCHK(hipMemcpy(hb.data(), in->bricks, nb * sizeof(uint64_t), hipMemcpyDefault));
    if (!occupancy_clear_of_faces(hb.data(), nx, ny, nz, in->resolution)) return SMP_ERR_ARG;
  }
  HIPCHK(p->d_bricks.reserve(nb));
  HIPCHK(p->d_d2.reserve(nc));
  // hipMemcpyDefault: a source on another GPU is a peer copy (xGMI), one on this GPU a device copy
  HIPCHK(hipMemcpyAsync(p->d_bricks.p, in->bricks, nb * sizeof(uint64_t), hipMemcpyDefault, p->stream));
  HIPCHK(hipMemcpyAsync(p->d_d2.p, in->d2, nc * sizeof(uint16_t), hipMemcpyDefault, p->stream));
  p->sc.d2b = nullptr;
  if (in->has_d2b) {
    HIPCHK(p->d_d2b.reserve(nc));
    HIPCHK(hipMemcpyAsync(p->d_d2b.p, in->d2b, nc, hipMemcpyDefault, p->stream));
    p->sc.d2b = p->d_d2b.p;
  }
  for (int k = 0; k < MAX_PRIM; ++k) p->sc.slab[k] = nullptr;
  if (d.n_prim > 0) {
    HIPCHK(p->d_slab.reserve(plane * d.n_prim));
    HIPCHK(hipMemcpyAsync(p->d_slab.p, in->slab, plane * d.n_prim * sizeof(uint16_t), hipMemcpyDefault, p->stream));
    for (int k = 0; k < d.n_prim; ++k) p->sc.slab[k] = p->d_slab.p + k * plane;
  }
  HIPCHK(hipStreamSynchronize(p->stream));  // the caller may release its buffers on return
  p->sc.nx = nx; p->sc.ny = ny; p->sc.nz = nz;
  p->sc.bnx = bnx; p->sc.bny = bny;
  p->sc.ox = in->origin[0]; p->sc.oy = in->origin[1]; p->sc.oz = in->origin[2];
  p->sc.res = in->resolution; p->sc.inv_res = 1.0 / in->resolution;
  p->sc.bricks = p->d_bricks.p;
  p->sc.d2 = p->d_d2.p;
  p->have_scene = true;
  p->scene_res = in->resolution;
  return update_mapcfg(p);
}

int smp_planners_share_scene(smp_planner* const* ps, int n, int src) {
  if (!ps || n <= 0 || src < 0 || src >= n || !ps[src]) return SMP_ERR_ARG;
  smp_scene_device v{};
  int rc = smp_planner_scene_device(ps[src], &v);
  if (rc != SMP_OK) return rc;
  v.bricks = ps[src]->d_bricks.p;
  v.d2 = ps[src]->d_d2.p;
  v.d2b = ps[src]->sc.d2b ? ps[src]->d_d2b.p : nullptr;
  v.slab = v.n_prim > 0 ? ps[src]->d_slab.p : nullptr;
  for (int i = 0; i < n; ++i) {
    if (i == src) continue;
    if (!ps[i]) return SMP_ERR_ARG;
    if (ps[i]->device != ps[src]->device) {
      // direct peer reads over xGMI where the pair allows it (else the runtime stages the copy)
      int can = 0;
      HIPCHK(hipDeviceCanAccessPeer(&can, ps[i]->device, ps[src]->device));
      if (can) {
        HIPCHK(hipSetDevice(ps[i]->device));
        const hipError_t e = hipDeviceEnablePeerAccess(ps[src]->device, 0);
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) HIPCHK(e);
        (void)hipGetLastError();
      }
    }
    rc = smp_planner_set_scene_device(ps[i], &v);
    if (rc != SMP_OK) return rc;
  }
  return SMP_OK;
}

int smp_set_disabled_map_links(smp_planner* p, const char* const* names, int n) {
  if (!p || (n > 0 && !names)) return SMP_ERR_ARG;
  if (int b_ = busy_check(const_cast<smp_planner*>(p))) return b_;
  HIPCHK(hipSetDevice(p->device));
  p->disabled.clear();
  for (int i = 0; i < n; ++i) if (names[i]) p->disabled.insert(names[i]);
  return update_mapcfg(p);
}

// The planner's robot swapped in place (an object attached or detached, smp_robot_attach).  Every kernel reads the
// model from d_rb and the per-sphere map constants from d_mc, so the swap is those two uploads; of the scene only the
// byte field depends on the spheres (it exists while every threshold is below 255), and the slab fields belong to
// the primitives, which therefore may not change under a scene.
int smp_planner_set_robot(smp_planner* p, const smp_robot* r) {
  if (!p || !r) return SMP_ERR_ARG;
  if (int b_ = busy_check(p)) return b_;
  const RobotDev& o = p->robot.dev;
  const RobotDev& d = r->h.dev;
  if (p->have_scene) {
    const bool same = d.n_prim == o.n_prim && !std::memcmp(d.prim_type, o.prim_type, sizeof(o.prim_type)) &&
                      !std::memcmp(d.prim_body, o.prim_body, sizeof(o.prim_body)) &&
                      !std::memcmp(d.prim_cb, o.prim_cb, sizeof(o.prim_cb)) &&
                      !std::memcmp(d.prim_ab, o.prim_ab, sizeof(o.prim_ab)) &&
                      !std::memcmp(d.prim_h, o.prim_h, sizeof(o.prim_h)) &&
                      !std::memcmp(d.prim_rxy, o.prim_rxy, sizeof(o.prim_rxy));
    if (!same) {
      fprintf(stderr, "smp_gpu: the new robot's primitives differ from the scene's slab fields (set the scene again)\n");
      return SMP_ERR_ARG;
    }
  }
  HIPCHK(hipSetDevice(p->device));
  const uint8_t* d2b = p->sc.d2b;
  if (p->have_scene) {
    uint32_t tmax = 0;
    for (int k = 0; k < d.n_sph; ++k) tmax = std::max(tmax, sphere_threshold(d.sph_r[k], p->scene_res));
    if (tmax >= 255) {
      d2b = nullptr;
    } else if (!d2b) {
      const size_t nc = (size_t)p->sc.nx * p->sc.ny * p->sc.nz;
      HIPCHK(p->d_d2b.reserve(nc));
      HIPCHK(launch_scene_bytes(p->stream, p->sc.d2, (long long)nc, p->d_d2b.p));
      d2b = p->d_d2b.p;
    }
  }
  RobotHost nh = r->h;
  self_flat_override(&nh.dev);
  HIPCHK(hipMemcpyAsync(p->d_rb, &nh.dev, sizeof(RobotDev), hipMemcpyHostToDevice, p->stream));
  HIPCHK(hipStreamSynchronize(p->stream));  // nh is pageable host memory and moves below
  p->robot = std::move(nh);
  p->sc.d2b = d2b;
  return update_mapcfg(p);
}

int smp_check_configs(smp_planner* p, const double* q_soa, int64_t n, int check_self, int check_map, uint8_t* valid) {
  if (!p || n < 0 || (n > 0 && (!q_soa || !valid))) return SMP_ERR_ARG;
  if (int b_ = busy_check(const_cast<smp_planner*>(p))) return b_;
  if (n == 0) return SMP_OK;
  HIPCHK(hipSetDevice(p->device));
  HIPCHK(p->d_cq.reserve((size_t)n * NJ));
  HIPCHK(p->d_valid.reserve((size_t)n));
  HIPCHK(hipMemcpyAsync(p->d_cq.p, q_soa, (size_t)n * NJ * sizeof(double), hipMemcpyHostToDevice, p->stream));
  long long tiles = (n + 31) / 32;
  int grid = (int)std::min<long long>(tiles, 256 * 8);
  HIPCHK(hipEventRecord(p->ev0, p->stream));
  launch_check(32, grid, p->stream, p->d_rb, p->sc, p->d_mc, p->d_cq.p, (long long)n, check_self,
               check_map && p->have_scene, p->d_valid.p, nullptr);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(p->ev1, p->stream));
  HIPCHK(hipMemcpyAsync(valid, p->d_valid.p, (size_t)n, hipMemcpyDeviceToHost, p->stream));
  HIPCHK(hipStreamSynchronize(p->stream));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, p->ev0, p->ev1));
  p->last_check_ms = ms;
  return SMP_OK;
}

// getCollisions (birrt_star.cpp:6910-6914 -> collision_checker.hpp:123-132, 594-630): one configuration's
// colliding self pairs (pair order, CC:378-388) and map-colliding links (std::map name order, CC:189, 615).
int smp_get_collisions(smp_planner* p, const double q[8], int32_t* self_pairs, int max_self, int* n_self,
                       int32_t* map_links, int max_map, int* n_map) {
  if (!p || !q || !n_self || !n_map || max_self < 0 || max_map < 0 || (max_self > 0 && !self_pairs) ||
      (max_map > 0 && !map_links))
    return SMP_ERR_ARG;
  if (int b_ = busy_check(const_cast<smp_planner*>(p))) return b_;
  const RobotDev& d = p->robot.dev;
  HIPCHK(hipSetDevice(p->device));
  HIPCHK(p->d_cq.reserve(NJ));
  HIPCHK(p->d_valid.reserve(MAX_CLINK + MAX_PAIRS));
  HIPCHK(hipMemcpyAsync(p->d_cq.p, q, NJ * sizeof(double), hipMemcpyHostToDevice, p->stream));
  launch_collisions(p->stream, p->d_rb, p->sc, p->d_mc, p->d_cq.p, p->have_scene ? 1 : 0, p->d_valid.p,
                    p->d_valid.p + MAX_CLINK);
  HIPCHK(hipGetLastError());
  uint8_t flags[MAX_CLINK + MAX_PAIRS];
  HIPCHK(hipMemcpyAsync(flags, p->d_valid.p, sizeof(flags), hipMemcpyDeviceToHost, p->stream));
  HIPCHK(hipStreamSynchronize(p->stream));
  int ns = 0;
  for (int k = 0; k < d.n_pairs; ++k) {
    if (!flags[MAX_CLINK + k]) continue;
    if (ns < max_self) {
      self_pairs[2 * ns] = d.cl_link[d.pair_a[k]];
      self_pairs[2 * ns + 1] = d.cl_link[d.pair_b[k]];
    }
    ++ns;
  }
  std::vector<int> links;
  for (int c = 0; c < d.n_clink; ++c)
    if (flags[c]) links.push_back(d.cl_link[c]);
  const std::vector<std::string>& names = p->robot.link_names;
  std::sort(links.begin(), links.end(), [&](int a, int b) { return names[a] < names[b]; });
  for (int k = 0; k < (int)links.size() && k < max_map; ++k) map_links[k] = links[k];
  *n_self = ns;
  *n_map = (int)links.size();
  return SMP_OK;
}

int smp_check_sequence(smp_planner* p, const double* q_rows, int64_t n, int check_self, int check_map,
                       int64_t* first_invalid) {
  if (!p || !first_invalid || n < 0 || (n > 0 && !q_rows)) return SMP_ERR_ARG;
  if (int b_ = busy_check(const_cast<smp_planner*>(p))) return b_;
  *first_invalid = -1;
  if (n == 0) return SMP_OK;
  std::vector<double> soa((size_t)n * NJ);
  for (int64_t i = 0; i < n; ++i)
    for (int j = 0; j < NJ; ++j) soa[(size_t)j * n + i] = q_rows[i * NJ + j];
  std::vector<uint8_t> v((size_t)n);
  const int st = smp_check_configs(p, soa.data(), n, check_self, check_map, v.data());
  if (st != SMP_OK) return st;
  for (int64_t i = 0; i < n; ++i)
    if (!v[i]) { *first_invalid = i; break; }
  return SMP_OK;
}

int smp_is_config_valid(smp_planner* p, const double q[8], int check_self, int check_map, int* valid) {
  if (!p || !q || !valid) return SMP_ERR_ARG;
  if (int b_ = busy_check(const_cast<smp_planner*>(p))) return b_;
  double soa[8];
  for (int j = 0; j < 8; ++j) soa[j] = q[j];
  uint8_t v = 0;
  int st = smp_check_configs(p, soa, 1, check_self, check_map, &v);
  *valid = v;
  return st;
}

// IK controller runs (getFullPoseFromEEPose, birrt_star.cpp:1627-1686): one wavefront per task, on p->stream.
// search != 0: the candidates of one findGoalPose -- a run that REACHED checks its pose (isConfigValid,
// birrt_star.cpp:6897-6908) in the same kernel and runs that can no longer be chosen stop early.
static int ik_run(smp_planner* p, const std::vector<IkTaskDev>& tasks, std::vector<IkOutDev>& outs, int search,
                  int check_self, int check_map, double* ms) {
  const int n = (int)tasks.size();
  outs.assign(n, IkOutDev{});
  if (n == 0) return SMP_OK;
  HIPCHK(hipSetDevice(p->device));
  HIPCHK(p->d_ik_tasks.reserve(n));
  HIPCHK(p->d_ik_out.reserve(n));
  HIPCHK(p->d_ik_best.reserve(1));
  HIPCHK(hipMemcpyAsync(p->d_ik_tasks.p, tasks.data(), n * sizeof(IkTaskDev), hipMemcpyHostToDevice, p->stream));
  HIPCHK(hipMemsetAsync(p->d_ik_best.p, 0x7f, sizeof(int), p->stream));
  HIPCHK(hipEventRecord(p->ev0, p->stream));
  launch_ik(search != 0, n, p->stream, p->d_rb, p->d_ik_tasks.p, p->d_ik_out.p, p->sc, p->d_mc, check_self,
            check_map && p->have_scene, p->d_ik_best.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(p->ev1, p->stream));
  HIPCHK(hipMemcpyAsync(outs.data(), p->d_ik_out.p, n * sizeof(IkOutDev), hipMemcpyDeviceToHost, p->stream));
  HIPCHK(hipStreamSynchronize(p->stream));
  float f = 0;
  HIPCHK(hipEventElapsedTime(&f, p->ev0, p->ev1));
  if (ms) *ms = f;
  return SMP_OK;
}

int smp_ik_solve(smp_planner* p, const smp_ik_request* reqs, int n, smp_ik_result* out) {
  if (!p || n < 0 || (n > 0 && (!reqs || !out))) return SMP_ERR_ARG;
  if (int b_ = busy_check(const_cast<smp_planner*>(p))) return b_;
  if (n == 0) return SMP_OK;
  std::vector<IkTaskDev> tasks(n);
  for (int i = 0; i < n; ++i) {
    const smp_ik_request& r = reqs[i];
    if (r.max_iter < 1) return SMP_ERR_ARG;
    IkTaskDev& t = tasks[i];
    std::memset(&t, 0, sizeof(t));
    ik_goal_quat(r.ee_pose, t.goal);
    for (int k = 0; k < 6; ++k) { t.lo[k] = r.deviation[k][0]; t.hi[k] = r.deviation[k][1]; }
    for (int j = 0; j < NJ; ++j) t.q[j] = r.q_init[j];
    t.max_iter = r.max_iter;
  }
  std::vector<IkOutDev> outs;
  double ms = 0;
  const int st = ik_run(p, tasks, outs, 0, 0, 0, &ms);
  if (st != SMP_OK) return st;
  p->last_check_ms = ms;
  for (int i = 0; i < n; ++i) {
    smp_ik_result& o = out[i];
    o.reached = outs[i].reached;
    o.iterations = outs[i].iters;
    o.fallback_iterations = outs[i].fallback;
    for (int j = 0; j < NJ; ++j) o.q[j] = outs[i].q[j];
    for (int k = 0; k < 6; ++k) o.error[k] = outs[i].err[k];
    o.manipulability = outs[i].manip;
  }
  return SMP_OK;
}

int smp_find_goal_pose(smp_planner* p, const double ee_pose[6], const double pose_current[8], double discretization_deg,
                       int check_self, int check_map, double pose_goal[8], int* result, smp_goal_search* info) {
  if (!p || !ee_pose || !pose_current || !pose_goal || !result || !(discretization_deg == discretization_deg))
    return SMP_ERR_ARG;
  if (int b_ = busy_check(const_cast<smp_planner*>(p))) return b_;
  int n = 0;
  ik_goal_candidates(ee_pose, pose_current, discretization_deg, nullptr, 0, &n);
  std::vector<IkTaskDev> tasks(n);
  const int down = ik_goal_candidates(ee_pose, pose_current, discretization_deg, tasks.data(), n, &n);
  std::vector<IkOutDev> outs;
  double ms = 0;
  const int st = ik_run(p, tasks, outs, 1, check_self, check_map, &ms);
  if (st != SMP_OK) return st;
  p->last_check_ms = ms;
  // candidates below the chosen one always run to the end; those above it may have stopped early (IK_ABANDONED)
  int chosen = -1, reached = 0;
  for (int i = 0; i < n; ++i) {
    if (!outs[i].reached) continue;
    ++reached;
    if (chosen < 0 && (outs[i].flags & IK_VALID)) chosen = i;
  }
  *result = chosen >= 0 ? 0 : (reached ? 1 : 2);
  if (chosen >= 0)
    for (int j = 0; j < NJ; ++j) pose_goal[j] = outs[chosen].q[j];
  if (info) {
    info->n_candidates = n;
    info->n_reached = reached;
    info->chosen = chosen;
    info->downward = down;
    info->kernel_ms = ms;
  }
  return SMP_OK;
}

int smp_last_kernel_ms(const smp_planner* p, double* check_ms, double* plan_ms, int64_t* plan_launches) {
  if (!p) return SMP_ERR_ARG;
  if (check_ms) *check_ms = p->last_check_ms;
  if (plan_ms) *plan_ms = p->last_plan_ms;
  if (plan_launches) *plan_launches = p->last_plan_launches;
  return SMP_OK;
}

}  // extern "C"
