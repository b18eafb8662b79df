// Internal to the C ABI's translation units (smp_api*.cpp): the handles behind include/smp_gpu.h and their device
// buffers.  One definition for all of them: smp_planner is one type across translation units, and so are its members.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <set>
#include <string>
#include <vector>

#include "../../include/smp_gpu.h"
#include "smp_carve.h"
#include "smp_clearance.h"
#include "smp_field.h"
#include "smp_pass.h"
#include "smp_host.h"
#include "smp_ik.h"
#include "smp_margin.h"
#include "smp_plan.h"
#include "smp_types.h"

struct smp_robot {
  smp::RobotHost h;
};

struct smp_scene {
  smp::SceneHost h;
};

#define HIPCHK(x)                                                                        \
  do {                                                                                    \
    hipError_t e_ = (x);                                                                  \
    if (e_ != hipSuccess) {                                                               \
      fprintf(stderr, "smp_gpu: HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); \
      return SMP_ERR_HIP;                                                                 \
    }                                                                                     \
  } while (0)

namespace smp {

template <typename T>
struct DBuf {  // device buffer that only grows
  T* p = nullptr;
  size_t n = 0;
  hipError_t reserve(size_t want) {
    if (want <= n) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
    hipError_t e = hipMalloc(&p, std::max<size_t>(want, 1) * sizeof(T));
    if (e == hipSuccess) n = want;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
};

struct QueryBuffers {
  DBuf<QState> st;
  DBuf<double> q, cost, e_start, e_target, rows;
  DBuf<float> qf;
  DBuf<int> parent, first_child, next_sib, prev_sib, stack, path_nodes;
  DBuf<ViaNode> via;
  DBuf<JobBoard> jb;               // the leader's collision-job board
  DBuf<JobBoard> sjb[MAX_SCOUTS];  // the scouts' collision-job boards, record boards and via scratch
  DBuf<ScoutBoard> scb[MAX_SCOUTS];
  DBuf<ViaNode> svia[MAX_SCOUTS];
  size_t cap = 0;
  void release() {
    st.release(); q.release(); qf.release(); cost.release(); e_start.release(); e_target.release(); rows.release();
    parent.release(); first_child.release(); next_sib.release(); prev_sib.release(); stack.release();
    path_nodes.release(); via.release(); jb.release();
    for (int s = 0; s < MAX_SCOUTS; ++s) { sjb[s].release(); scb[s].release(); svia[s].release(); }
    cap = 0;
  }
};

}  // namespace smp

struct smp_planner {
  int device = 0;
  hipStream_t stream = nullptr;
  smp::RobotHost robot;
  smp_params params;
  smp::RobotDev* d_rb = nullptr;
  smp::MapCfg mc_host;
  smp::MapCfg* d_mc = nullptr;
  smp::DBuf<uint64_t> d_bricks;
  smp::DBuf<uint16_t> d_d2;
  smp::DBuf<uint8_t> d_d2b;
  smp::DBuf<uint16_t> d_slab;           // per-primitive 2-D slab fields (SceneDev::slab), n_prim x nx x ny
  // scratch of the device scene build (smp_planner_set_scene_keys): uploaded keys, two bit grids, the occupied-cell
  // count, the slabs' layer ranges
  smp::DBuf<uint16_t> d_keys;
  smp::DBuf<unsigned long long> d_sbits, d_sdil, d_scount;
  smp::DBuf<int> d_sk01;
  smp::SceneDev sc{};
  bool have_scene = false;
  double scene_res = 0.05;
  std::set<std::string> disabled;
  std::vector<smp::QueryBuffers> qb;
  smp::DBuf<smp::QueryDev> d_qdev;
  smp::DBuf<int> d_counts;
  smp::DBuf<unsigned> d_lfin;  // finished queries of the current launch
  smp::DBuf<double> d_cq;
  smp::DBuf<uint8_t> d_valid;
  smp::DBuf<smp::IkTaskDev> d_ik_tasks;
  smp::DBuf<smp::IkOutDev> d_ik_out;
  smp::DBuf<int> d_ik_best;
  smp::DBuf<double> d_path_edges;       // path_edges_kernel output (the path's edges, one copy to the host)
  // batched dense edge checks (smp_check_edges / smp_shortcut_path): edge table, longest-first order, results and
  // the work counter
  smp::DBuf<smp::EdgeDev> d_edges;
  smp::DBuf<int> d_eorder, d_efirst;
  smp::DBuf<unsigned> d_ecounter;
  // batched one-via detours (smp_sample_detours / smp_repair_path): gap table and per-item results; the work counter
  // is d_ecounter
  smp::DBuf<smp::GapDev> d_gaps;
  smp::DBuf<smp::DetourDev> d_detours;
  // clearance queries (smp_clearance_configs / smp_clearance_edges): configuration rows and per-item results; the edge
  // table, its order and the work counter are d_edges, d_eorder and d_ecounter
  smp::DBuf<double> d_clq;
  smp::DBuf<smp::ClearDev> d_clc;
  smp::DBuf<smp::EdgeClearDev> d_cle;
  // margin checks (smp_check_configs_margin): per-configuration results; the rows are d_clq, the other tables those of
  // the plain passes
  smp::DBuf<uint8_t> d_mclear;
  // the base's free map (smp_base_free_map): one word per tile of 32 lattice nodes; the work counter is d_ecounter
  smp::DBuf<uint32_t> d_lbits;
  // the cost field (smp_base_cost_field / smp_base_route_gpu): the uploaded free bits, the costs, the tiles' activity
  // flags of both round parities, a batch's per-round changed counters, parents, the walked chain, the small record
  smp::DBuf<uint32_t> d_fbits;
  smp::DBuf<double> d_fcost;
  smp::DBuf<unsigned> d_factive, d_fchanged;
  smp::DBuf<int32_t> d_fparent, d_fchain;
  smp::DBuf<smp::FieldStats> d_fstats;
  // self filter (smp_planner_set_carve / smp_carve_keys): the sticky carve of the device scene builds, its links by
  // name (resolved against the robot at every build), and the carve launches' scratch: the world items, the flags of
  // the standalone call, the carved-key count; ev2 / ev3 time the carve launches inside a build
  bool carve_on = false;
  double carve_q[smp::NJ] = {0}, carve_pad = 0.0;
  std::vector<std::string> carve_links;
  smp::DBuf<smp::CarveItems> d_citems;
  smp::DBuf<uint8_t> d_cflags;
  smp::DBuf<unsigned long long> d_ccount;
  hipEvent_t ev2 = nullptr, ev3 = nullptr;
  smp_carve_info last_carve{0, 0.0, 0.0};
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  double last_check_ms = 0, last_plan_ms = 0;
  int64_t last_plan_launches = 0;
  double wall_rate_hz = 1e8;
  int num_cus = 256;
  int num_xcd = 8;                 // XCDs (hipDeviceAttributeNumberOfXccs): the per-XCD helper budget of provision()
  unsigned* h_ttff = nullptr;      // host-mapped first-solution flags, one per query (QueryDev::ttff)
  unsigned* h_abort = nullptr;     // host-mapped abort word of the planner's launches (QueryDev::abort)
  smp::QState* h_st = nullptr;          // pinned host copies of the queries' loop states (asynchronous uploads)
  int* h_trace = nullptr;          // host-mapped progress markers of query 0's leader (SMP_DEBUG; QueryDev::trace)
  int n_st = 0;
  int n_ttff = 0;
  // last plan (query 0) bookkeeping for smp_get_tree
  int last_n[2] = {0, 0};
  int slots_cache = 0;  // resident_slots (occupancy queries) once per planner
  int slot_share = 1;   // planners planning on this planner's GPU at once (smp_plan_multi): its share of the slots
  // processes planning on this GPU at once (SMP_SLOT_SHARE, e.g. several ranks of one job on a one-GPU box): every
  // workgroup of a query must be co-resident, so each process provisions its share of the device
  int proc_share = 1;
  // a planning call gave up (SMP_ERR_HIP) while its kernels may still run on these buffers: every later call that
  // would touch them fails with SMP_ERR_HIP until both streams are idle again (busy_check), and destroy leaks them
  // rather than freeing memory a live kernel uses
  bool busy = false;
};

// SMP_OK once no kernel of an abandoned planning call runs any more (smp_planner::busy), else SMP_ERR_HIP.
inline int busy_check(smp_planner* p) {
  if (!p->busy) return SMP_OK;
  (void)hipSetDevice(p->device);
  if (hipStreamQuery(p->stream) == hipErrorNotReady) return SMP_ERR_HIP;
  (void)hipGetLastError();
  p->busy = false;
  return SMP_OK;
}
