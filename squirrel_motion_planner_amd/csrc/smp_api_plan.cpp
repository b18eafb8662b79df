// C ABI implementation (include/smp_gpu.h), planning: smp_plan / smp_plan_batch / smp_plan_multi, their results and
// smp_get_tree.  The call runs as stages (plan_prepare, plan_launch_loop, plan_assemble) over one PlanCall; what each
// query gets of the device is smp_provision.cpp's rule.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "smp_kernels.h"
#include "smp_planner.h"
#include "smp_provision.h"

using namespace smp;

static_assert(PROV_MAX_SCOUTS == MAX_SCOUTS && PROV_SCAN_P == SCAN_P && PROV_SCAN_PNEAR == SCAN_PNEAR,
              "smp_provision.h restates smp_plan.h");

// Workgroups of BLOCK threads that can be resident at once on the device for plan_kernel (leaders, scouts and helpers
// of a launch are its blocks): occupancy per CU (registers, LDS) x CUs.
static int resident_slots(smp_planner* p) {
  if (p->slots_cache > 0) return std::max(1, p->slots_cache / std::max(1, p->slot_share));
  int occ_plan = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ_plan, reinterpret_cast<const void*>(&plan_kernel), BLOCK, 0) !=
      hipSuccess) {
    (void)hipGetLastError();
    return p->num_cus;
  }
  p->slots_cache = p->num_cus * std::max(1, occ_plan);
  return std::max(1, p->slots_cache / std::max(1, p->slot_share));
}

// ------------------------------------------------------------------------------------------ planning
// C = H * diag(1, .., 1, det H), H = I - 2 v v^T / v^T v, v = e1 - a (DESIGN.md "Informed sampling");
// a non-finite direction (start == goal in a block) falls back to a = e1 (the reference divides by zero).
static void householder_C(const double* a_in, int n, double* C) {
  double a[6], v[6], vv = 0.0;
  bool fin = true;
  for (int i = 0; i < n; ++i) { a[i] = a_in[i]; if (!std::isfinite(a[i])) fin = false; }
  if (!fin) for (int i = 0; i < n; ++i) a[i] = (i == 0) ? 1.0 : 0.0;
  for (int i = 0; i < n; ++i) { v[i] = (i == 0 ? 1.0 : 0.0) - a[i]; vv += v[i] * v[i]; }
  double det = vv == 0.0 ? 1.0 : -1.0;
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < n; ++k) {
      double h = (i == k ? 1.0 : 0.0) - (vv == 0.0 ? 0.0 : 2.0 * v[i] * v[k] / vv);
      C[i * n + k] = (k == n - 1) ? h * det : h;
    }
}

static void init_qstate(const smp_planner* p, const smp_query& q, int64_t cap, int via_cap, QState* S) {
  std::memset(S, 0, sizeof(QState));
  const RobotDev& rb = p->robot.dev;
  S->status = 0;
  S->phase = 0;
  S->A = 0;
  S->n[0] = S->n[1] = 1;
  S->cap = (int)cap;
  S->via_cap = via_cap;
  S->max_iter = q.budget_kind == SMP_BUDGET_ITERATIONS ? (long long)q.budget : (long long)1 << 62;
  S->max_checked = q.budget_kind == SMP_BUDGET_SAMPLES ? std::max<long long>((long long)q.budget, 1) : 0;
  S->first_iter = -1;
  S->last_iter = -1;
  S->cbest[0] = S->cbest[1] = S->cbest[2] = 10000.0;
  double a = 0, r = 0, pp = 0;  // distance_heuristics.cpp:160-217
  for (int j = 0; j < NJ; ++j) {
    double d = q.goal[j] - q.start[j];
    a += d * d;
    if (rb.rev[j]) r += d * d; else pp += d * d;
  }
  S->h0[0] = std::sqrt(a); S->h0[1] = std::sqrt(r); S->h0[2] = std::sqrt(pp);
  for (int j = 0; j < NJ; ++j) { S->qs[j] = q.start[j]; S->qg[j] = q.goal[j]; }
  double arev[6], apr[2];
  int ir = 0, ip = 0;
  for (int j = 0; j < NJ; ++j) {  // jointConfigEllipseInitialization (birrt_star.cpp:3472-3604)
    if (rb.rev[j]) { S->ctr_rev[ir] = (q.start[j] + q.goal[j]) / 2.0; arev[ir++] = (q.goal[j] - q.start[j]) / S->h0[1]; }
    else { S->ctr_pr[ip] = (q.start[j] + q.goal[j]) / 2.0; apr[ip++] = (q.goal[j] - q.start[j]) / S->h0[2]; }
  }
  householder_C(arev, 6, S->Crev);
  householder_C(apr, 2, S->Cpr);
  S->env_x[0] = q.env_x[0]; S->env_x[1] = q.env_x[1];
  S->env_y[0] = q.env_y[0]; S->env_y[1] = q.env_y[1];
  S->near_r = p->params.near_threshold;
  S->step = p->params.step_factor;
  S->opt_thresh = p->params.path_optimality_threshold;
  S->n_pts = p->params.num_traj_segments;
  S->max_near = p->params.max_near_nodes;
  S->tree_opt = p->params.tree_optimization;
  S->informed = p->params.informed_sampling;
  S->self = q.check_self;
  S->map = q.check_map && p->have_scene;
  S->seed = q.seed;
  S->query = q.query_id;
}

static hipError_t alloc_query(QueryBuffers& b, size_t cap, int via_cap, long long rows) {
  hipError_t e;
  if ((e = b.st.reserve(1))) return e;
  if ((e = b.q.reserve(cap * NJ * 2))) return e;
  if ((e = b.qf.reserve(cap * NJ * 2))) return e;
  if ((e = b.cost.reserve(cap * 3 * 2))) return e;
  if ((e = b.e_start.reserve(cap * NJ * 2))) return e;
  if ((e = b.e_target.reserve(cap * NJ * 2))) return e;
  if ((e = b.parent.reserve(cap * 2))) return e;
  if ((e = b.first_child.reserve(cap * 2))) return e;
  if ((e = b.next_sib.reserve(cap * 2))) return e;
  if ((e = b.prev_sib.reserve(cap * 2))) return e;
  if ((e = b.stack.reserve(cap))) return e;
  if ((e = b.path_nodes.reserve(cap * 2))) return e;
  if ((e = b.via.reserve(via_cap))) return e;
  if ((e = b.rows.reserve(std::max<long long>(rows, 1) * 5))) return e;
  if ((e = b.jb.reserve(1))) return e;
  for (int s = 0; s < MAX_SCOUTS; ++s) {
    if ((e = b.sjb[s].reserve(1))) return e;
    if ((e = b.scb[s].reserve(1))) return e;
    if ((e = b.svia[s].reserve(via_cap))) return e;
  }
  b.cap = cap;
  return hipSuccess;
}

static QueryDev make_qdev(QueryBuffers& b, size_t cap, long long rows, const PlanKnobs& k) {
  QueryDev d;
  std::memset(&d, 0, sizeof(d));
  d.st = b.st.p;
  for (int t = 0; t < 2; ++t) {
    TreeDev& T = d.tr[t];
    T.q = b.q.p + (size_t)t * cap * NJ;
    T.qf = b.qf.p + (size_t)t * cap * NJ;
    T.cost = b.cost.p + (size_t)t * cap * 3;
    T.e_start = b.e_start.p + (size_t)t * cap * NJ;
    T.e_target = b.e_target.p + (size_t)t * cap * NJ;
    T.parent = b.parent.p + (size_t)t * cap;
    T.first_child = b.first_child.p + (size_t)t * cap;
    T.next_sib = b.next_sib.p + (size_t)t * cap;
    T.prev_sib = b.prev_sib.p + (size_t)t * cap;
  }
  d.via = b.via.p;
  d.stack = b.stack.p;
  d.rows = b.rows.p;
  d.rows_cap = rows;
  d.path_nodes = b.path_nodes.p;
  d.jb = nullptr;
  d.sampler_jb = nullptr;
  d.nscouts = 0;
  d.pre_delay = 0;
  d.pre_commit = 0;
  d.pre_refresh = 0;
  for (int s = 0; s < MAX_SCOUTS; ++s) {
    d.scbs[s] = nullptr; d.sjbs[s] = nullptr; d.svias[s] = nullptr; d.sworkers_s[s] = 1;
  }
  d.scb = nullptr;
  d.sjb = nullptr;
  d.svia = nullptr;
  d.sworkers = 1;
  d.nworkers = 1;
  d.tile_ct = k.tile_ct;
  d.sampler = 0;
  d.trace = nullptr;
  d.ttff = nullptr;
  d.abort = nullptr;
  d.lfin = nullptr;
  d.lquota = 0;
  d.scan_min = k.scan_min;  // the split scans' knobs (smp_provision.h; DESIGN.md "Scans of large trees")
  d.scan_nshift = k.scan_nshift;
  d.scan_ps0 = k.scan_ps0;
  d.scan_pnn = k.scan_pnn;
  d.scan_pnear = k.scan_pnear;
  d.conn_ov_max = k.scout_conn_ov_max;
  return d;
}

// One smp_plan_batch call: what its stages share.
struct PlanCall {
  smp_planner* p;
  const smp_query* qs;
  int nq;
  std::chrono::steady_clock::time_point t_entry;
  PlanKnobs k;
  std::vector<QueryDev> qdev;     // every query's record
  std::vector<QueryDev> qlaunch;  // the launch's query records, compacted to the queries still running
  QState* S = nullptr;            // the loop states' host copies (smp_planner::h_st)
  std::vector<int> act;           // the queries still running
  std::vector<double> host_ttff;  // seconds from entry to each query's first path on the host's clock, -1: none yet
  std::vector<std::array<unsigned long long, 32>> scout_prof;
  std::vector<unsigned long long> scout_conn_ov;  // the scouts' ScoutBoard::conn_ov_n, summed
  Provision prov;                 // the current launch's provisioning
  int nh_first = 0, ns_first = 0;  // the first provisioning's helpers and scouts (the statistics report them)
  float total_ms = 0;
  int64_t launches = 0;
};

// SMP_HOST_PROF: microseconds from smp_plan entry to each host stage of the first launch (experiments)
static void hstamp(const PlanCall& c, const char* what) {
  if (c.k.host_prof)
    std::fprintf(stderr, "[smp host] %-22s %8.1f us\n", what,
                 std::chrono::duration<double>(std::chrono::steady_clock::now() - c.t_entry).count() * 1e6);
}

static void poll_ttff(PlanCall& c) {
  for (int i = 0; i < c.nq; ++i)
    if (c.host_ttff[i] < 0 && __atomic_load_n(&c.p->h_ttff[i], __ATOMIC_ACQUIRE))
      c.host_ttff[i] = std::chrono::duration<double>(std::chrono::steady_clock::now() - c.t_entry).count();
}

// The provisioning rule (smp_provision.cpp) for the queries `act`, written into their records with the boards the
// workgroups meet on.
static void provision_queries(PlanCall& c, const std::vector<int>& act) {
  smp_planner* p = c.p;
  ProvisionIn in;
  in.slots = resident_slots(p);
  in.num_cus = p->num_cus;
  in.num_xcd = p->num_xcd;
  in.slot_share = p->slot_share;
  in.helpers = p->params.helpers;
  in.scout = p->params.scout;
  std::vector<char> have_sol(act.size());
  for (size_t a = 0; a < act.size(); ++a) have_sol[a] = c.S[act[a]].have_sol ? 1 : 0;
  provision(in, c.k, have_sol.data(), (int)act.size(), &c.prov);
  const int nh = c.prov.nh, ns = c.prov.ns;
  for (size_t a = 0; a < act.size(); ++a) {
    const int i = act[a];
    const QueryProvision& qp = c.prov.q[a];
    QueryDev& d = c.qdev[i];
    d.jb = nh > 0 ? p->qb[i].jb.p : nullptr;
    d.sampler = qp.sampler;
    d.nworkers = qp.nworkers;
    d.nscouts = qp.nscouts;
    d.pre_delay = c.k.pre_delay;
    d.pre_commit = c.k.pre_commit;
    d.early_ask = c.k.early_ask;
    d.pre_refresh = c.k.pre_refresh;
    d.conn_check = c.k.conn_check;
    d.sampler_jb = p->qb[i].jb.p;
    for (int s = 0; s < ns; ++s) {
      d.sjbs[s] = p->qb[i].sjb[s].p;
      d.scbs[s] = p->qb[i].scb[s].p;
      d.svias[s] = p->qb[i].svia[s].p;
      d.sworkers_s[s] = qp.sworkers_s[s];
    }
  }
}

// The running queries' records, with the launch's end conditions, to the device.
static int upload_active(PlanCall& c) {
  smp_planner* p = c.p;
  const std::vector<int>& act = c.act;
  c.qlaunch.clear();
  const int quota = c.k.rebalance && act.size() >= 2 ? std::max(1, (int)act.size() / c.k.rebalance_div) : 0;
  for (int i : act) {
    c.qdev[i].lfin = p->d_lfin.p;
    c.qdev[i].lquota = quota;
    c.qdev[i].lticks = act.size() >= 2 && c.k.slice_ms > 0 ? (long long)(c.k.slice_ms * 1e-3 * p->wall_rate_hz) : 0;
    c.qlaunch.push_back(c.qdev[i]);
  }
  // (qlaunch outlives the copy: it changes only after the next launch has completed)
  if (!c.qlaunch.empty())
    HIPCHK(hipMemcpyAsync(p->d_qdev.p, c.qlaunch.data(), c.qlaunch.size() * sizeof(QueryDev), hipMemcpyHostToDevice,
                          p->stream));
  return SMP_OK;
}

// Stage 1: arguments, the queries' buffers and loop states, the host-mapped words, the first provisioning and upload.
static int plan_prepare(PlanCall& c) {
  smp_planner* p = c.p;
  const smp_query* qs = c.qs;
  const int nq = c.nq;
  HIPCHK(hipSetDevice(p->device));
  // arguments; init_planner's validity of start and goal (birrt_star.cpp:350-362) is the kernel's first step (its
  // first launch checks both with the query's own self / map flags: no separate check launch and wait here)
  std::vector<int> status(nq, SMP_OK);
  for (int i = 0; i < nq; ++i) {
    const int bk = qs[i].budget_kind;
    if (!(qs[i].budget >= 0) || (bk != SMP_BUDGET_ITERATIONS && bk != SMP_BUDGET_SECONDS && bk != SMP_BUDGET_SAMPLES))
      status[i] = SMP_ERR_ARG;
  }
  hstamp(c, "arguments checked");
  if ((int)p->qb.size() < nq) p->qb.resize(nq);
  c.qdev.resize(nq);
  // the loop states in pinned host memory: their uploads and read-backs are true asynchronous copies (a pageable
  // source is staged synchronously: tens of microseconds before the first launch, inside the time to a first path)
  if (p->n_st < nq) {
    if (p->h_st) (void)hipHostFree(p->h_st);
    p->h_st = nullptr;
    p->n_st = 0;
    HIPCHK(hipHostMalloc(&p->h_st, (size_t)nq * sizeof(QState), hipHostMallocDefault));
    p->n_st = nq;
  }
  QState* S = c.S = p->h_st;
  hstamp(c, "host states");
  std::vector<long long> rows_cap(nq, 0);
  for (int i = 0; i < nq; ++i) {
    const smp_query& q = qs[i];
    int64_t cap = p->params.node_capacity;
    const bool by_iter = q.budget_kind == SMP_BUDGET_ITERATIONS;
    long long iters = by_iter ? (long long)q.budget : 0;
    if (cap <= 0) {
      if (by_iter) cap = std::min<int64_t>(1024 + 16 * iters, (int64_t)1 << 27);
      else if (q.budget_kind == SMP_BUDGET_SAMPLES) cap = std::min<int64_t>(1024 + (int64_t)q.budget / 2, (int64_t)1 << 27);
      else cap = (int64_t)4 << 20;
    }
    rows_cap[i] = by_iter ? std::max<long long>(iters, 1) : 1 << 20;
    // via nodes one connect / choose-parent chain may add (a chain of step_factor steps across the workspace: a few
    // dozen on a 10 m map); an eighth of the tree capacity, so that a seconds budget's stop margin (two chains) leaves
    // three quarters of an explicit node_capacity usable.  A longer chain ends the run with SMP_ERR_CAPACITY.
    const int via_cap = (int)std::max<int64_t>(64, std::min<int64_t>(4096, cap / 8));
    HIPCHK(alloc_query(p->qb[i], (size_t)cap, via_cap, rows_cap[i]));
    if (i == 0) hstamp(c, "query 0 buffers");
    c.qdev[i] = make_qdev(p->qb[i], (size_t)cap, rows_cap[i], c.k);
    init_qstate(p, q, cap, via_cap, &S[i]);
    if (i == 0) hstamp(c, "query 0 state");
    if (q.budget_kind == SMP_BUDGET_SECONDS) {
      // the budget counts from smp_plan entry (start / goal checks and first-call allocation included); the kernel
      // turns the rest into a deadline when it records the planning start
      const double left = q.budget - std::chrono::duration<double>(std::chrono::steady_clock::now() - c.t_entry).count();
      S[i].has_deadline = 1;
      S[i].budget_ticks = (unsigned long long)(std::max(left, 0.0) * p->wall_rate_hz);
      S[i].stop_margin = 2 * via_cap + 4;  // nodes one iteration can add at most (two via chains + x_new + connection)
    }
    if (status[i] != SMP_OK) { S[i].status = status[i]; S[i].phase = 2; }
    if (by_iter && iters <= 0 && S[i].phase == 0) S[i].max_iter = 0;
    // (the two roots are written by the kernel's first launch from QState::qs / qg: no per-word uploads)
    HIPCHK(hipMemcpyAsync(c.qdev[i].st, &S[i], sizeof(QState), hipMemcpyHostToDevice, p->stream));
  }
  // the queries to launch: those not decided on the host (an invalid start / goal or argument)
  for (int i = 0; i < nq; ++i)
    if (S[i].phase != 2 && S[i].status == 0) c.act.push_back(i);
  if (c.act.empty()) {
    std::vector<int> all(nq);
    for (int i = 0; i < nq; ++i) all[i] = i;
    provision_queries(c, all);
  } else {
    provision_queries(c, c.act);
  }
  c.nh_first = c.prov.nh;
  c.ns_first = c.prov.ns;
  if (c.k.debug && !p->h_trace) HIPCHK(hipHostMalloc(&p->h_trace, 256 * sizeof(int), hipHostMallocMapped));
  if (c.k.debug) {
    int* trace_dev = nullptr;
    std::memset(p->h_trace, 0, 256 * sizeof(int));
    HIPCHK(hipHostGetDevicePointer((void**)&trace_dev, p->h_trace, 0));
    c.qdev[0].trace = trace_dev;
  }
  // first feasible path on the host's clock (from run_planner entry): the kernel sets a host-mapped flag
  // when it commits the first solution and the launch loop polls it
  if (p->n_ttff < nq) {
    if (p->h_ttff) (void)hipHostFree(p->h_ttff);
    p->h_ttff = nullptr;
    p->n_ttff = 0;
    HIPCHK(hipHostMalloc(&p->h_ttff, nq * sizeof(unsigned), hipHostMallocMapped | hipHostMallocCoherent));
    p->n_ttff = nq;
  }
  for (int i = 0; i < nq; ++i) __atomic_store_n(&p->h_ttff[i], 0u, __ATOMIC_RELAXED);
  {
    unsigned* dflag = nullptr;
    HIPCHK(hipHostGetDevicePointer((void**)&dflag, p->h_ttff, 0));
    for (int i = 0; i < nq; ++i) c.qdev[i].ttff = dflag + i;
  }
  // the abort word (QueryDev::abort): cleared for this call (busy_check has seen every earlier launch drain)
  if (!p->h_abort) HIPCHK(hipHostMalloc(&p->h_abort, sizeof(unsigned), hipHostMallocMapped | hipHostMallocCoherent));
  __atomic_store_n(p->h_abort, 0u, __ATOMIC_RELEASE);
  {
    unsigned* dabort = nullptr;
    HIPCHK(hipHostGetDevicePointer((void**)&dabort, p->h_abort, 0));
    for (int i = 0; i < nq; ++i) c.qdev[i].abort = dabort;
  }
  c.host_ttff.assign(nq, -1.0);
  HIPCHK(p->d_qdev.reserve(nq));
  HIPCHK(p->d_counts.reserve(2 * nq));
  HIPCHK(p->d_lfin.reserve(1));
  hstamp(c, "queries uploaded");
  if (int st = upload_active(c)) return st;
  hstamp(c, "provisioned");
  return SMP_OK;
}

// Stage 2, the launch loop: each launch advances every running query by up to `chunk` iterations; time budgets use a
// device deadline.
static int plan_launch_loop(PlanCall& c) {
  smp_planner* p = c.p;
  const smp_query* qs = c.qs;
  const int nq = c.nq;
  const PlanKnobs& k = c.k;
  QState* S = c.S;
  std::vector<int>& act = c.act;
  std::vector<int> sol_seen(nq, 0);
  double tmax = 0;
  for (int i = 0; i < nq; ++i) if (qs[i].budget_kind == SMP_BUDGET_SECONDS) tmax = std::max(tmax, qs[i].budget);
  auto t_begin = std::chrono::steady_clock::now();
  int chunk = k.chunk0;
  c.scout_prof.resize(nq);
  for (auto& a : c.scout_prof) a.fill(0);
  c.scout_conn_ov.assign(nq, 0);
  long long max_iters = 0;
  for (int i = 0; i < nq; ++i)
    if (qs[i].budget_kind != SMP_BUDGET_SECONDS) max_iters = std::max(max_iters, (long long)qs[i].budget);
  while (!act.empty()) {
    const int nh = c.prov.nh, ns = c.prov.ns;
    // no progress: never spin forever (a launch ended early by finished queries counts too)
    if (tmax == 0 && c.launches > max_iters / 256 + 64 + 2 * nq +
                                      (k.slice_ms > 0 ? (long long)(c.total_ms / k.slice_ms) * 2 : 0))
      return SMP_ERR_HIP;
    if (tmax > 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count() > tmax * 4 + k.wait_slack_s)
      return SMP_ERR_HIP;
    const int na = (int)act.size();
    HIPCHK(hipMemsetAsync(p->d_lfin.p, 0, sizeof(unsigned), p->stream));
    if (nh > 0) {
      // fresh boards before the launch (its helpers poll them from their start and leave on the leader's stop)
      hipLaunchKernelGGL(boards_reset_kernel, dim3(na * (1 + 2 * ns)), dim3(BLOCK), 0, p->stream, p->d_qdev.p, ns);
      HIPCHK(hipGetLastError());
    }
    if (c.launches == 0) hstamp(c, "boards reset issued");
    HIPCHK(hipEventRecord(p->ev0, p->stream));
    // one dispatch for every workgroup of the launch (plan_kernel): leaders at blocks [0, na), scout s of query q at
    // scout_base + s * round8(na) + q, helper h of query q at helper_base + h * na + q; scout_base and helper_base are
    // multiples of 8, so blocks b and b + 8 are dealt to the same XCD (a query's leader and scouts share one).  The
    // leaders and scouts come first in dispatch order, so their workgroups find CUs first.
    const int r8 = (na + 7) / 8 * 8;
    const int scout_base = ns > 0 ? r8 : 0;
    const int helper_base = nh > 0 ? (ns > 0 ? scout_base + ns * r8 : r8) : (1 << 30);
    const int grid = nh > 0 ? helper_base + na * nh : (ns > 0 ? scout_base + (ns - 1) * r8 + na : na);
    hipLaunchKernelGGL(plan_kernel, dim3(grid), dim3(BLOCK), 0, p->stream, p->d_rb, p->sc,
                       p->d_mc, p->d_qdev.p, na, scout_base, helper_base, chunk);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(p->ev1, p->stream));
    if (c.launches == 0) hstamp(c, "kernels launched");
    c.launches++;
    // time the first feasible path on the host: poll the flags while the launch runs -- spinning (with a yield) until
    // every query has its first path, then sleeping between polls; a seconds budget bounds the wait (SMP_DEBUG builds
    // skip this loop for the bounded diagnostic wait below)
    if (!k.debug) {
      hipError_t qe;
      while ((qe = hipEventQuery(p->ev1)) == hipErrorNotReady) {
        poll_ttff(c);
        bool all = true;
        for (int i : act) all = all && c.host_ttff[i] >= 0;
        if (all) std::this_thread::sleep_for(std::chrono::microseconds(50));
        else std::this_thread::yield();
        if (tmax > 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count() > tmax * 4 + k.wait_slack_s) {
          // the launch still runs on this planner's buffers: ask it to end (its leaders poll the abort word every
          // ABORT_EVERY iterations) and refuse calls until it has drained (busy_check)
          __atomic_store_n(p->h_abort, 1u, __ATOMIC_RELEASE);
          p->busy = true;
          return SMP_ERR_HIP;
        }
      }
      if (qe != hipSuccess) HIPCHK(qe);
      poll_ttff(c);
    }
    if (k.debug) {  // bounded wait: print the leader's progress markers if the launch does not finish
      auto tw = std::chrono::steady_clock::now();
      hipError_t qe;
      while ((qe = hipStreamQuery(p->stream)) == hipErrorNotReady || qe != hipSuccess) {
        if (qe != hipErrorNotReady || std::chrono::duration<double>(std::chrono::steady_clock::now() - tw).count() > 10.0) {
          if (qe != hipErrorNotReady) std::fprintf(stderr, "[smp] launch %lld failed: %s\n", (long long)c.launches, hipGetErrorString(qe));
          std::fprintf(stderr, "[smp] launch %lld did not finish in 10 s; leader trace:", (long long)c.launches);
          for (int i = 0; i < 8; ++i) std::fprintf(stderr, " %d", p->h_trace[i]);
          std::fprintf(stderr, "\n");
          std::_Exit(3);
        }
      }
    }
    for (int i : act)
      HIPCHK(hipMemcpyAsync(&S[i], c.qdev[i].st, sizeof(QState), hipMemcpyDeviceToHost, p->stream));
    if (ns > 0) {  // every scout's phase clocks, summed (per-pass averages divide by the summed pass count)
      HIPCHK(hipStreamSynchronize(p->stream));
      for (int i : act)
        for (int sc = 0; sc < ns; ++sc) {
          // conn_ov_n, cprof and prof lie side by side on the board: one copy
          static_assert(offsetof(ScoutBoard, prof) - offsetof(ScoutBoard, conn_ov_n) == 7 * sizeof(unsigned long long),
                        "ScoutBoard: conn_ov_n, cprof[6], prof[32]");
          unsigned long long w[7 + 32];
          HIPCHK(hipMemcpy(w, &c.qdev[i].scbs[sc]->conn_ov_n, sizeof(w), hipMemcpyDeviceToHost));
          const unsigned long long* sp = w + 7;
          for (int j = 0; j < 32; ++j) c.scout_prof[i][j] += sp[j];
          c.scout_conn_ov[i] += w[0];
          if (i == 0 && k.conn_prof) {  // SMP_CONN_PROF builds (tools/perf_probe.py): PlanLds::cprof, two per word
            unsigned v[12];
            for (int j = 0; j < 12; ++j) v[j] = (unsigned)(w[1 + j / 2] >> (32 * (j & 1)));
            const double us = p->wall_rate_hz * 1e-6;
            auto per = [&](unsigned t, unsigned n) { return n ? t / us / n : 0.0; };
            std::fprintf(stderr, "[smp] launch %lld scout %d: rewire jobs before a connect record %u, cgo there when the "
                         "window opened %u; second near sets %u, %.2f us each; SC_DONE -> SC_CONN %u times, %.2f us each "
                         "(cgo wait %.2f, scan %.2f, rest %.2f); rewire check %u times %.2f us, expand check %u times "
                         "%.2f us\n", (long long)c.launches, sc, v[0], v[1], v[2], per(v[3], v[2]), v[4], per(v[5], v[4]),
                         per(v[6], v[4]), per(v[7], v[4]), per(v[5] - v[6] - v[7], v[4]), v[9], per(v[8], v[9]), v[11],
                         per(v[10], v[11]));
          }
          if (i == 0 && k.debug_scouts) {  // per-scout passes and XCD (experiments)
            int xcc = 0;
            HIPCHK(hipMemcpy(&xcc, &c.qdev[i].scbs[sc]->xcc, sizeof(int), hipMemcpyDeviceToHost));
            std::fprintf(stderr, "[smp] launch %lld scout %d: passes %llu busy %.1f us idle %.1f us xcc %d\n",
                         (long long)c.launches, sc, sp[30], sp[31] / (p->wall_rate_hz * 1e-6), sp[28] / (p->wall_rate_hz * 1e-6),
                         xcc - 1);
          }
        }
    }
    HIPCHK(hipStreamSynchronize(p->stream));
    if (k.bounds) {
      int dbg[8];
      if (smp_debug_bounds(dbg) == 0 && dbg[0])
        std::fprintf(stderr, "[smp] bounds: %s:%d id %d block %d tree %d limit %d (launch %lld)\n", site_file(dbg[0]),
                     site_line(dbg[0]), dbg[1], dbg[2], dbg[3], dbg[4], (long long)c.launches);
    }
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, p->ev0, p->ev1));
    c.total_ms += ms;
    if (k.debug) {
      JobBoard jbh;
      const int i0 = act[0];
      if (nh > 0) HIPCHK(hipMemcpy(&jbh, c.qdev[i0].jb, sizeof(JobBoard), hipMemcpyDeviceToHost));
      std::fprintf(stderr, "[smp] launch %lld queries %d grid %d chunk %d: %.3f ms phase %d status %d iter %lld checked %lld"
                   " board stop %d job %u tile0 %llx\n", (long long)c.launches, na, na * (1 + nh), chunk, ms, S[i0].phase,
                   S[i0].status, S[i0].iter, S[i0].checked, nh ? jbh.stop : -1, nh ? (unsigned)(jbh.pay[0] >> 32) : 0u,
                   nh ? jbh.res[0] : 0ull);
    }
    std::vector<int> still;
    int solved_before = 0, solved_now = 0;
    for (int i : act) solved_before += sol_seen[i];
    for (int i : act)
      if (!(S[i].phase == 2 || S[i].status != 0)) still.push_back(i);
    for (int i : act) { sol_seen[i] = S[i].have_sol ? 1 : 0; solved_now += sol_seen[i]; }
    const bool shrank = still.size() < act.size();
    act.swap(still);
    if (act.empty()) break;
    // (a query that found its first path gives its pre-solution scouts back: re-provisioned too)
    if (shrank || (ns > c.prov.ns_base && solved_now != solved_before)) {
      if (k.rebalance) provision_queries(c, act);
      if (int st = upload_active(c)) return st;
    }
    if (chunk < 4096) chunk *= 2;
  }
  hstamp(c, "launch loop done");
#ifdef SMP_RING_CHECK
  smp_ringchk_dump();
#endif
  return SMP_OK;
}

// Stage 3: the paths extracted on the device, then every query's statistics, cost rows and waypoints.  done[i] is set
// once out[i] holds query i's complete result.
static int plan_assemble(PlanCall& c, smp_result* out, std::vector<char>& done) {
  smp_planner* p = c.p;
  const int nq = c.nq;
  QState* S = c.S;
  // path extraction reads every query's record: the full array again
  HIPCHK(hipMemcpyAsync(p->d_qdev.p, c.qdev.data(), nq * sizeof(QueryDev), hipMemcpyHostToDevice, p->stream));
  p->last_plan_ms = c.total_ms;
  p->last_plan_launches = c.launches;

  // path extraction
  hipLaunchKernelGGL(path_kernel, dim3(nq), dim3(64), 0, p->stream, p->d_qdev.p, p->d_counts.p);
  HIPCHK(hipGetLastError());
  std::vector<int> counts(2 * nq);
  HIPCHK(hipMemcpyAsync(counts.data(), p->d_counts.p, 2 * nq * sizeof(int), hipMemcpyDeviceToHost, p->stream));
  HIPCHK(hipStreamSynchronize(p->stream));
  int rc = SMP_OK;
  for (int i = 0; i < nq; ++i) {
    QState& s = S[i];
    smp_result& r = out[i];
    r.status = s.status != 0 ? s.status : (s.have_sol ? SMP_OK : SMP_ERR_NO_SOLUTION);
    smp_stats& st = r.stats;
    st.iterations = s.iter;
    st.first_solution_iter = s.first_iter;
    st.last_solution_iter = s.last_iter;
    st.configs_checked = s.checked;
    st.configs_valid = s.valid;
    st.time_first_solution = s.have_sol && s.t_first >= s.t0 ? (double)(s.t_first - s.t0) / p->wall_rate_hz : -1.0;
    st.time_total = s.t_end >= s.t0 ? (double)(s.t_end - s.t0) / p->wall_rate_hz : 0.0;
    st.time_first_solution_host = s.have_sol ? c.host_ttff[i] : -1.0;
    for (int k = 0; k < 3; ++k) { st.cost_best[k] = s.cbest[k]; st.cost_theoretical[k] = s.h0[k]; }
    st.nodes_start = s.n[0]; st.nodes_goal = s.n[1];
    st.edges_start = s.edges[0]; st.edges_goal = s.edges[1];
    st.rewires_start = s.rewires[0]; st.rewires_goal = s.rewires[1];
    st.connected_tree_is_start = s.conn_start;
    st.conn_node_b = s.nB.id; st.conn_node_a = s.nA.id;
    st.nn_nodes_scanned = s.nn_nodes;
    st.near_nodes_scanned = s.near_nodes;
    st.samples_precomputed = s.smp_hits;
    st.scout_nn_hits = s.sc_nn;
    st.scout_near_hits = s.sc_near;
    st.scout_edge_hits = s.sc_edge_hit;
    st.scout_edge_misses = s.sc_edge_miss;
    st.scout_conn_row_hits = s.sc_conn_row;
    st.scout_conn_batch_hits = s.sc_conn_batch;
    st.scout_conn_ov_hits = (int64_t)c.scout_conn_ov[i];
    st.scout_wait_seconds = (double)s.sc_wait / p->wall_rate_hz;
    for (int k = 0; k < 32; ++k) {
      const bool count = k == 8 || k == 11 || (k >= 20 && k < 28) || k == 30;
      st.scout_phase_seconds[k] = count ? (double)c.scout_prof[i][k] : (double)c.scout_prof[i][k] / p->wall_rate_hz;
    }
    st.helpers = c.nh_first;
    st.scout = c.ns_first;
    for (int k = 0; k < 32; ++k)
      st.phase_seconds[k] = (k == 8 || k == 11 || k >= 20) ? (double)s.prof[k] : (double)s.prof[k] / p->wall_rate_hz;
    if (i == 0) { p->last_n[0] = s.n[0]; p->last_n[1] = s.n[1]; }
    // cost rows
    r.n_cost_rows = s.n_rows;
    if (s.n_rows > 0) {
      r.cost_rows = (double*)malloc(sizeof(double) * 5 * s.n_rows);
      HIPCHK(hipMemcpy(r.cost_rows, p->qb[i].rows.p, sizeof(double) * 5 * s.n_rows, hipMemcpyDeviceToHost));
      for (int64_t k = 0; k < s.n_rows; ++k) r.cost_rows[k * 5 + 1] /= p->wall_rate_hz;
    }
    if (r.status != SMP_OK) { done[i] = 1; continue; }
    const int n_sp = counts[2 * i], n_gp = counts[2 * i + 1];  // path nodes of the start tree and of the goal tree
    const int np = p->params.num_traj_segments;
    // the path's edges (e_start, e_target of every path node, start-tree nodes root first, then the goal-tree nodes
    // from the connection) gathered on the device: one copy instead of one per value
    std::vector<double> pe((size_t)(n_sp + n_gp) * 2 * NJ);
    if (n_sp + n_gp > 0) {
      HIPCHK(p->d_path_edges.reserve(pe.size()));
      const int nthr = (int)pe.size();
      hipLaunchKernelGGL(path_edges_kernel, dim3((nthr + 255) / 256), dim3(256), 0, p->stream, p->d_qdev.p, i, n_sp,
                         n_gp, p->d_path_edges.p);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(pe.data(), p->d_path_edges.p, pe.size() * sizeof(double), hipMemcpyDeviceToHost, p->stream));
      HIPCHK(hipStreamSynchronize(p->stream));
    }
    std::vector<double> wp;
    for (int k = 0; k < n_sp + n_gp; ++k) {
      // start-tree edges contribute points 0 .. np-1; goal-tree edges reversed: points np .. 1, then point 0 of the
      // last one (computeFinalSolutionPathTrajectories, birrt_star.cpp:6173-6274)
      const double* a = &pe[(size_t)k * 2 * NJ];
      const double* b = a + NJ;
      double stp[NJ];
      for (int j = 0; j < NJ; ++j) stp[j] = (b[j] - a[j]) / double(np);
      if (k < n_sp) {
        for (int inc = 0; inc < np; ++inc)
          for (int j = 0; j < NJ; ++j) wp.push_back(a[j] + inc * stp[j]);
      } else {
        for (int inc = np; inc > 0; --inc)
          for (int j = 0; j < NJ; ++j) wp.push_back(a[j] + inc * stp[j]);
        if (k == n_sp + n_gp - 1)
          for (int j = 0; j < NJ; ++j) wp.push_back(a[j] + 0 * stp[j]);
      }
    }
    r.n_waypoints = (int64_t)(wp.size() / NJ);
    if (!wp.empty()) {
      r.waypoints = (double*)malloc(sizeof(double) * wp.size());
      std::memcpy(r.waypoints, wp.data(), sizeof(double) * wp.size());
    }
    done[i] = 1;
  }
  for (int i = 0; i < nq; ++i) if (out[i].status != SMP_OK && rc == SMP_OK) rc = out[i].status;
  hstamp(c, "results assembled");
  return rc;
}

// smp_plan_batch's body.  A call that fails on the way (a HIP error, the no-progress guard) returns early, and
// smp_plan_batch then reports that status in every result not yet complete (done[i] unset).
static int plan_batch_impl(smp_planner* p, const smp_query* qs, int nq, smp_result* out, std::vector<char>& done) {
  PlanCall c;
  c.t_entry = std::chrono::steady_clock::now();
  c.p = p;
  c.qs = qs;
  c.nq = nq;
  c.k = read_plan_knobs(p->params.helpers, nq);
  if (int st = plan_prepare(c)) return st;
  if (int st = plan_launch_loop(c)) return st;
  return plan_assemble(c, out, done);
}

extern "C" int smp_plan_batch(smp_planner* p, const smp_query* qs, int nq, smp_result* out) {
  if (!p || !qs || nq <= 0 || !out) return SMP_ERR_ARG;
  for (int i = 0; i < nq; ++i) std::memset(&out[i], 0, sizeof(smp_result));
  if (int b_ = busy_check(p)) {
    for (int i = 0; i < nq; ++i) out[i].status = b_;
    return b_;
  }
  std::vector<char> done(nq, 0);
  const int rc = plan_batch_impl(p, qs, nq, out, done);
  // the runtime's last-error slot still holds a failed call's error (e.g. an allocation): clear it, so the next
  // call's launch checks do not report it again
  if (rc == SMP_ERR_HIP) (void)hipGetLastError();
  // a call that stopped early leaves no result looking like a success
  for (int i = 0; i < nq; ++i) {
    if (done[i]) continue;
    smp_result_free(&out[i]);
    out[i].status = rc != SMP_OK ? rc : SMP_ERR_HIP;
  }
  return rc;
}

extern "C" int smp_plan(smp_planner* p, const smp_query* q, smp_result* out) { return smp_plan_batch(p, q, 1, out); }

// Queries dealt round-robin over the planners (query i -> planner i % np), one host thread per planner, so the
// planners' GPUs plan concurrently; out[i] is query i's result.  The return code is the first non-OK status in query
// order, as smp_plan_batch's.
extern "C" int smp_plan_multi(smp_planner* const* ps, int np, const smp_query* qs, int nq, smp_result* out) {
  if (!ps || np <= 0 || !qs || nq <= 0 || !out) return SMP_ERR_ARG;
  for (int i = 0; i < nq; ++i) std::memset(&out[i], 0, sizeof(smp_result));
  for (int k = 0; k < np; ++k)
    for (int j = 0; j <= k; ++j)
      if (!ps[k] || (j < k && ps[k] == ps[j])) {  // a planner is not thread-safe: each at most once
        for (int i = 0; i < nq; ++i) out[i].status = SMP_ERR_ARG;
        return SMP_ERR_ARG;
      }
  const int used = std::min(np, nq);
  std::vector<std::vector<smp_query>> part(used);
  std::vector<std::vector<smp_result>> res(used);
  for (int i = 0; i < nq; ++i) part[i % used].push_back(qs[i]);
  std::vector<int> rcs(used, SMP_OK);
  // planners on the same GPU run at once: each provisions its share of that GPU's co-resident workgroups (every
  // workgroup of a query polls the others, so all of them must be resident)
  for (int k = 0; k < used; ++k) {
    int same = 0;
    for (int j = 0; j < used; ++j) same += ps[j]->device == ps[k]->device;
    ps[k]->slot_share = same * ps[k]->proc_share;
  }
  std::vector<std::thread> th;
  th.reserve(used);
  for (int k = 0; k < used; ++k) {
    res[k].resize(part[k].size());
    th.emplace_back([&, k] { rcs[k] = smp_plan_batch(ps[k], part[k].data(), (int)part[k].size(), res[k].data()); });
  }
  for (auto& t : th) t.join();
  for (int k = 0; k < used; ++k) ps[k]->slot_share = ps[k]->proc_share;
  int rc = SMP_OK;
  for (int i = 0; i < nq; ++i) {
    out[i] = res[i % used][i / used];
    if (rc == SMP_OK && out[i].status != SMP_OK) rc = out[i].status;
  }
  for (int k = 0; k < used; ++k)
    if (rc == SMP_OK && rcs[k] != SMP_OK) rc = rcs[k];
  return rc;
}

extern "C" void smp_result_free(smp_result* r) {
  if (!r) return;
  free(r->waypoints);
  free(r->cost_rows);
  r->waypoints = nullptr;
  r->cost_rows = nullptr;
  r->n_waypoints = r->n_cost_rows = 0;
}

extern "C" int64_t smp_get_tree(smp_planner* p, int which, int32_t* parent, double* conf, double* cost) {
  if (!p || p->qb.empty() || which < 0 || which > 1) return -1;
  if (hipSetDevice(p->device) != hipSuccess) return -1;
  QueryBuffers& b = p->qb[0];
  size_t cap = b.cap;
  int n = p->last_n[which];
  if (parent && hipMemcpy(parent, b.parent.p + (size_t)which * cap, n * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  std::vector<double> tmp((size_t)n);
  if (conf)
    for (int j = 0; j < NJ; ++j) {
      if (hipMemcpy(tmp.data(), b.q.p + (size_t)which * cap * NJ + (size_t)j * cap, n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return -1;
      for (int i = 0; i < n; ++i) conf[(size_t)i * NJ + j] = tmp[i];
    }
  if (cost)
    for (int k = 0; k < 3; ++k) {
      if (hipMemcpy(tmp.data(), b.cost.p + (size_t)which * cap * 3 + (size_t)k * cap, n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return -1;
      for (int i = 0; i < n; ++i) cost[(size_t)i * 3 + k] = tmp[i];
    }
  return n;
}
