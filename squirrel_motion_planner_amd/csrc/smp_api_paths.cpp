// C ABI implementation (include/smp_gpu.h), path tools: batched dense edge checks, shortcutting, one-via detours and
// path repair, clearance queries, the margin variants of the passes and the base's free map (kernels: smp_edges.hip,
// smp_repair.hip, smp_clearance.hip, smp_margin.hip, smp_lattice.hip).  Every entry point validates, builds its tables, launches (run_pass),
// post-processes and fills its info record; the plain logic between the launches is smp_paths.cpp's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "smp_paths.h"
#include "smp_planner.h"
#include "smp_route.h"

using namespace smp;

// ------------------------------------------------------------------------------------------ one launch of a pass
// The launch protocol of every pass kernel (smp_pass.h's ticket_loop): the uploads, the work counter zeroed on the
// stream, the launch between the two events on min(n_items, CUs) workgroups -- the tiles' LDS admits one per CU --,
// the download, and the kernel's time once the stream is idle.  upload() reserves and fills the call's device tables
// and returns a status, launch(grid) starts the kernel, and the n_out records it leaves in d_out are copied to out.
template <typename T, typename Upload, typename Launch>
static int run_pass(smp_planner* p, size_t n_items, Upload&& upload, Launch&& launch, DBuf<T>& d_out, void* out,
                    size_t n_out, double* kernel_ms) {
  HIPCHK(hipSetDevice(p->device));
  HIPCHK(p->d_ecounter.reserve(1));
  HIPCHK(d_out.reserve(n_out));
  if (int st = upload()) return st;
  HIPCHK(hipMemsetAsync(p->d_ecounter.p, 0, sizeof(unsigned), p->stream));
  const int grid = (int)std::min<size_t>(n_items, (size_t)p->num_cus);
  HIPCHK(hipEventRecord(p->ev0, p->stream));
  launch(grid);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(p->ev1, p->stream));
  HIPCHK(hipMemcpyAsync(out, d_out.p, n_out * sizeof(T), hipMemcpyDeviceToHost, p->stream));
  HIPCHK(hipStreamSynchronize(p->stream));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, p->ev0, p->ev1));
  *kernel_ms = ms;
  return SMP_OK;
}

// The two times every info record ends with.
template <typename Info>
static void fill_times(Info* info, double kernel_ms, std::chrono::steady_clock::time_point t_begin) {
  info->kernel_ms = kernel_ms;
  info->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
}

static EdgeRule edge_rule(const smp_planner* p) {
  return EdgeRule{p->robot.dev.rev, p->params.step_factor, p->params.num_traj_segments, SMP_EDGE_MAX_POINTS};
}

// n records into a device table that grows to hold them (an upload of run_pass).
template <typename T>
static int upload(smp_planner* p, DBuf<T>& d, const T* src, size_t n) {
  HIPCHK(d.reserve(n));
  HIPCHK(hipMemcpyAsync(d.p, src, n * sizeof(T), hipMemcpyHostToDevice, p->stream));
  return SMP_OK;
}

// The edge table and its longest-first order into d_edges and d_eorder.
static int upload_edges(smp_planner* p, const std::vector<EdgeDev>& edges, const std::vector<int>& order) {
  if (int st = upload(p, p->d_edges, edges.data(), edges.size())) return st;
  return upload(p, p->d_eorder, order.data(), order.size());
}

// ------------------------------------------------------------------------------------------ the passes' predicate
// How a call checks its configurations, edges and detour items: the flags, and the margin tables when a part asked for
// has a positive margin (mg != nullptr: the kernels of smp_margin.hip; else the plain ones).  The host logic between
// the launches consumes valid, first_invalid and free and does not care which predicate produced them.
struct Checks {
  int self, map;
  const MarginCfg* mg;
};

// The margin tables of one call into *c; *on = whether a part asked for has a positive margin (false: the call is the
// plain one).  SMP_ERR_ARG for a margin that is not finite or negative, or a map margin whose largest prefilter
// threshold reaches the box-gap field's clamp (clear_cfg's rule for max_dist).
static int margin_cfg(const smp_planner* p, const smp_margin* margin, int self, int map, MarginCfg* c, bool* on) {
  *on = false;
  const double mm = margin ? margin->map : 0.0, ms = margin ? margin->self : 0.0;
  if (!std::isfinite(mm) || !std::isfinite(ms) || mm < 0.0 || ms < 0.0) return SMP_ERR_ARG;
  std::memset(c, 0, sizeof(*c));
  c->self = self ? 1 : 0;
  c->map = (map && p->have_scene) ? 1 : 0;
  c->mm = map ? mm : 0.0;
  c->ms = self ? ms : 0.0;
  if (c->mm > 0.0) {
    const RobotDev& d = p->robot.dev;
    auto threshold = [&](double r, uint32_t* out) {
      const double a = (r + c->mm + 1e-6) / p->scene_res;
      const double t = std::floor(a * a);
      if (!(t < 65535.0)) return false;
      *out = (uint32_t)t;
      return true;
    };
    for (int s = 0; s < d.n_sph; ++s) {
      if (!threshold(d.sph_r[s], &c->T[s])) return SMP_ERR_ARG;
      c->S[s] = margin_threshold(d.sph_r[s], c->mm);
    }
    for (int k = 0; k < d.n_prim; ++k) {
      const double hz = d.prim_type[k] == 1 ? d.prim_h[k * 3 + 2] : d.prim_h[k * 3 + 1];
      if (!threshold(std::sqrt(d.prim_rxy[k] * d.prim_rxy[k] + hz * hz), &c->pT[k])) return SMP_ERR_ARG;
    }
    c->Sp = margin_threshold(0.0, c->mm);
  }
  *on = c->mm > 0.0 || c->ms > 0.0;
  return SMP_OK;
}

// One launch over the table: first[i] = the first point of edge i that fails the predicate, -1 if none does.
static int run_edges(smp_planner* p, const std::vector<EdgeDev>& edges, const Checks& ck, std::vector<int>& first,
                     double* kernel_ms) {
  const size_t n = edges.size();
  const std::vector<int> order = longest_first(edges);
  first.assign(n, -1);
  return run_pass(
      p, n, [&] { return upload_edges(p, edges, order); },
      [&](int grid) {
        if (ck.mg)
          launch_margin_edges(grid, p->stream, p->d_rb, p->sc, p->d_mc, *ck.mg, p->d_edges.p, p->d_eorder.p, (int)n,
                              p->d_ecounter.p, p->d_efirst.p);
        else
          launch_edges(grid, p->stream, p->d_rb, p->sc, p->d_mc, p->d_edges.p, p->d_eorder.p, (int)n, ck.self,
                       ck.map && p->have_scene, p->d_ecounter.p, p->d_efirst.p);
      },
      p->d_efirst, first.data(), n, kernel_ms);
}

// One margin_configs_kernel launch: clear[i] for the n rows (row-major n x 8).
static int run_margin_configs(smp_planner* p, const MarginCfg& mg, const double* q_rows, int64_t n, uint8_t* clear,
                              double* kernel_ms) {
  const int n_items = (int)((n + PASS_CT - 1) / PASS_CT);
  return run_pass(
      p, (size_t)n_items, [&] { return upload(p, p->d_clq, q_rows, (size_t)n * NJ); },
      [&](int grid) {
        launch_margin_configs(grid, p->stream, p->d_rb, p->sc, p->d_mc, mg, p->d_clq.p, (long long)n, n_items,
                              p->d_ecounter.p, p->d_mclear.p);
      },
      p->d_mclear, clear, (size_t)n, kernel_ms);
}

static bool finite_rows(const double* rows, int64_t n) {
  for (int64_t i = 0; i < n * NJ; ++i)
    if (!std::isfinite(rows[i])) return false;
  return true;
}

extern "C" {

// The predicate on n rows (row-major n x 8): the batch checker, or the margin tiles.
static int check_rows(smp_planner* p, const Checks& ck, const double* rows, int64_t n, uint8_t* ok, double* kernel_ms) {
  if (ck.mg) return run_margin_configs(p, *ck.mg, rows, n, ok, kernel_ms);
  std::vector<double> soa((size_t)n * NJ);
  for (int64_t i = 0; i < n; ++i)
    for (int j = 0; j < NJ; ++j) soa[(size_t)j * n + i] = rows[i * NJ + j];
  const int st = smp_check_configs(p, soa.data(), n, ck.self, ck.map, ok);
  if (st == SMP_OK) *kernel_ms = p->last_check_ms;
  return st;
}

// ------------------------------------------------------------------------------------------ dense edge checks
static int check_edges_body(smp_planner* p, const double* from_rows, const double* to_rows, int64_t n,
                            const Checks& ck, int64_t* first_invalid, int32_t* n_points) {
  if (n > SMP_EDGE_TABLE_MAX) return SMP_ERR_CAPACITY;
  const EdgeRule rule = edge_rule(p);
  std::vector<EdgeDev> edges((size_t)n);
  for (int64_t i = 0; i < n; ++i)
    if (!make_edge(rule, from_rows + i * NJ, to_rows + i * NJ, &edges[(size_t)i])) return SMP_ERR_ARG;
  std::vector<int> first;
  double ms = 0;
  const int st = run_edges(p, edges, ck, first, &ms);
  if (st != SMP_OK) return st;
  p->last_check_ms = ms;
  for (int64_t i = 0; i < n; ++i) {
    first_invalid[i] = first[(size_t)i];
    if (n_points) n_points[i] = edges[(size_t)i].M + 1;
  }
  return SMP_OK;
}

// Batched isEdgeValid (birrt_star.cpp:6864-6895) at the density rule.
int smp_check_edges(smp_planner* p, const double* from_rows, const double* to_rows, int64_t n, int check_self,
                    int check_map, int64_t* first_invalid, int32_t* n_points) {
  if (!p || n < 0 || (n > 0 && (!from_rows || !to_rows || !first_invalid))) return SMP_ERR_ARG;
  if (int b_ = busy_check(p)) return b_;
  if (n == 0) return SMP_OK;
  if (check_map && !p->have_scene) return SMP_ERR_ARG;
  return check_edges_body(p, from_rows, to_rows, n, Checks{check_self, check_map, nullptr}, first_invalid, n_points);
}

int smp_check_edges_margin(smp_planner* p, const double* from_rows, const double* to_rows, int64_t n, int check_self,
                           int check_map, const smp_margin* margin, int64_t* first_invalid, int32_t* n_points) {
  if (!p || n < 0 || (n > 0 && (!from_rows || !to_rows || !first_invalid))) return SMP_ERR_ARG;
  if (int b_ = busy_check(p)) return b_;
  MarginCfg mg;
  bool on;
  if (int st = margin_cfg(p, margin, check_self, check_map, &mg, &on)) return st;
  if (n == 0) return SMP_OK;
  if (check_map && !p->have_scene) return SMP_ERR_ARG;
  return check_edges_body(p, from_rows, to_rows, n, Checks{check_self, check_map, on ? &mg : nullptr}, first_invalid,
                          n_points);
}

// The predicate on n configurations (row-major n x 8): clear[i] = 1 iff configuration i is clear.
int smp_check_configs_margin(smp_planner* p, const double* q_rows, int64_t n, int check_self, int check_map,
                             const smp_margin* margin, uint8_t* clear) {
  if (!p || n < 0 || (n > 0 && (!q_rows || !clear))) return SMP_ERR_ARG;
  if (int b_ = busy_check(p)) return b_;
  MarginCfg mg;
  bool on;
  if (int st = margin_cfg(p, margin, check_self, check_map, &mg, &on)) return st;
  if (on && check_map && !p->have_scene) return SMP_ERR_ARG;
  if (n == 0) return SMP_OK;
  if (on && n > SMP_EDGE_TABLE_MAX) return SMP_ERR_CAPACITY;
  if (on && !finite_rows(q_rows, n)) return SMP_ERR_ARG;
  double ms = 0;
  const int st = check_rows(p, Checks{check_self, check_map, on ? &mg : nullptr}, q_rows, n, clear, &ms);
  if (st == SMP_OK) p->last_check_ms = ms;
  return st;
}

// Path shortcutting: every candidate waypoint pair checked densely in one launch, then the cheapest route through the
// valid pairs (host, fp64), with the via nodes of the chosen edges inserted.
static int shortcut_body(smp_planner* p, const double* waypoints, int64_t k, int check_self, int check_map, int window,
                         const smp_margin* margin, double** out_waypoints, int64_t* n_out, smp_shortcut_info* info) {
  if (!p || !waypoints || !out_waypoints || !n_out || k < 2) return SMP_ERR_ARG;
  const auto t_begin = std::chrono::steady_clock::now();
  *out_waypoints = nullptr;
  *n_out = 0;
  if (info) {
    std::memset(info, 0, sizeof(*info));
    info->first_blocked = -1;
  }
  if (int b_ = busy_check(p)) return b_;
  MarginCfg mg;
  bool on;
  if (int st = margin_cfg(p, margin, check_self, check_map, &mg, &on)) return st;
  const Checks ck{check_self, check_map, on ? &mg : nullptr};
  if (check_map && !p->have_scene) return SMP_ERR_ARG;
  if (k > SMP_EDGE_TABLE_MAX) return SMP_ERR_CAPACITY;
  const int64_t w = shortcut_window(k, window);
  const int64_t n_edges = shortcut_candidates(k, w);
  if (n_edges > SMP_EDGE_TABLE_MAX) return SMP_ERR_CAPACITY;
  std::vector<EdgeDev> edges;
  if (!shortcut_edges(edge_rule(p), waypoints, k, w, &edges)) return SMP_ERR_ARG;
  std::vector<int> first;
  double ms = 0;
  const int st = run_edges(p, edges, ck, first, &ms);
  if (st != SMP_OK) return st;
  smp_shortcut_info s;
  const std::vector<EdgeDev> route = shortcut_route(waypoints, k, w, edges, first, &s);
  int rc = SMP_ERR_NO_SOLUTION;
  if (!route.empty()) {
    *out_waypoints = route_rows(route, p->params.num_traj_segments, n_out);
    if (!*out_waypoints) return SMP_ERR_CAPACITY;
    rc = SMP_OK;
  }
  if (info) {
    *info = s;
    fill_times(info, ms, t_begin);
  }
  p->last_check_ms = ms;
  return rc;
}

int smp_shortcut_path(smp_planner* p, const double* waypoints, int64_t k, int check_self, int check_map, int window,
                      double** out_waypoints, int64_t* n_out, smp_shortcut_info* info) {
  return shortcut_body(p, waypoints, k, check_self, check_map, window, nullptr, out_waypoints, n_out, info);
}

int smp_shortcut_path_margin(smp_planner* p, const double* waypoints, int64_t k, int check_self, int check_map,
                             int window, const smp_margin* margin, double** out_waypoints, int64_t* n_out,
                             smp_shortcut_info* info) {
  return shortcut_body(p, waypoints, k, check_self, check_map, window, margin, out_waypoints, n_out, info);
}

// ------------------------------------------------------------------------------------------ path repair
static_assert(sizeof(smp_detour) == sizeof(DetourDev), "smp_detour is the kernel's record");

// One launch of detour items: out[g * samples + s] for the gaps of the table.
static int run_detours(smp_planner* p, const std::vector<GapDev>& gaps, int samples, double h, uint64_t seed,
                       uint32_t round, const Checks& ck, DetourDev* out, double* kernel_ms) {
  const size_t n_items = gaps.size() * (size_t)samples;
  const DetourArgs a{(int)n_items, samples, p->params.num_traj_segments, SMP_EDGE_MAX_POINTS, ck.self,
                     ck.map && p->have_scene, round, seed, p->params.step_factor, h};
  return run_pass(
      p, n_items, [&] { return upload(p, p->d_gaps, gaps.data(), gaps.size()); },
      [&](int grid) {
        if (ck.mg)
          launch_margin_detours(grid, p->stream, p->d_rb, p->sc, p->d_mc, *ck.mg, p->d_gaps.p, a, p->d_ecounter.p,
                                p->d_detours.p);
        else
          launch_detours(grid, p->stream, p->d_rb, p->sc, p->d_mc, p->d_gaps.p, a, p->d_ecounter.p, p->d_detours.p);
      },
      p->d_detours, out, n_items, kernel_ms);
}

static GapDev make_gap(const double* a, const double* b, unsigned g) {
  GapDev d;
  for (int j = 0; j < NJ; ++j) { d.a[j] = a[j]; d.b[j] = b[j]; }
  d.g = g;
  d.pad = 0;
  return d;
}

static int sample_detours_body(smp_planner* p, const double* from_rows, const double* to_rows, int64_t n_gaps,
                               int samples, double half_width, uint64_t seed, uint32_t round, int check_self,
                               int check_map, const smp_margin* margin, smp_detour* out) {
  if (!p || n_gaps < 0 || samples < 1 || !std::isfinite(half_width) || (n_gaps > 0 && (!from_rows || !to_rows || !out)))
    return SMP_ERR_ARG;
  if (int b_ = busy_check(p)) return b_;
  MarginCfg mg;
  bool on;
  if (int st = margin_cfg(p, margin, check_self, check_map, &mg, &on)) return st;
  const Checks ck{check_self, check_map, on ? &mg : nullptr};
  if (n_gaps == 0) return SMP_OK;
  if (check_map && !p->have_scene) return SMP_ERR_ARG;
  if (n_gaps > SMP_EDGE_TABLE_MAX || n_gaps * (int64_t)samples > SMP_EDGE_TABLE_MAX) return SMP_ERR_CAPACITY;
  if (!finite_rows(from_rows, n_gaps) || !finite_rows(to_rows, n_gaps)) return SMP_ERR_ARG;
  std::vector<GapDev> gaps((size_t)n_gaps);
  for (int64_t g = 0; g < n_gaps; ++g) gaps[(size_t)g] = make_gap(from_rows + g * NJ, to_rows + g * NJ, (unsigned)g);
  double ms = 0;
  const int st = run_detours(p, gaps, samples, half_width, seed, round, ck, reinterpret_cast<DetourDev*>(out), &ms);
  if (st != SMP_OK) return st;
  p->last_check_ms = ms;
  return SMP_OK;
}

int smp_sample_detours(smp_planner* p, const double* from_rows, const double* to_rows, int64_t n_gaps, int samples,
                       double half_width, uint64_t seed, uint32_t round, int check_self, int check_map,
                       smp_detour* out) {
  return sample_detours_body(p, from_rows, to_rows, n_gaps, samples, half_width, seed, round, check_self, check_map,
                             nullptr, out);
}

int smp_sample_detours_margin(smp_planner* p, const double* from_rows, const double* to_rows, int64_t n_gaps,
                              int samples, double half_width, uint64_t seed, uint32_t round, int check_self,
                              int check_map, const smp_margin* margin, smp_detour* out) {
  return sample_detours_body(p, from_rows, to_rows, n_gaps, samples, half_width, seed, round, check_self, check_map,
                             margin, out);
}

void smp_repair_opts_default(smp_repair_opts* o) {
  if (!o) return;
  o->samples = 256;
  o->rounds = 4;
  o->seed = 1;
}

// Path repair: the waypoints and the adjacent edges checked, the blocked stretches gathered into gaps between valid
// waypoints, and each gap bridged by the cheapest free one-via detour of the first round that has one.
static int repair_body(smp_planner* p, const double* waypoints, int64_t k, int check_self, int check_map,
                       const smp_repair_opts* opts, const smp_margin* margin, double** out_waypoints, int64_t* n_out,
                       smp_repair_info* info) {
  if (!p || !waypoints || !out_waypoints || !n_out || k < 2) return SMP_ERR_ARG;
  const auto t_begin = std::chrono::steady_clock::now();
  *out_waypoints = nullptr;
  *n_out = 0;
  if (info) {
    std::memset(info, 0, sizeof(*info));
    info->first_blocked = -1;
  }
  smp_repair_opts o;
  smp_repair_opts_default(&o);
  if (opts) o = *opts;
  if (o.samples < 1 || o.rounds < 1 || o.rounds > 32) return SMP_ERR_ARG;
  if (int b_ = busy_check(p)) return b_;
  MarginCfg mg;
  bool on;
  if (int st = margin_cfg(p, margin, check_self, check_map, &mg, &on)) return st;
  const Checks ck{check_self, check_map, on ? &mg : nullptr};
  if (check_map && !p->have_scene) return SMP_ERR_ARG;
  if (k > SMP_EDGE_TABLE_MAX) return SMP_ERR_CAPACITY;
  if (!finite_rows(waypoints, k)) return SMP_ERR_ARG;
  auto W = [&](int64_t i) { return waypoints + i * NJ; };
  const EdgeRule rule = edge_rule(p);
  double kernel_ms = 0, ms = 0;
  // 1. validity of the waypoints and of the adjacent edges
  std::vector<uint8_t> valid((size_t)k);
  {
    const int st = check_rows(p, ck, waypoints, k, valid.data(), &ms);
    if (st != SMP_OK) return st;
    kernel_ms += ms;
  }
  if (!valid[0]) return SMP_ERR_START_INVALID;
  if (!valid[(size_t)(k - 1)]) return SMP_ERR_GOAL_INVALID;
  std::vector<EdgeDev> edges((size_t)(k - 1));
  for (int64_t i = 0; i + 1 < k; ++i)
    if (!make_edge(rule, W(i), W(i + 1), &edges[(size_t)i])) return SMP_ERR_ARG;
  std::vector<int> first;
  {
    const int st = run_edges(p, edges, ck, first, &ms);
    if (st != SMP_OK) return st;
    kernel_ms += ms;
  }
  // 2. gaps (both end waypoints are valid here, as find_gaps requires); r is what *info receives
  smp_repair_info r{};
  r.first_blocked = -1;
  std::vector<Gap> gaps = find_gaps(valid.data(), first.data(), k, &r.n_blocked_edges);
  for (int64_t i = 0; i + 1 < k; ++i) r.cost_in += dist(W(i), W(i + 1));
  const int64_t n_gaps = r.n_gaps = (int64_t)gaps.size();
  if (n_gaps * (int64_t)o.samples > SMP_EDGE_TABLE_MAX) return SMP_ERR_CAPACITY;
  // 3. rounds over the gaps still open
  int64_t n_open = n_gaps;
  std::vector<GapDev> table;
  std::vector<DetourDev> items;
  for (int rho = 0; rho < o.rounds && n_open > 0; ++rho) {
    table.clear();
    for (int64_t g = 0; g < n_gaps; ++g)
      if (gaps[(size_t)g].open) table.push_back(make_gap(W(gaps[(size_t)g].l), W(gaps[(size_t)g].r), (unsigned)g));
    items.resize(table.size() * (size_t)o.samples);
    const double h = std::ldexp(p->params.step_factor, rho);
    const int st = run_detours(p, table, o.samples, h, o.seed, (uint32_t)rho, ck, items.data(), &ms);
    if (st != SMP_OK) return st;
    kernel_ms += ms;
    ++r.rounds_used;
    r.n_items += (int64_t)items.size();
    for (size_t t = 0; t < table.size(); ++t)
      if (close_gap(&gaps[table[t].g], table[t].a, table[t].b, &items[t * (size_t)o.samples], o.samples, &r.n_free) >= 0)
        --n_open;
  }
  int rc = SMP_OK;
  if (n_open > 0) {
    rc = SMP_ERR_NO_SOLUTION;  // 4.
    for (const Gap& g : gaps)
      if (g.open) { r.first_blocked = g.e; break; }
  } else {
    // 5. the route's rows, then the via nodes of every route edge between them
    std::vector<EdgeDev> route;
    if (!repaired_route(rule, waypoints, k, gaps, &route, &r.cost_out)) return SMP_ERR_ARG;
    *out_waypoints = route_rows(route, p->params.num_traj_segments, n_out);
    if (!*out_waypoints) return SMP_ERR_CAPACITY;
  }
  r.n_repaired = n_gaps - n_open;
  if (info) {
    *info = r;
    fill_times(info, kernel_ms, t_begin);
  }
  p->last_check_ms = kernel_ms;
  return rc;
}

int smp_repair_path(smp_planner* p, const double* waypoints, int64_t k, int check_self, int check_map,
                    const smp_repair_opts* opts, double** out_waypoints, int64_t* n_out, smp_repair_info* info) {
  return repair_body(p, waypoints, k, check_self, check_map, opts, nullptr, out_waypoints, n_out, info);
}

int smp_repair_path_margin(smp_planner* p, const double* waypoints, int64_t k, int check_self, int check_map,
                           const smp_repair_opts* opts, const smp_margin* margin, double** out_waypoints, int64_t* n_out,
                           smp_repair_info* info) {
  return repair_body(p, waypoints, k, check_self, check_map, opts, margin, out_waypoints, n_out, info);
}

void smp_buffer_free(void* buffer) { std::free(buffer); }

// ------------------------------------------------------------------------------------------ the base's free map
// One launch over the tiles of the lattice's nodes; the kernels form the configurations themselves, so the call uploads
// nothing but its arguments, and the words it downloads are the caller's bit grid.
int smp_base_free_map(smp_planner* p, const smp_base_lattice* lat, const smp_margin* margin, uint32_t* free_bits,
                      smp_base_map_info* info) {
  if (!p || !lat || !free_bits) return SMP_ERR_ARG;
  const auto t_begin = std::chrono::steady_clock::now();
  if (info) std::memset(info, 0, sizeof(*info));
  if (int b_ = busy_check(p)) return b_;
  LatticeDev ld;
  if (int st = lattice_dev(lat, &ld)) return st;
  const smp_margin map_only{margin ? margin->map : 0.0, 0.0};
  MarginCfg mg;
  bool on;
  if (int st = margin_cfg(p, &map_only, 0, 1, &mg, &on)) return st;
  if (!p->have_scene) return SMP_ERR_ARG;
  const int n_items = (int)((ld.n + PASS_CT - 1) / PASS_CT);
  double ms = 0;
  const int st = run_pass(
      p, (size_t)n_items, [] { return (int)SMP_OK; },
      [&](int grid) {
        if (on)
          launch_margin_base_map(grid, p->stream, p->d_rb, p->sc, p->d_mc, mg, ld, n_items, p->d_ecounter.p,
                                 p->d_lbits.p);
        else
          launch_base_map(grid, p->stream, p->d_rb, p->sc, p->d_mc, ld, n_items, p->d_ecounter.p, p->d_lbits.p);
      },
      p->d_lbits, free_bits, (size_t)n_items, &ms);
  if (st != SMP_OK) return st;
  p->last_check_ms = ms;
  if (info) {
    info->n_nodes = ld.n;
    for (int i = 0; i < n_items; ++i) info->n_free += __builtin_popcount(free_bits[i]);
    fill_times(info, ms, t_begin);
  }
  return SMP_OK;
}

// ------------------------------------------------------------------------------------------ clearance queries
static_assert(sizeof(smp_clearance) == sizeof(ClearDev) && sizeof(smp_edge_clearance) == sizeof(EdgeClearDev),
              "smp_clearance and smp_edge_clearance are the kernel's records");

// The widened prefilter thresholds of one call (smp_clearance.h).  SMP_ERR_ARG for a max_dist that is not finite and
// positive, or whose largest threshold reaches the box-gap field's clamp.
static int clear_cfg(const smp_planner* p, double D, int with_self, int with_map, ClearCfg* c) {
  if (!std::isfinite(D) || !(D > 0.0)) return SMP_ERR_ARG;
  std::memset(c, 0, sizeof(*c));
  c->D = D;
  c->with_self = with_self ? 1 : 0;
  c->with_map = with_map ? 1 : 0;
  if (!with_map) return SMP_OK;
  const RobotDev& d = p->robot.dev;
  auto threshold = [&](double r, uint32_t* out) {
    const double a = (r + D + 1e-6) / p->scene_res;
    const double t = std::floor(a * a);
    if (!(t < 65535.0)) return false;
    *out = (uint32_t)t;
    return true;
  };
  for (int s = 0; s < d.n_sph; ++s)
    if (!threshold(d.sph_r[s], &c->T[s])) return SMP_ERR_ARG;
  for (int k = 0; k < d.n_prim; ++k) {
    const double hz = d.prim_type[k] == 1 ? d.prim_h[k * 3 + 2] : d.prim_h[k * 3 + 1];
    if (!threshold(std::sqrt(d.prim_rxy[k] * d.prim_rxy[k] + hz * hz), &c->pT[k])) return SMP_ERR_ARG;
  }
  return SMP_OK;
}

// What a clearance call leaves behind once its launch succeeded.
static int clearance_done(smp_planner* p, smp_clearance_info* info, int64_t points, double ms,
                          std::chrono::steady_clock::time_point t_begin) {
  p->last_check_ms = ms;
  if (info) {
    info->n_points = points;
    fill_times(info, ms, t_begin);
  }
  return SMP_OK;
}

int smp_clearance_configs(smp_planner* p, const double* q_rows, int64_t n, double max_dist, int with_self, int with_map,
                          smp_clearance* out, smp_clearance_info* info) {
  if (!p || n < 0 || (n > 0 && (!q_rows || !out))) return SMP_ERR_ARG;
  const auto t_begin = std::chrono::steady_clock::now();
  if (info) std::memset(info, 0, sizeof(*info));
  if (int b_ = busy_check(p)) return b_;
  if (with_map && !p->have_scene) return SMP_ERR_ARG;
  ClearCfg cfg;
  if (int st = clear_cfg(p, max_dist, with_self, with_map, &cfg)) return st;
  if (n == 0) return SMP_OK;
  if (n > SMP_EDGE_TABLE_MAX) return SMP_ERR_CAPACITY;
  if (!finite_rows(q_rows, n)) return SMP_ERR_ARG;
  const int n_items = (int)((n + PASS_CT - 1) / PASS_CT);
  double ms = 0;
  const int st = run_pass(
      p, (size_t)n_items, [&] { return upload(p, p->d_clq, q_rows, (size_t)n * NJ); },
      [&](int grid) {
        launch_clearance(grid, p->stream, p->d_rb, p->sc, p->d_mc, cfg, p->d_clq.p, (long long)n, nullptr, nullptr,
                         n_items, p->d_ecounter.p, p->d_clc.p, nullptr);
      },
      p->d_clc, out, (size_t)n, &ms);
  return st != SMP_OK ? st : clearance_done(p, info, n, ms, t_begin);
}

int smp_clearance_edges(smp_planner* p, const double* from_rows, const double* to_rows, int64_t n, double max_dist,
                        int with_self, int with_map, smp_edge_clearance* out, smp_clearance_info* info) {
  if (!p || n < 0 || (n > 0 && (!from_rows || !to_rows || !out))) return SMP_ERR_ARG;
  const auto t_begin = std::chrono::steady_clock::now();
  if (info) std::memset(info, 0, sizeof(*info));
  if (int b_ = busy_check(p)) return b_;
  if (with_map && !p->have_scene) return SMP_ERR_ARG;
  ClearCfg cfg;
  if (int st = clear_cfg(p, max_dist, with_self, with_map, &cfg)) return st;
  if (n == 0) return SMP_OK;
  if (n > SMP_EDGE_TABLE_MAX) return SMP_ERR_CAPACITY;
  const EdgeRule rule = edge_rule(p);
  std::vector<EdgeDev> edges((size_t)n);
  int64_t points = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (!make_edge(rule, from_rows + i * NJ, to_rows + i * NJ, &edges[(size_t)i])) return SMP_ERR_ARG;
    points += edges[(size_t)i].M + 1;
  }
  const std::vector<int> order = longest_first(edges);
  double ms = 0;
  const int st = run_pass(
      p, (size_t)n, [&] { return upload_edges(p, edges, order); },
      [&](int grid) {
        launch_clearance(grid, p->stream, p->d_rb, p->sc, p->d_mc, cfg, nullptr, 0, p->d_edges.p, p->d_eorder.p, (int)n,
                         p->d_ecounter.p, nullptr, p->d_cle.p);
      },
      p->d_cle, out, (size_t)n, &ms);
  return st != SMP_OK ? st : clearance_done(p, info, points, ms, t_begin);
}

}  // extern "C"
