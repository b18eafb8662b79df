// C ABI implementation (include/smp_gpu.h), path tools: batched dense edge checks, shortcutting, one-via detours and
// path repair (kernels: smp_edges.hip, smp_repair.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "smp_planner.h"

using namespace smp;

extern "C" {

// ------------------------------------------------------------------------------------------ dense edge checks
// The density rule (include/smp_gpu.h, smp_check_edges): m hops of at most one planner step, the revolute and the
// prismatic length each summed for joints ascending as stepTowardsRandSample does (birrt_star.cpp:5712-5868).  False
// for a non-finite coordinate or more than SMP_EDGE_MAX_POINTS - 1 segments.
static bool edge_density(const smp_planner* p, const double* a, const double* b, int* m_out) {
  const int* rev = p->robot.dev.rev;
  double sr = 0.0, sp = 0.0;
  for (int j = 0; j < NJ; ++j) {
    if (!std::isfinite(a[j]) || !std::isfinite(b[j])) return false;
    const double d = b[j] - a[j];
    if (rev[j]) sr += d * d; else sp += d * d;
  }
  const double lr = std::sqrt(sr), lp = std::sqrt(sp);
  const double x = std::ceil(std::max(lr, lp) / p->params.step_factor);
  if (!(x * p->params.num_traj_segments <= (double)(SMP_EDGE_MAX_POINTS - 1))) return false;
  *m_out = x < 1.0 ? 1 : (int)x;
  return true;
}

static bool make_edge(const smp_planner* p, const double* a, const double* b, EdgeDev* e) {
  int m = 0;
  if (!edge_density(p, a, b, &m)) return false;
  for (int j = 0; j < NJ; ++j) { e->a[j] = a[j]; e->b[j] = b[j]; }
  e->M = p->params.num_traj_segments * m;
  e->pad = 0;
  return true;
}

// One edges_kernel launch over the table: first[i] = first colliding point of edge i, -1 if it is free.  The
// workgroups draw the edges longest first from a counter zeroed on the stream.
static int run_edges(smp_planner* p, const std::vector<EdgeDev>& edges, int self, int map, std::vector<int>& first,
                     double* kernel_ms) {
  const size_t n = edges.size();
  std::vector<int> order(n);
  for (size_t i = 0; i < n; ++i) order[i] = (int)i;
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return edges[x].M > edges[y].M; });
  first.assign(n, -1);
  HIPCHK(hipSetDevice(p->device));
  HIPCHK(p->d_edges.reserve(n));
  HIPCHK(p->d_eorder.reserve(n));
  HIPCHK(p->d_efirst.reserve(n));
  HIPCHK(p->d_ecounter.reserve(1));
  HIPCHK(hipMemcpyAsync(p->d_edges.p, edges.data(), n * sizeof(EdgeDev), hipMemcpyHostToDevice, p->stream));
  HIPCHK(hipMemcpyAsync(p->d_eorder.p, order.data(), n * sizeof(int), hipMemcpyHostToDevice, p->stream));
  HIPCHK(hipMemsetAsync(p->d_ecounter.p, 0, sizeof(unsigned), p->stream));
  const int grid = (int)std::min<size_t>(n, (size_t)p->num_cus);  // the tile's LDS admits one workgroup per CU
  HIPCHK(hipEventRecord(p->ev0, p->stream));
  launch_edges(grid, p->stream, p->d_rb, p->sc, p->d_mc, p->d_edges.p, p->d_eorder.p, (int)n, self,
               map && p->have_scene, p->d_ecounter.p, p->d_efirst.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(p->ev1, p->stream));
  HIPCHK(hipMemcpyAsync(first.data(), p->d_efirst.p, n * sizeof(int), hipMemcpyDeviceToHost, p->stream));
  HIPCHK(hipStreamSynchronize(p->stream));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, p->ev0, p->ev1));
  if (kernel_ms) *kernel_ms = ms;
  return SMP_OK;
}

// Batched isEdgeValid (birrt_star.cpp:6864-6895) at the density rule.
int smp_check_edges(smp_planner* p, const double* from_rows, const double* to_rows, int64_t n, int check_self,
                    int check_map, int64_t* first_invalid, int32_t* n_points) {
  if (!p || n < 0 || (n > 0 && (!from_rows || !to_rows || !first_invalid))) return SMP_ERR_ARG;
  if (int b_ = busy_check(p)) return b_;
  if (n == 0) return SMP_OK;
  if (check_map && !p->have_scene) return SMP_ERR_ARG;
  if (n > SMP_EDGE_TABLE_MAX) return SMP_ERR_CAPACITY;
  std::vector<EdgeDev> edges((size_t)n);
  for (int64_t i = 0; i < n; ++i)
    if (!make_edge(p, from_rows + i * NJ, to_rows + i * NJ, &edges[(size_t)i])) return SMP_ERR_ARG;
  std::vector<int> first;
  double ms = 0;
  const int st = run_edges(p, edges, check_self, check_map, first, &ms);
  if (st != SMP_OK) return st;
  p->last_check_ms = ms;
  for (int64_t i = 0; i < n; ++i) {
    first_invalid[i] = first[(size_t)i];
    if (n_points) n_points[i] = edges[(size_t)i].M + 1;
  }
  return SMP_OK;
}

// Path shortcutting: every candidate waypoint pair checked densely in one launch, then the cheapest route through the
// valid pairs (host, fp64), with the via nodes of the chosen edges inserted.
int smp_shortcut_path(smp_planner* p, const double* waypoints, int64_t k, int check_self, int check_map, int window,
                      double** out_waypoints, int64_t* n_out, smp_shortcut_info* info) {
  if (!p || !waypoints || !out_waypoints || !n_out || k < 2) return SMP_ERR_ARG;
  const auto t_begin = std::chrono::steady_clock::now();
  *out_waypoints = nullptr;
  *n_out = 0;
  if (info) {
    std::memset(info, 0, sizeof(*info));
    info->first_blocked = -1;
  }
  if (int b_ = busy_check(p)) return b_;
  if (check_map && !p->have_scene) return SMP_ERR_ARG;
  if (k > SMP_EDGE_TABLE_MAX) return SMP_ERR_CAPACITY;
  const int64_t w = (window <= 0 || window > k - 1) ? k - 1 : window;
  // candidates (i, j), i < j <= i + w, in the order of the dynamic program: j ascending, then i ascending
  const int64_t n_edges = w * (k - 1) - w * (w - 1) / 2;
  if (n_edges > SMP_EDGE_TABLE_MAX) return SMP_ERR_CAPACITY;
  std::vector<EdgeDev> edges((size_t)n_edges);
  {
    size_t e = 0;
    for (int64_t j = 1; j < k; ++j)
      for (int64_t i = std::max<int64_t>(0, j - w); i < j; ++i, ++e)
        if (!make_edge(p, waypoints + i * NJ, waypoints + j * NJ, &edges[e])) return SMP_ERR_ARG;
  }
  std::vector<int> first;
  double ms = 0;
  const int st = run_edges(p, edges, check_self, check_map, first, &ms);
  if (st != SMP_OK) return st;
  auto dist = [&](int64_t i, int64_t j) {  // DH:128-156
    double s = 0.0;
    for (int c = 0; c < NJ; ++c) {
      const double d = waypoints[j * NJ + c] - waypoints[i * NJ + c];
      s += d * d;
    }
    return std::sqrt(s);
  };
  std::vector<double> dp((size_t)k, HUGE_VAL);
  std::vector<int64_t> pred((size_t)k, -1), pred_edge((size_t)k, -1);
  dp[0] = 0.0;
  int64_t n_valid = 0, checked = 0, first_blocked = -1;
  double cost_in = 0.0;
  {
    size_t e = 0;
    for (int64_t j = 1; j < k; ++j) {
      cost_in += dist(j - 1, j);
      for (int64_t i = std::max<int64_t>(0, j - w); i < j; ++i, ++e) {
        const int f = first[e];
        checked += f < 0 ? edges[e].M + 1 : f + 1;
        if (f >= 0) {
          if (i == j - 1 && first_blocked < 0) first_blocked = i;
          continue;
        }
        ++n_valid;
        const double c = dp[(size_t)i] + dist(i, j);
        if (c < dp[(size_t)j]) { dp[(size_t)j] = c; pred[(size_t)j] = i; pred_edge[(size_t)j] = (int64_t)e; }
      }
    }
  }
  const bool reached = pred[(size_t)(k - 1)] >= 0;
  int rc = SMP_ERR_NO_SOLUTION;
  if (reached) {
    std::vector<int64_t> route;  // edge indices, goal to start
    for (int64_t j = k - 1; j > 0; j = pred[(size_t)j]) route.push_back(pred_edge[(size_t)j]);
    const int nseg = p->params.num_traj_segments;
    int64_t rows = 1;
    for (int64_t e : route) rows += edges[(size_t)e].M / nseg;
    double* out = static_cast<double*>(std::malloc((size_t)rows * NJ * sizeof(double)));
    if (!out) return SMP_ERR_CAPACITY;
    int64_t r = 0;
    for (size_t t = route.size(); t-- > 0;) {
      const EdgeDev& ed = edges[(size_t)route[t]];
      double step[NJ];
      for (int c = 0; c < NJ; ++c) step[c] = (ed.b[c] - ed.a[c]) / (double)ed.M;
      for (int h = 0; h < ed.M; h += nseg, ++r)  // the start waypoint (h = 0), then the via nodes
        for (int c = 0; c < NJ; ++c) out[r * NJ + c] = h == 0 ? ed.a[c] : ed.a[c] + (double)h * step[c];
    }
    for (int c = 0; c < NJ; ++c) out[r * NJ + c] = waypoints[(k - 1) * NJ + c];
    *out_waypoints = out;
    *n_out = rows;
    rc = SMP_OK;
  }
  if (info) {
    info->n_edges = n_edges;
    info->n_valid = n_valid;
    info->configs_checked = checked;
    info->cost_in = cost_in;
    info->cost_out = reached ? dp[(size_t)(k - 1)] : 0.0;
    info->first_blocked = reached ? -1 : first_blocked;
    info->kernel_ms = ms;
    info->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  }
  p->last_check_ms = ms;
  return rc;
}

// ------------------------------------------------------------------------------------------ path repair
static_assert(sizeof(smp_detour) == sizeof(DetourDev), "smp_detour is the kernel's record");

// One detours_kernel launch: out[g * samples + s] for the gaps of the table, items drawn from a counter zeroed on the
// stream.
static int run_detours(smp_planner* p, const std::vector<GapDev>& gaps, int samples, double h, uint64_t seed,
                       uint32_t round, int self, int map, DetourDev* out, double* kernel_ms) {
  const size_t n_items = gaps.size() * (size_t)samples;
  HIPCHK(hipSetDevice(p->device));
  HIPCHK(p->d_gaps.reserve(gaps.size()));
  HIPCHK(p->d_detours.reserve(n_items));
  HIPCHK(p->d_ecounter.reserve(1));
  HIPCHK(hipMemcpyAsync(p->d_gaps.p, gaps.data(), gaps.size() * sizeof(GapDev), hipMemcpyHostToDevice, p->stream));
  HIPCHK(hipMemsetAsync(p->d_ecounter.p, 0, sizeof(unsigned), p->stream));
  DetourArgs a;
  a.n_items = (int)n_items;
  a.samples = samples;
  a.n_seg = p->params.num_traj_segments;
  a.max_points = SMP_EDGE_MAX_POINTS;
  a.self = self;
  a.map = map && p->have_scene;
  a.round = round;
  a.seed = seed;
  a.step = p->params.step_factor;
  a.h = h;
  const int grid = (int)std::min<size_t>(n_items, (size_t)p->num_cus);  // the tile's LDS admits one workgroup per CU
  HIPCHK(hipEventRecord(p->ev0, p->stream));
  launch_detours(grid, p->stream, p->d_rb, p->sc, p->d_mc, p->d_gaps.p, a, p->d_ecounter.p, p->d_detours.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(p->ev1, p->stream));
  HIPCHK(hipMemcpyAsync(out, p->d_detours.p, n_items * sizeof(DetourDev), hipMemcpyDeviceToHost, p->stream));
  HIPCHK(hipStreamSynchronize(p->stream));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, p->ev0, p->ev1));
  if (kernel_ms) *kernel_ms = ms;
  return SMP_OK;
}

static bool finite_rows(const double* rows, int64_t n) {
  for (int64_t i = 0; i < n * NJ; ++i)
    if (!std::isfinite(rows[i])) return false;
  return true;
}

int smp_sample_detours(smp_planner* p, const double* from_rows, const double* to_rows, int64_t n_gaps, int samples,
                       double half_width, uint64_t seed, uint32_t round, int check_self, int check_map,
                       smp_detour* out) {
  if (!p || n_gaps < 0 || samples < 1 || !std::isfinite(half_width) || (n_gaps > 0 && (!from_rows || !to_rows || !out)))
    return SMP_ERR_ARG;
  if (int b_ = busy_check(p)) return b_;
  if (n_gaps == 0) return SMP_OK;
  if (check_map && !p->have_scene) return SMP_ERR_ARG;
  if (n_gaps > SMP_EDGE_TABLE_MAX || n_gaps * (int64_t)samples > SMP_EDGE_TABLE_MAX) return SMP_ERR_CAPACITY;
  if (!finite_rows(from_rows, n_gaps) || !finite_rows(to_rows, n_gaps)) return SMP_ERR_ARG;
  std::vector<GapDev> gaps((size_t)n_gaps);
  for (int64_t g = 0; g < n_gaps; ++g) {
    for (int j = 0; j < NJ; ++j) {
      gaps[(size_t)g].a[j] = from_rows[g * NJ + j];
      gaps[(size_t)g].b[j] = to_rows[g * NJ + j];
    }
    gaps[(size_t)g].g = (unsigned)g;
    gaps[(size_t)g].pad = 0;
  }
  double ms = 0;
  const int st = run_detours(p, gaps, samples, half_width, seed, round, check_self, check_map,
                             reinterpret_cast<DetourDev*>(out), &ms);
  if (st != SMP_OK) return st;
  p->last_check_ms = ms;
  return SMP_OK;
}

void smp_repair_opts_default(smp_repair_opts* o) {
  if (!o) return;
  o->samples = 256;
  o->rounds = 4;
  o->seed = 1;
}

// Path repair: the waypoints and the adjacent edges checked, the blocked stretches gathered into gaps between valid
// waypoints, and each gap bridged by the cheapest free one-via detour of the first round that has one.
int smp_repair_path(smp_planner* p, const double* waypoints, int64_t k, int check_self, int check_map,
                    const smp_repair_opts* opts, double** out_waypoints, int64_t* n_out, smp_repair_info* info) {
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
  if (check_map && !p->have_scene) return SMP_ERR_ARG;
  if (k > SMP_EDGE_TABLE_MAX) return SMP_ERR_CAPACITY;
  if (!finite_rows(waypoints, k)) return SMP_ERR_ARG;
  auto W = [&](int64_t i) { return waypoints + i * NJ; };
  auto dist = [](const double* a, const double* b) {  // DH:128-156
    double s = 0.0;
    for (int c = 0; c < NJ; ++c) {
      const double d = b[c] - a[c];
      s += d * d;
    }
    return std::sqrt(s);
  };
  double kernel_ms = 0, ms = 0;
  // 1. validity of the waypoints and of the adjacent edges
  std::vector<uint8_t> valid((size_t)k);
  {
    std::vector<double> soa((size_t)k * NJ);
    for (int64_t i = 0; i < k; ++i)
      for (int j = 0; j < NJ; ++j) soa[(size_t)j * k + i] = W(i)[j];
    const int st = smp_check_configs(p, soa.data(), k, check_self, check_map, valid.data());
    if (st != SMP_OK) return st;
    kernel_ms += p->last_check_ms;
  }
  if (!valid[0]) return SMP_ERR_START_INVALID;
  if (!valid[(size_t)(k - 1)]) return SMP_ERR_GOAL_INVALID;
  std::vector<EdgeDev> edges((size_t)(k - 1));
  for (int64_t i = 0; i + 1 < k; ++i)
    if (!make_edge(p, W(i), W(i + 1), &edges[(size_t)i])) return SMP_ERR_ARG;
  std::vector<int> first;
  {
    const int st = run_edges(p, edges, check_self, check_map, first, &ms);
    if (st != SMP_OK) return st;
    kernel_ms += ms;
  }
  // 2. gaps: (l, r) waypoint indices of the anchors, e = the gap's smallest blocked edge
  struct Gap { int64_t l, r, e; bool open; double v[NJ]; };
  std::vector<Gap> gaps;
  int64_t n_blocked = 0;
  double cost_in = 0.0;
  for (int64_t i = 0; i + 1 < k; ++i) {
    cost_in += dist(W(i), W(i + 1));
    if (first[(size_t)i] < 0) continue;
    ++n_blocked;
    int64_t l = i, r = i + 1;
    while (!valid[(size_t)l]) --l;  // w_0 and w_k-1 are valid
    while (!valid[(size_t)r]) ++r;
    if (!gaps.empty() && l < gaps.back().r) {
      gaps.back().r = std::max(gaps.back().r, r);
    } else {
      Gap g{};
      g.l = l; g.r = r; g.e = i; g.open = true;
      gaps.push_back(g);
    }
  }
  const int64_t n_gaps = (int64_t)gaps.size();
  if (n_gaps * (int64_t)o.samples > SMP_EDGE_TABLE_MAX) return SMP_ERR_CAPACITY;
  // 3. rounds over the gaps still open
  int64_t n_items = 0, n_free = 0, n_open = n_gaps;
  int rounds_used = 0;
  std::vector<GapDev> table;
  std::vector<DetourDev> items;
  for (int rho = 0; rho < o.rounds && n_open > 0; ++rho) {
    table.clear();
    for (int64_t g = 0; g < n_gaps; ++g) {
      if (!gaps[(size_t)g].open) continue;
      GapDev d;
      for (int j = 0; j < NJ; ++j) {
        d.a[j] = W(gaps[(size_t)g].l)[j];
        d.b[j] = W(gaps[(size_t)g].r)[j];
      }
      d.g = (unsigned)g;
      d.pad = 0;
      table.push_back(d);
    }
    items.resize(table.size() * (size_t)o.samples);
    const double h = std::ldexp(p->params.step_factor, rho);
    const int st = run_detours(p, table, o.samples, h, o.seed, (uint32_t)rho, check_self, check_map, items.data(), &ms);
    if (st != SMP_OK) return st;
    kernel_ms += ms;
    ++rounds_used;
    n_items += (int64_t)items.size();
    for (size_t t = 0; t < table.size(); ++t) {
      Gap& g = gaps[table[t].g];
      double best = HUGE_VAL;
      int chosen = -1;
      for (int s = 0; s < o.samples; ++s) {
        const DetourDev& it = items[t * (size_t)o.samples + (size_t)s];
        if (!it.free) continue;
        ++n_free;
        const double c = dist(table[t].a, it.v) + dist(it.v, table[t].b);
        if (c < best) { best = c; chosen = s; }
      }
      if (chosen >= 0) {
        for (int j = 0; j < NJ; ++j) g.v[j] = items[t * (size_t)o.samples + (size_t)chosen].v[j];
        g.open = false;
        --n_open;
      }
    }
  }
  int rc = SMP_OK;
  int64_t first_blocked = -1;
  double cost_out = 0.0;
  if (n_open > 0) {
    rc = SMP_ERR_NO_SOLUTION;  // 4.
    for (const Gap& g : gaps)
      if (g.open) { first_blocked = g.e; break; }
  } else {
    // 5. the route's rows, then the via nodes of every route edge between them
    std::vector<const double*> route;
    {
      size_t g = 0;
      for (int64_t i = 0; i < k;) {
        route.push_back(W(i));
        if (g < gaps.size() && gaps[g].l == i) {
          route.push_back(gaps[g].v);
          i = gaps[g].r;
          ++g;
        } else {
          ++i;
        }
      }
    }
    const int nseg = p->params.num_traj_segments;
    std::vector<EdgeDev> re(route.size() - 1);
    int64_t rows = 1;
    for (size_t t = 0; t + 1 < route.size(); ++t) {
      if (!make_edge(p, route[t], route[t + 1], &re[t])) return SMP_ERR_ARG;
      rows += re[t].M / nseg;
      cost_out += dist(route[t], route[t + 1]);
    }
    double* out = static_cast<double*>(std::malloc((size_t)rows * NJ * sizeof(double)));
    if (!out) return SMP_ERR_CAPACITY;
    int64_t r = 0;
    for (const EdgeDev& ed : re) {
      double step[NJ];
      for (int c = 0; c < NJ; ++c) step[c] = (ed.b[c] - ed.a[c]) / (double)ed.M;
      for (int h = 0; h < ed.M; h += nseg, ++r)  // the edge's start (h = 0), then its via nodes
        for (int c = 0; c < NJ; ++c) out[r * NJ + c] = h == 0 ? ed.a[c] : ed.a[c] + (double)h * step[c];
    }
    for (int c = 0; c < NJ; ++c) out[r * NJ + c] = W(k - 1)[c];
    *out_waypoints = out;
    *n_out = rows;
  }
  if (info) {
    info->n_blocked_edges = n_blocked;
    info->n_gaps = n_gaps;
    info->n_repaired = n_gaps - n_open;
    info->n_items = n_items;
    info->n_free = n_free;
    info->rounds_used = rounds_used;
    info->cost_in = cost_in;
    info->cost_out = cost_out;
    info->first_blocked = first_blocked;
    info->kernel_ms = kernel_ms;
    info->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  }
  p->last_check_ms = kernel_ms;
  return rc;
}

void smp_buffer_free(void* buffer) { std::free(buffer); }

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
  const int n_items = (int)((n + CLEAR_CT - 1) / CLEAR_CT);
  HIPCHK(hipSetDevice(p->device));
  HIPCHK(p->d_clq.reserve((size_t)n * NJ));
  HIPCHK(p->d_clc.reserve((size_t)n));
  HIPCHK(p->d_ecounter.reserve(1));
  HIPCHK(hipMemcpyAsync(p->d_clq.p, q_rows, (size_t)n * NJ * sizeof(double), hipMemcpyHostToDevice, p->stream));
  HIPCHK(hipMemsetAsync(p->d_ecounter.p, 0, sizeof(unsigned), p->stream));
  const int grid = std::min(n_items, p->num_cus);  // the tile's LDS admits one workgroup per CU
  HIPCHK(hipEventRecord(p->ev0, p->stream));
  launch_clearance(grid, p->stream, p->d_rb, p->sc, p->d_mc, cfg, p->d_clq.p, (long long)n, nullptr, nullptr, n_items,
                   p->d_ecounter.p, p->d_clc.p, nullptr);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(p->ev1, p->stream));
  HIPCHK(hipMemcpyAsync(out, p->d_clc.p, (size_t)n * sizeof(ClearDev), hipMemcpyDeviceToHost, p->stream));
  HIPCHK(hipStreamSynchronize(p->stream));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, p->ev0, p->ev1));
  p->last_check_ms = ms;
  if (info) {
    info->n_points = n;
    info->kernel_ms = ms;
    info->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  }
  return SMP_OK;
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
  std::vector<EdgeDev> edges((size_t)n);
  int64_t points = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (!make_edge(p, from_rows + i * NJ, to_rows + i * NJ, &edges[(size_t)i])) return SMP_ERR_ARG;
    points += edges[(size_t)i].M + 1;
  }
  std::vector<int> order((size_t)n);
  for (int64_t i = 0; i < n; ++i) order[(size_t)i] = (int)i;
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return edges[x].M > edges[y].M; });
  HIPCHK(hipSetDevice(p->device));
  HIPCHK(p->d_edges.reserve((size_t)n));
  HIPCHK(p->d_eorder.reserve((size_t)n));
  HIPCHK(p->d_cle.reserve((size_t)n));
  HIPCHK(p->d_ecounter.reserve(1));
  HIPCHK(hipMemcpyAsync(p->d_edges.p, edges.data(), (size_t)n * sizeof(EdgeDev), hipMemcpyHostToDevice, p->stream));
  HIPCHK(hipMemcpyAsync(p->d_eorder.p, order.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, p->stream));
  HIPCHK(hipMemsetAsync(p->d_ecounter.p, 0, sizeof(unsigned), p->stream));
  const int grid = (int)std::min<int64_t>(n, p->num_cus);  // the tile's LDS admits one workgroup per CU
  HIPCHK(hipEventRecord(p->ev0, p->stream));
  launch_clearance(grid, p->stream, p->d_rb, p->sc, p->d_mc, cfg, nullptr, 0, p->d_edges.p, p->d_eorder.p, (int)n,
                   p->d_ecounter.p, nullptr, p->d_cle.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(p->ev1, p->stream));
  HIPCHK(hipMemcpyAsync(out, p->d_cle.p, (size_t)n * sizeof(EdgeClearDev), hipMemcpyDeviceToHost, p->stream));
  HIPCHK(hipStreamSynchronize(p->stream));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, p->ev0, p->ev1));
  p->last_check_ms = ms;
  if (info) {
    info->n_points = points;
    info->kernel_ms = ms;
    info->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  }
  return SMP_OK;
}

}  // extern "C"
