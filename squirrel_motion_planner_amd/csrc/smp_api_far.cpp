// C ABI implementation (include/smp_gpu.h "Far goals"): smp_plan_far, the staged call -- the base's free map
// (smp_base_free_map, smp_api_paths.cpp), the route over it (smp_base_route, smp_route.cpp; with route_device
// smp_base_route_gpu, smp_api_field.cpp, whose answer is the same), the route's dense check
// (smp_shortcut_path_margin) and smp_plan for the tail.  It only composes entry points of the ABI: every stage is the
// call a caller could make itself, so the stages' results are theirs bit for bit.
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "smp_planner.h"
#include "smp_route.h"

using namespace smp;

namespace {

double ms_since(std::chrono::steady_clock::time_point t) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}

// out->waypoints = the rows `head` (n_head x 8) followed by the result's own rows from `skip` on.
int prefix_waypoints(smp_result* out, const double* head, int64_t n_head, int64_t skip) {
  const int64_t n_tail = out->n_waypoints > skip ? out->n_waypoints - skip : 0;
  double* w = (double*)std::malloc(sizeof(double) * NJ * (size_t)(n_head + n_tail));
  if (!w) return SMP_ERR_CAPACITY;
  std::memcpy(w, head, sizeof(double) * NJ * (size_t)n_head);
  if (n_tail > 0) std::memcpy(w + NJ * n_head, out->waypoints + NJ * skip, sizeof(double) * NJ * (size_t)n_tail);
  std::free(out->waypoints);
  out->waypoints = w;
  out->n_waypoints = n_head + n_tail;
  return SMP_OK;
}

}  // namespace

extern "C" void smp_far_opts_default(smp_far_opts* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->pitch = 0.1;
  o->n_theta = 8;
  const double folded[5] = {-0.7, 1.9, 0.0, 1.7, 0.0};  // pose_folded_arm (parameters.yaml:38)
  for (int j = 0; j < 5; ++j) o->arm[j] = folded[j];
  o->handover_distance = 2.0;
  o->map_margin = 0.0;
  o->window = 0;
  o->snap_cells = 2;
  o->route_device = 0;
}

extern "C" int smp_plan_far(smp_planner* p, const smp_query* q, const smp_far_opts* opts, smp_result* out,
                            smp_far_info* info) {
  if (!p || !q || !out) return SMP_ERR_ARG;
  const auto t_begin = std::chrono::steady_clock::now();
  std::memset(out, 0, sizeof(*out));
  smp_far_info I;
  std::memset(&I, 0, sizeof(I));
  I.check.first_blocked = -1;
  for (int k = 0; k < 3; ++k) I.route.from_node[k] = I.route.to_node[k] = I.handover_node[k] = -1;
  smp_far_opts o;
  smp_far_opts_default(&o);
  if (opts) o = *opts;
  // every return goes through here: the status into the result, the record to the caller
  auto leave = [&](int stage, int rc) {
    I.stage = stage;
    I.total_ms = ms_since(t_begin);
    if (info) *info = I;
    out->status = rc;
    return rc;
  };
  // 1. the lattice over the query's environment and its free map
  const bool confined = !(q->env_x[0] == 0.0 && q->env_x[1] == 0.0) && !(q->env_y[0] == 0.0 && q->env_y[1] == 0.0);
  if (!confined || !std::isfinite(o.handover_distance)) return leave(1, SMP_ERR_ARG);
  smp_base_lattice lat;
  if (int st = smp_base_lattice_fit(q->env_x, q->env_y, o.pitch, o.n_theta, 0.0, o.arm, &lat)) return leave(1, st);
  LatticeDev ld;
  if (int st = lattice_dev(&lat, &ld)) return leave(1, st);
  std::vector<uint32_t> bits((size_t)((ld.n + 31) / 32));
  const smp_margin margin{o.map_margin, 0.0};
  if (int st = smp_base_free_map(p, &lat, &margin, bits.data(), &I.map)) return leave(1, st);
  // 2. the route
  const auto t_route = std::chrono::steady_clock::now();
  double* rows = nullptr;
  int64_t n_rows = 0;
  int32_t* chain = nullptr;
  const int rs = o.route_device
                     ? smp_base_route_gpu(p, &lat, bits.data(), q->start, q->goal, o.snap_cells, &rows, &n_rows, &chain,
                                          &I.route, nullptr)
                     : smp_base_route(&lat, bits.data(), q->start, q->goal, o.snap_cells, &rows, &n_rows, &chain, &I.route);
  I.route_ms = ms_since(t_route);
  std::free(rows);  // (the rows wanted are those of the chain up to the handover)
  if (rs != SMP_OK) return leave(2, rs);
  // 3. the handover
  const int64_t j = handover_index(ld, chain, I.route.n_chain, o.handover_distance);
  for (int k = 0; k < 3; ++k) I.handover_node[k] = chain[3 * j + k];
  if (j == 0) {
    std::free(chain);
    const int rc = smp_plan(p, q, out);
    return leave(rc == SMP_OK ? 0 : 4, rc);
  }
  // 4. the route rows, checked densely and shortened
  std::vector<double> w(q->start, q->start + NJ);
  {
    const std::vector<double> r = chain_rows(ld, chain, j + 1);
    w.insert(w.end(), r.begin(), r.end());
  }
  std::free(chain);
  double* route = nullptr;
  int64_t n_route = 0;
  const int cs = smp_shortcut_path_margin(p, w.data(), (int64_t)(w.size() / NJ), q->check_self, q->check_map, o.window,
                                          &margin, &route, &n_route, &I.check);
  if (cs != SMP_OK) return leave(3, cs);
  // 5. the tail, from the last route row
  smp_query tail = *q;
  std::memcpy(tail.start, route + NJ * (n_route - 1), sizeof(double) * NJ);
  const int rc = smp_plan(p, &tail, out);
  I.n_route_rows = n_route;
  const bool has_path = rc == SMP_OK && out->n_waypoints > 0;
  const int ps = prefix_waypoints(out, route, n_route, has_path ? 1 : out->n_waypoints);
  std::free(route);
  if (ps != SMP_OK) {
    smp_result_free(out);
    I.n_route_rows = 0;
    return leave(4, ps);
  }
  return leave(rc == SMP_OK ? 0 : 4, rc);
}
