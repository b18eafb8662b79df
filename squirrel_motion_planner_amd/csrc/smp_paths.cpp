// Host logic of the path tools (smp_paths.h): plain C++17, no HIP.
#include "smp_paths.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace smp {

bool make_edge(const EdgeRule& r, const double* a, const double* b, EdgeDev* e) {
  double sr = 0.0, sp = 0.0;
  for (int j = 0; j < NJ; ++j) {
    if (!std::isfinite(a[j]) || !std::isfinite(b[j])) return false;
    const double d = b[j] - a[j];
    if (r.rev[j]) sr += d * d; else sp += d * d;
  }
  const int M = edge_segments(sr, sp, r.step_factor, r.num_traj_segments, r.max_points);
  if (M == 0) return false;
  for (int j = 0; j < NJ; ++j) { e->a[j] = a[j]; e->b[j] = b[j]; }
  e->M = M;
  e->pad = 0;
  return true;
}

std::vector<int> longest_first(const std::vector<EdgeDev>& edges) {
  std::vector<int> order(edges.size());
  for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return edges[x].M > edges[y].M; });
  return order;
}

double dist(const double* a, const double* b) {
  double s = 0.0;
  for (int c = 0; c < NJ; ++c) {
    const double d = b[c] - a[c];
    s += d * d;
  }
  return std::sqrt(s);
}

bool shortcut_edges(const EdgeRule& r, const double* waypoints, int64_t k, int64_t w, std::vector<EdgeDev>* edges) {
  edges->resize((size_t)shortcut_candidates(k, w));
  size_t e = 0;
  for (int64_t j = 1; j < k; ++j)
    for (int64_t i = std::max<int64_t>(0, j - w); i < j; ++i, ++e)
      if (!make_edge(r, waypoints + i * NJ, waypoints + j * NJ, &(*edges)[e])) return false;
  return true;
}

std::vector<EdgeDev> shortcut_route(const double* waypoints, int64_t k, int64_t w, const std::vector<EdgeDev>& edges,
                                    const std::vector<int>& first, smp_shortcut_info* info) {
  *info = smp_shortcut_info{};
  info->n_edges = (int64_t)edges.size();
  std::vector<double> dp((size_t)k, HUGE_VAL);
  std::vector<int64_t> pred((size_t)k, -1), pred_edge((size_t)k, -1);
  dp[0] = 0.0;
  int64_t first_blocked = -1;
  size_t e = 0;
  for (int64_t j = 1; j < k; ++j) {
    info->cost_in += dist(waypoints + (j - 1) * NJ, waypoints + j * NJ);
    for (int64_t i = std::max<int64_t>(0, j - w); i < j; ++i, ++e) {
      const int f = first[e];
      info->configs_checked += f < 0 ? edges[e].M + 1 : f + 1;
      if (f >= 0) {
        if (i == j - 1 && first_blocked < 0) first_blocked = i;
        continue;
      }
      ++info->n_valid;
      const double c = dp[(size_t)i] + dist(waypoints + i * NJ, waypoints + j * NJ);
      if (c < dp[(size_t)j]) { dp[(size_t)j] = c; pred[(size_t)j] = i; pred_edge[(size_t)j] = (int64_t)e; }
    }
  }
  std::vector<EdgeDev> route;
  const bool reached = pred[(size_t)(k - 1)] >= 0;
  info->first_blocked = reached ? -1 : first_blocked;
  info->cost_out = reached ? dp[(size_t)(k - 1)] : 0.0;
  for (int64_t j = k - 1; reached && j > 0; j = pred[(size_t)j]) route.push_back(edges[(size_t)pred_edge[(size_t)j]]);
  std::reverse(route.begin(), route.end());
  return route;
}

std::vector<Gap> find_gaps(const uint8_t* valid, const int* first, int64_t k, int64_t* n_blocked) {
  std::vector<Gap> gaps;
  *n_blocked = 0;
  for (int64_t i = 0; i + 1 < k; ++i) {
    if (first[(size_t)i] < 0) continue;
    ++*n_blocked;
    int64_t l = i, r = i + 1;
    while (!valid[(size_t)l]) --l;  // w_0 and w_k-1 are valid (the precondition)
    while (!valid[(size_t)r]) ++r;
    if (!gaps.empty() && l < gaps.back().r) {
      gaps.back().r = std::max(gaps.back().r, r);
    } else {
      Gap g{};
      g.l = l; g.r = r; g.e = i; g.open = true;
      gaps.push_back(g);
    }
  }
  return gaps;
}

int close_gap(Gap* g, const double* a, const double* b, const DetourDev* items, int samples, int64_t* n_free) {
  double best = HUGE_VAL;
  int chosen = -1;
  for (int s = 0; s < samples; ++s) {
    const DetourDev& it = items[s];
    if (!it.free) continue;
    ++*n_free;
    const double c = dist(a, it.v) + dist(it.v, b);
    if (c < best) { best = c; chosen = s; }
  }
  for (int j = 0; chosen >= 0 && j < NJ; ++j) g->v[j] = items[chosen].v[j];
  g->open = chosen < 0;
  return chosen;
}

bool repaired_route(const EdgeRule& r, const double* waypoints, int64_t k, const std::vector<Gap>& gaps,
                    std::vector<EdgeDev>* route, double* cost) {
  std::vector<const double*> rows;
  size_t g = 0;
  for (int64_t i = 0; i < k;) {
    rows.push_back(waypoints + i * NJ);
    if (g < gaps.size() && gaps[g].l == i) {
      rows.push_back(gaps[g].v);
      i = gaps[g].r;
      ++g;
    } else {
      ++i;
    }
  }
  route->resize(rows.size() - 1);
  *cost = 0.0;
  for (size_t t = 0; t + 1 < rows.size(); ++t) {
    if (!make_edge(r, rows[t], rows[t + 1], &(*route)[t])) return false;
    *cost += dist(rows[t], rows[t + 1]);
  }
  return true;
}

double* route_rows(const std::vector<EdgeDev>& route, int num_traj_segments, int64_t* rows) {
  const int nseg = num_traj_segments;
  int64_t n = 1;
  for (const EdgeDev& ed : route) n += ed.M / nseg;
  double* out = static_cast<double*>(std::malloc((size_t)n * NJ * sizeof(double)));
  if (!out) return nullptr;
  *rows = n;
  int64_t r = 0;
  for (const EdgeDev& ed : route) {
    double step[NJ];
    for (int c = 0; c < NJ; ++c) step[c] = (ed.b[c] - ed.a[c]) / (double)ed.M;
    for (int h = 0; h < ed.M; h += nseg, ++r)  // the edge's start (h = 0), then its via nodes
      for (int c = 0; c < NJ; ++c) out[r * NJ + c] = h == 0 ? ed.a[c] : ed.a[c] + (double)h * step[c];
  }
  for (int c = 0; c < NJ; ++c) out[r * NJ + c] = route.back().b[c];
  return out;
}

double margin_threshold(double r, double m) {
  auto within = [&](double S) {
    const double t = std::sqrt(S);
    return t - r <= m;
  };
  double S = (r + m) * (r + m);
  if (within(S)) {
    for (double up = std::nextafter(S, HUGE_VAL); within(up); up = std::nextafter(S, HUGE_VAL)) S = up;
  } else {
    do S = std::nextafter(S, 0.0); while (!within(S));  // (within(0): -r <= m)
  }
  return S;
}

}  // namespace smp
