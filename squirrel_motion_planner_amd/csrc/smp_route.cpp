// The route search over the base's free map and the rest of the far-goal stage's host logic (smp_route.h;
// include/smp_gpu.h "Far goals").  Small, sequential work: a Dijkstra over the bit grid with a fixed tie order, so a
// heapq restatement (tests/lattice_restatement.py) reproduces chain, rows and cost bit for bit.
#include "smp_route.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <queue>
#include <utility>

namespace smp {

int lattice_dev(const smp_base_lattice* lat, LatticeDev* d) {
  if (!lat || !d) return SMP_ERR_ARG;
  const double f[5] = {lat->x0, lat->y0, lat->pitch, lat->theta0, lat->dtheta};
  for (double v : f)
    if (!std::isfinite(v)) return SMP_ERR_ARG;
  for (double v : lat->arm)
    if (!std::isfinite(v)) return SMP_ERR_ARG;
  if (!(lat->pitch > 0.0) || lat->nx < 1 || lat->ny < 1 || lat->n_theta < 1) return SMP_ERR_ARG;
  // (each factor is below 2^31: the product of two fits an int64, and the third is compared by division)
  const int64_t layer = (int64_t)lat->nx * lat->ny;
  if (layer > SMP_LATTICE_MAX_NODES || lat->n_theta > SMP_LATTICE_MAX_NODES / layer) return SMP_ERR_CAPACITY;
  d->x0 = lat->x0;
  d->y0 = lat->y0;
  d->pitch = lat->pitch;
  d->theta0 = lat->theta0;
  d->dtheta = lat->dtheta;
  for (int j = 0; j < NJ - 3; ++j) d->arm[j] = lat->arm[j];
  d->nx = lat->nx;
  d->ny = lat->ny;
  d->n = layer * lat->n_theta;
  return SMP_OK;
}

static bool same_step(const int32_t* a, const int32_t* b, const int32_t* c) {
  return b[0] - a[0] == c[0] - b[0] && b[1] - a[1] == c[1] - b[1] && b[2] - a[2] == c[2] - b[2];
}

std::vector<double> chain_rows(const LatticeDev& lat, const int32_t* chain, int64_t n) {
  std::vector<double> rows;
  for (int64_t i = 0; i < n; ++i) {
    const int32_t* c = chain + 3 * i;
    if (i > 0 && i + 1 < n && same_step(c - 3, c, c + 3)) continue;
    for (int j = 0; j < NJ; ++j) rows.push_back(lattice_coord(lat, c[0], c[1], c[2], j));
  }
  return rows;
}

int64_t handover_index(const LatticeDev& lat, const int32_t* chain, int64_t n, double distance) {
  const double diag = std::sqrt(lat.pitch * lat.pitch + lat.pitch * lat.pitch);
  double acc = 0.0;
  int64_t j = n - 1;
  while (j > 0 && acc < distance) {
    const int32_t *a = chain + 3 * j, *b = a - 3;
    const int moved = (a[0] != b[0]) + (a[1] != b[1]);
    acc += moved == 2 ? diag : moved == 1 ? lat.pitch : 0.0;
    --j;
  }
  return j;
}

namespace {

// floor(v + 0.5) as an index, false where it is not finite or does not fit an int.
bool round_index(double v, int64_t* out) {
  const double f = std::floor(v + 0.5);
  if (!std::isfinite(f) || f < -2147483648.0 || f > 2147483647.0) return false;
  *out = (int64_t)f;
  return true;
}

// The node (x, y, theta) snaps to: SMP_ERR_ARG outside the lattice, `blocked` where no free node is found within
// snap_cells rings of the same heading layer.
int snap(const RouteLattice& L, const double p[3], int snap_cells, int blocked, int32_t node[3]) {
  if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) return SMP_ERR_ARG;
  int64_t ix, iy, t;
  if (!round_index((p[0] - L.d.x0) / L.d.pitch, &ix) || !round_index((p[1] - L.d.y0) / L.d.pitch, &iy) ||
      !round_index((p[2] - L.d.theta0) / L.d.dtheta, &t))
    return SMP_ERR_ARG;
  if (L.wrap) t = ((t % L.nt) + L.nt) % L.nt;
  if (ix < 0 || ix >= L.nx || iy < 0 || iy >= L.ny || t < 0 || t >= L.nt) return SMP_ERR_ARG;
  const int x0 = (int)ix, y0 = (int)iy;
  node[2] = (int32_t)t;
  if (L.free_at(x0, y0, (int)t)) {
    node[0] = x0;
    node[1] = y0;
    return SMP_OK;
  }
  const int r_max = std::min(snap_cells, std::max(L.nx, L.ny));  // (wider rings hold no node)
  for (int r = 1; r <= r_max; ++r) {
    int64_t best_d = -1;
    // (y ascending, then x ascending: node numbers ascend within a layer, so the first least distance is the tie's)
    for (int y = std::max(y0 - r, 0); y <= std::min((int64_t)y0 + r, (int64_t)L.ny - 1); ++y)
      for (int x = std::max(x0 - r, 0); x <= std::min((int64_t)x0 + r, (int64_t)L.nx - 1); ++x) {
        if (std::max(std::abs(x - x0), std::abs(y - y0)) != r || !L.free_at(x, y, (int)t)) continue;
        const int64_t d = (int64_t)(x - x0) * (x - x0) + (int64_t)(y - y0) * (y - y0);
        if (best_d < 0 || d < best_d) {
          best_d = d;
          node[0] = x;
          node[1] = y;
        }
      }
    if (best_d >= 0) return SMP_OK;
  }
  return blocked;
}

}  // namespace

RouteWeights route_weights(const LatticeDev& d) {
  return RouteWeights{d.pitch, std::sqrt(d.pitch * d.pitch + d.pitch * d.pitch), std::fabs(d.dtheta)};
}

int route_lattice(const smp_base_lattice* lat, const uint32_t* free_bits, RouteLattice* L) {
  if (int st = lattice_dev(lat, &L->d)) return st;
  L->nx = lat->nx;
  L->ny = lat->ny;
  L->nt = lat->n_theta;
  L->wrap = lat->wrap_theta ? 1 : 0;
  L->bits = free_bits;
  return SMP_OK;
}

int route_ends(const RouteLattice& L, const double from[3], const double to[3], int snap_cells, smp_route_info* r) {
  int st = snap(L, from, snap_cells, SMP_ERR_START_INVALID, r->from_node);
  if (st != SMP_OK) {
    for (int k = 0; k < 3; ++k) r->from_node[k] = -1;
    return st;
  }
  st = snap(L, to, snap_cells, SMP_ERR_GOAL_INVALID, r->to_node);
  if (st != SMP_OK)
    for (int k = 0; k < 3; ++k) r->to_node[k] = -1;
  return st;
}

bool route_search(const RouteLattice& L, int64_t src, int64_t dst, std::vector<double>* dp_out,
                  std::vector<int32_t>* parent_out, int64_t* n_settled) {
  *n_settled = 0;
  const int64_t N = L.d.n, layer = (int64_t)L.nx * L.ny;
  const RouteWeights w = route_weights(L.d);
  const double w_axis = w.axis, w_diag = w.diag, w_turn = w.turn;
  std::vector<double>& dp = *dp_out;
  std::vector<int32_t>& parent = *parent_out;
  dp.assign((size_t)N, std::numeric_limits<double>::infinity());
  parent.assign((size_t)N, -1);
  std::vector<bool> settled((size_t)N, false);
  typedef std::pair<double, int64_t> Item;
  std::priority_queue<Item, std::vector<Item>, std::greater<Item>> heap;
  dp[(size_t)src] = 0.0;
  heap.push(Item(0.0, src));
  static const int AX[4][2] = {{0, -1}, {-1, 0}, {1, 0}, {0, 1}};
  static const int DG[4][2] = {{-1, -1}, {1, -1}, {-1, 1}, {1, 1}};
  bool found = false;
  while (!heap.empty()) {
    const int64_t u = heap.top().second;
    heap.pop();
    if (settled[(size_t)u]) continue;
    settled[(size_t)u] = true;
    ++*n_settled;
    if (u == dst) {
      found = true;
      break;
    }
    const int t = (int)(u / layer), iy = (int)((u - (int64_t)t * layer) / L.nx), ix = (int)(u % L.nx);
    const double du = dp[(size_t)u];
    auto relax = [&](int64_t v, double w) {
      const double c = du + w;
      if (c < dp[(size_t)v]) {
        dp[(size_t)v] = c;
        parent[(size_t)v] = (int32_t)u;
        heap.push(Item(c, v));
      }
    };
    for (const auto& a : AX)
      if (L.free_at(ix + a[0], iy + a[1], t)) relax(L.node(ix + a[0], iy + a[1], t), w_axis);
    for (const auto& g : DG)
      if (L.free_at(ix + g[0], iy + g[1], t) && L.free_at(ix + g[0], iy, t) && L.free_at(ix, iy + g[1], t))
        relax(L.node(ix + g[0], iy + g[1], t), w_diag);
    for (int s = -1; s <= 1; s += 2) {
      int tt = t + s;
      if (L.wrap) tt = (tt + L.nt) % L.nt;
      if (tt >= 0 && tt < L.nt && L.free_at(ix, iy, tt)) relax(L.node(ix, iy, tt), w_turn);
    }
  }
  return found;
}

int route_output(const RouteLattice& L, const std::vector<int32_t>& chain, double** out_rows, int64_t* n_out,
                 int32_t** out_chain) {
  const std::vector<double> rows = chain_rows(L.d, chain.data(), (int64_t)(chain.size() / 3));
  double* rbuf = (double*)std::malloc(rows.size() * sizeof(double));
  int32_t* cbuf = out_chain ? (int32_t*)std::malloc(chain.size() * sizeof(int32_t)) : nullptr;
  if (!rbuf || (out_chain && !cbuf)) {
    std::free(rbuf);
    std::free(cbuf);
    return SMP_ERR_CAPACITY;
  }
  std::memcpy(rbuf, rows.data(), rows.size() * sizeof(double));
  *out_rows = rbuf;
  *n_out = (int64_t)(rows.size() / NJ);
  if (out_chain) {
    std::memcpy(cbuf, chain.data(), chain.size() * sizeof(int32_t));
    *out_chain = cbuf;
  }
  return SMP_OK;
}

}  // namespace smp

using namespace smp;

extern "C" int smp_base_lattice_fit(const double env_x[2], const double env_y[2], double pitch, int n_theta,
                                    double theta0, const double arm[5], smp_base_lattice* out) {
  if (!env_x || !env_y || !arm || !out) return SMP_ERR_ARG;
  if (!std::isfinite(pitch) || !(pitch > 0.0) || n_theta < 1 || !std::isfinite(theta0)) return SMP_ERR_ARG;
  const double cx = std::floor((env_x[1] - env_x[0]) / pitch), cy = std::floor((env_y[1] - env_y[0]) / pitch);
  if (!std::isfinite(env_x[0]) || !std::isfinite(env_y[0]) || !std::isfinite(cx) || !std::isfinite(cy) || cx < 0.0 ||
      cy < 0.0)
    return SMP_ERR_ARG;
  if (cx >= (double)SMP_LATTICE_MAX_NODES || cy >= (double)SMP_LATTICE_MAX_NODES) return SMP_ERR_CAPACITY;
  smp_base_lattice l;
  std::memset(&l, 0, sizeof(l));
  l.x0 = env_x[0];
  l.y0 = env_y[0];
  l.pitch = pitch;
  l.nx = (int)cx + 1;
  l.ny = (int)cy + 1;
  l.theta0 = theta0;
  l.dtheta = (2.0 * M_PI) / n_theta;
  l.n_theta = n_theta;
  l.wrap_theta = 1;
  for (int j = 0; j < 5; ++j) l.arm[j] = arm[j];
  LatticeDev d;
  if (int st = lattice_dev(&l, &d)) return st;
  *out = l;
  return SMP_OK;
}

extern "C" int smp_base_route(const smp_base_lattice* lat, const uint32_t* free_bits, const double from[3],
                              const double to[3], int snap_cells, double** out_rows, int64_t* n_out,
                              int32_t** out_chain, smp_route_info* info) {
  if (out_rows) *out_rows = nullptr;
  if (n_out) *n_out = 0;
  if (out_chain) *out_chain = nullptr;
  smp_route_info r;
  std::memset(&r, 0, sizeof(r));
  for (int k = 0; k < 3; ++k) r.from_node[k] = r.to_node[k] = -1;
  if (info) *info = r;
  if (!lat || !free_bits || !from || !to || !out_rows || !n_out) return SMP_ERR_ARG;
  RouteLattice L;
  if (int st = route_lattice(lat, free_bits, &L)) return st;
  if (int st = route_ends(L, from, to, snap_cells, &r)) {
    if (info) *info = r;
    return st;
  }
  const int64_t layer = (int64_t)L.nx * L.ny;
  const int64_t src = L.node(r.from_node[0], r.from_node[1], r.from_node[2]);
  const int64_t dst = L.node(r.to_node[0], r.to_node[1], r.to_node[2]);
  std::vector<double> dp;
  std::vector<int32_t> parent;
  const bool found = route_search(L, src, dst, &dp, &parent, &r.n_settled);
  if (!found) {
    if (info) *info = r;
    return SMP_ERR_NO_SOLUTION;
  }
  r.cost = dp[(size_t)dst];
  std::vector<int32_t> chain;
  for (int64_t v = dst;; v = parent[(size_t)v]) {
    const int t = (int)(v / layer);
    chain.push_back(t);
    chain.push_back((int32_t)((v - (int64_t)t * layer) / L.nx));
    chain.push_back((int32_t)(v % L.nx));
    if (v == src) break;
  }
  // (collected goal first as t, iy, ix: reversed it is start first, ix, iy, t)
  for (size_t a = 0, b = chain.size() - 1; a < b; ++a, --b) std::swap(chain[a], chain[b]);
  r.n_chain = (int64_t)(chain.size() / 3);
  const int os = route_output(L, chain, out_rows, n_out, out_chain);
  if (info) *info = r;
  return os;
}
