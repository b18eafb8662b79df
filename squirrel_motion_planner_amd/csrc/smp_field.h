// The cost field over the base's free map (include/smp_gpu.h "Far goals", smp_base_cost_field): what the
// kernels of smp_field.hip and the host share -- the tile geometry, the round cap, the fallback test -- and the host
// forms of what the small kernels compute from a finished field (parents, chain, settled count).  Everything outside
// the __HIPCC__ part is plain C++17 that tests/cpp/field_table.cpp builds without HIP.
//
// The field.  cost[src] = 0, cost[v] = min over the neighbours u of v in smp_base_route's graph of fl(cost[u] + w(u, v)),
// +inf for blocked and unreachable nodes.  While every step weight exceeds half an ulp of the largest finite cost
// (field_unique) the system has one solution, the bits smp_base_route's Dijkstra produces, and any relaxation order that
// only lowers values from +inf reaches it.
#pragma once
#include <cstdint>
#include <vector>

#include "smp_route.h"

namespace smp {

// A tile owns FIELD_BX x FIELD_BY x FIELD_BT nodes (fewer at the lattice's far ends).  Its halo is one node wide: the
// eight (dx, dy) directions within a heading layer, and the layers below and above at the tile's own (ix, iy).
constexpr int FIELD_BX = 16, FIELD_BY = 16, FIELD_BT = 8;
constexpr int FIELD_THREADS = FIELD_BX * FIELD_BY;  // one thread per (ix, iy) column of a tile
constexpr int FIELD_SWEEPS = 96;                    // local sweeps of one tile run at the most
constexpr int FIELD_DIRS = 10;                      // directions a tile has neighbours in: 8 in the layer, t - 1, t + 1

// The lattice as the field's kernels see it: the counts, the tile counts and the weights (route_weights).
struct FieldGrid {
  int nx, ny, nt;
  int wrap;        // 1: headings 0 and nt - 1 are neighbours (wrap_theta and nt > 1)
  int tx, ty, tz;  // tiles per axis
  double w_axis, w_diag, w_turn;
};

inline FieldGrid field_grid(const RouteLattice& L) {
  const RouteWeights w = route_weights(L.d);
  FieldGrid g;
  g.nx = L.nx;
  g.ny = L.ny;
  g.nt = L.nt;
  g.wrap = (L.wrap && L.nt > 1) ? 1 : 0;
  g.tx = (L.nx + FIELD_BX - 1) / FIELD_BX;
  g.ty = (L.ny + FIELD_BY - 1) / FIELD_BY;
  g.tz = (L.nt + FIELD_BT - 1) / FIELD_BT;
  g.w_axis = w.axis;
  g.w_diag = w.diag;
  g.w_turn = w.turn;
  return g;
}

SMP_HD long long field_n_tiles(const FieldGrid& g) { return (long long)g.tx * g.ty * g.tz; }
SMP_HD long long field_node(const FieldGrid& g, int ix, int iy, int t) { return ((long long)t * g.ny + iy) * g.nx + ix; }
SMP_HD int field_tile_id(const FieldGrid& g, int a, int b, int c) { return (c * g.ty + b) * g.tx + a; }
SMP_HD int field_tile_of(const FieldGrid& g, int ix, int iy, int t) {
  return field_tile_id(g, ix / FIELD_BX, iy / FIELD_BY, t / FIELD_BT);
}
// Tile (a, b, c): its first node lo[] and its extent ext[] (ix, iy, t).
SMP_HD void field_tile_range(const FieldGrid& g, int a, int b, int c, int lo[3], int ext[3]) {
  lo[0] = a * FIELD_BX;
  lo[1] = b * FIELD_BY;
  lo[2] = c * FIELD_BT;
  ext[0] = g.nx - lo[0] < FIELD_BX ? g.nx - lo[0] : FIELD_BX;
  ext[1] = g.ny - lo[1] < FIELD_BY ? g.ny - lo[1] : FIELD_BY;
  ext[2] = g.nt - lo[2] < FIELD_BT ? g.nt - lo[2] : FIELD_BT;
}
// A tile whose headings are the whole circle wraps inside itself: it has no halo in t.
SMP_HD bool field_wraps_inside(const FieldGrid& g) { return g.wrap && g.tz == 1; }

// Direction d of FIELD_DIRS: 0..7 are (dx, dy) = (-1,-1), (0,-1), (1,-1), (-1,0), (1,0), (-1,1), (0,1), (1,1); 8 is
// t - 1 and 9 is t + 1.
SMP_HD void field_dir(int d, int* dx, int* dy, int* dt) {
  const int k = d < 4 ? d : d + 1;  // (skips the centre of the 3 x 3)
  *dx = d < 8 ? k % 3 - 1 : 0;
  *dy = d < 8 ? k / 3 - 1 : 0;
  *dt = d == 8 ? -1 : d == 9 ? 1 : 0;
}
// The directions in which the node at (lx, ly, lt) of a tile of extent ext[] lies in a neighbour's halo, as a mask.
SMP_HD unsigned field_dir_mask(const int ext[3], int lx, int ly, int lt) {
  unsigned m = 0;
  for (int d = 0; d < 8; ++d) {
    int dx, dy, dt;
    field_dir(d, &dx, &dy, &dt);
    const bool x = dx == 0 || (dx < 0 ? lx == 0 : lx == ext[0] - 1);
    const bool y = dy == 0 || (dy < 0 ? ly == 0 : ly == ext[1] - 1);
    if (x && y) m |= 1u << d;
  }
  if (lt == 0) m |= 1u << 8;
  if (lt == ext[2] - 1) m |= 1u << 9;
  return m;
}
// The tile in direction d of tile (a, b, c), -1 where there is none.
SMP_HD int field_dir_tile(const FieldGrid& g, int a, int b, int c, int d) {
  int dx, dy, dt;
  field_dir(d, &dx, &dy, &dt);
  a += dx;
  b += dy;
  c += dt;
  if (dt != 0) {
    if (field_wraps_inside(g)) return -1;
    if (g.wrap) c = (c + g.tz) % g.tz;
  }
  if (a < 0 || a >= g.tx || b < 0 || b >= g.ty || c < 0 || c >= g.tz) return -1;
  return field_tile_id(g, a, b, c);
}

// Whether `tile` runs in round 0 for the source (ix, iy, t): the source's own tile, and every tile whose halo holds the
// source.  The source is never lowered, so no tile run would ever flag those neighbours for it: a source on a tile's rim
// whose only free neighbours lie in the next tile reaches them only this way.
SMP_HD bool field_starts_active(const FieldGrid& g, int ix, int iy, int t, long long tile) {
  const int a = ix / FIELD_BX, b = iy / FIELD_BY, c = t / FIELD_BT;
  if (tile == field_tile_id(g, a, b, c)) return true;
  int lo[3], ext[3];
  field_tile_range(g, a, b, c, lo, ext);
  const unsigned m = field_dir_mask(ext, ix - lo[0], iy - lo[1], t - lo[2]);
  for (int d = 0; d < FIELD_DIRS; ++d)
    if (((m >> d) & 1u) && tile == field_dir_tile(g, a, b, c, d)) return true;
  return false;
}

// The parent rule on node (ix, iy, t), host and device alike: free_at(ix, iy, t) answers in-range nodes, cost_at(n) a
// node's cost.  -1 for the source (cost 0) and for +inf nodes, else the neighbour u with fl(cost[u] + w) == cost[n] and
// the least (cost[u], u); -1 too where no neighbour qualifies (never on a fixed point).
template <typename Free, typename Cost>
SMP_HD long long field_parent_rule(const FieldGrid& g, Free&& free_at, Cost&& cost_at, int ix, int iy, int t) {
  const double c = cost_at(field_node(g, ix, iy, t));
  if (!(c > 0.0) || c == __builtin_inf()) return -1;
  long long best = -1;
  double best_c = 0.0;
  auto cand = [&](int x, int y, int z, double w) {
    const long long u = field_node(g, x, y, z);
    const double cu = cost_at(u);
    if (cu + w != c) return;
    if (best < 0 || cu < best_c || (cu == best_c && u < best)) {
      best = u;
      best_c = cu;
    }
  };
  auto in = [&](int x, int y) { return x >= 0 && x < g.nx && y >= 0 && y < g.ny && free_at(x, y, t); };
  for (int d = 0; d < 8; ++d) {
    int dx, dy, dt;
    field_dir(d, &dx, &dy, &dt);
    const int x = ix + dx, y = iy + dy;
    if (!in(x, y)) continue;
    if (dx != 0 && dy != 0) {
      if (in(x, iy) && in(ix, y)) cand(x, y, t, g.w_diag);
    } else {
      cand(x, y, t, g.w_axis);
    }
  }
  for (int s = -1; s <= 1; s += 2) {
    int z = t + s;
    if (g.wrap) z = (z + g.nt) % g.nt;
    if (z >= 0 && z < g.nt && free_at(ix, iy, z)) cand(ix, iy, z, g.w_turn);
  }
  return best;
}

// The tiles a change of node (ix, iy, t) activates: those whose halo holds it, ascending, each once.
std::vector<int> field_activates(const FieldGrid& g, int ix, int iy, int t);

// The host's round loop gives up after this many rounds: every round with work in it finalises at least one more node.
inline int64_t field_round_cap(int64_t n_free) { return n_free + 1; }

// Whether the uniqueness argument holds for a field whose largest finite cost is cost_max: the least weight still moves
// it.  False: the call falls back to smp_base_route.
inline bool field_unique(double cost_max, const FieldGrid& g) {
  double w = g.w_axis;  // (w_diag > w_axis)
  if (g.nt > 1 && g.w_turn < w) w = g.w_turn;
  return cost_max + w != cost_max;
}

// The parent of node n in a finished field: -1 for the source (cost 0) and for +inf nodes, else the neighbour u with
// fl(cost[u] + w(u, n)) == cost[n] and the least (cost[u], u).
int32_t field_parent(const RouteLattice& L, const FieldGrid& g, const double* cost, int64_t n);
// The chain from -> to through field_parent, start first, (ix, iy, t) per node; empty where to is not reached.
std::vector<int32_t> field_chain(const RouteLattice& L, const FieldGrid& g, const double* cost, int64_t from, int64_t to);
// smp_base_route's n_settled: the reachable nodes with (cost[n], n) <= (cost[to], to), or all of them when to is not
// reached; *n_reached = the reachable nodes, the source included.
int64_t field_settled(const double* cost, int64_t n_nodes, int64_t to, int64_t* n_reached);

#if defined(__HIPCC__)

// What a route call brings back from the device besides the chain.
struct FieldStats {
  unsigned long long n_reached, n_settled;
  unsigned long long max_bits;  // the largest finite cost's bits (costs are >= 0: their bits order as they do)
  double cost_to;
  int n_chain;  // nodes of the walked chain; 0: to is not reached; -1: the walk left the field (never on a fixed point)
  int pad;
};

// The launches of smp_field.hip, all on stream st.
//   init:    cost = +inf but 0 at src, the activity flags cleared but field_starts_active's set for round 0, stats cleared;
//   round:   one workgroup per tile; a tile whose flag of this round's parity is set relaxes in LDS, stores what it
//            lowered, sets the next round's flags and adds 1 to changed[slot] if it lowered anything;
//   stats:   n_reached, max_bits, cost_to and n_settled for node `to` (to < 0: none);
//   parents: parent[n] by field_parent's rule;
//   chain:   one wave walks to -> from through parent[], nodes into chain[] (to first), the count into stats.
void launch_field_init(hipStream_t st, FieldGrid g, long long src, double* cost, unsigned* active, FieldStats* stats);
void launch_field_round(hipStream_t st, FieldGrid g, const uint32_t* bits, double* cost, unsigned* active, int parity,
                        unsigned* changed);
void launch_field_stats(hipStream_t st, FieldGrid g, const double* cost, long long to, FieldStats* stats);
void launch_field_parents(hipStream_t st, FieldGrid g, const uint32_t* bits, const double* cost, int32_t* parent);
void launch_field_chain(hipStream_t st, FieldGrid g, const int32_t* parent, long long from, long long to, int32_t* chain,
                        FieldStats* stats);
size_t field_kernels_private_bytes();

#endif  // __HIPCC__

}  // namespace smp
