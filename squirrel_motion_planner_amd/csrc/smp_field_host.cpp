// Reference forms, built by the CPU tests only (not part of libsmp_gpu.so).
// Host forms of the cost field's small steps (smp_field.h): which tiles a change activates, and the
// parents, the chain and the settled count of a finished field.  Plain sequential C++: the device kernels of
// smp_field.hip compute the same from the same rules, and tests/cpp/field_table.cpp pins these against a restatement.
#include "smp_field.h"

#include <algorithm>
#include <cmath>

namespace smp {

std::vector<int> field_activates(const FieldGrid& g, int ix, int iy, int t) {
  const int a = ix / FIELD_BX, b = iy / FIELD_BY, c = t / FIELD_BT;
  int lo[3], ext[3];
  field_tile_range(g, a, b, c, lo, ext);
  const unsigned m = field_dir_mask(ext, ix - lo[0], iy - lo[1], t - lo[2]);
  std::vector<int> out;
  for (int d = 0; d < FIELD_DIRS; ++d) {
    if (!((m >> d) & 1u)) continue;
    const int tile = field_dir_tile(g, a, b, c, d);
    if (tile >= 0 && tile != field_tile_id(g, a, b, c)) out.push_back(tile);
  }
  std::sort(out.begin(), out.end());
  out.erase(std::unique(out.begin(), out.end()), out.end());
  return out;
}

int32_t field_parent(const RouteLattice& L, const FieldGrid& g, const double* cost, int64_t n) {
  const int64_t layer = (int64_t)g.nx * g.ny;
  const int t = (int)(n / layer), iy = (int)((n - (int64_t)t * layer) / g.nx), ix = (int)(n % g.nx);
  return (int32_t)field_parent_rule(
      g, [&](int x, int y, int z) { return lattice_free(L.bits, L.node(x, y, z)); },
      [&](long long u) { return cost[u]; }, ix, iy, t);
}

std::vector<int32_t> field_chain(const RouteLattice& L, const FieldGrid& g, const double* cost, int64_t from, int64_t to) {
  std::vector<int32_t> chain;
  if (!std::isfinite(cost[to])) return chain;
  const int64_t layer = (int64_t)g.nx * g.ny, n_nodes = layer * g.nt;
  int64_t v = to;
  for (int64_t k = 0; k <= n_nodes; ++k) {  // (a chain visits a node once)
    const int t = (int)(v / layer);
    chain.push_back(t);
    chain.push_back((int32_t)((v - (int64_t)t * layer) / g.nx));
    chain.push_back((int32_t)(v % g.nx));
    if (v == from) break;
    v = field_parent(L, g, cost, v);
    if (v < 0) return std::vector<int32_t>();
  }
  if (v != from) return std::vector<int32_t>();
  // (collected goal first as t, iy, ix: reversed it is start first, ix, iy, t)
  std::reverse(chain.begin(), chain.end());
  return chain;
}

int64_t field_settled(const double* cost, int64_t n_nodes, int64_t to, int64_t* n_reached) {
  int64_t reached = 0, settled = 0;
  const double ct = cost[to];
  for (int64_t n = 0; n < n_nodes; ++n) {
    if (!std::isfinite(cost[n])) continue;
    ++reached;
    if (cost[n] < ct || (cost[n] == ct && n <= to)) ++settled;
  }
  if (n_reached) *n_reached = reached;
  return std::isfinite(ct) ? settled : reached;
}

}  // namespace smp
