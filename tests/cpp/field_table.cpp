// Driver of the cost field's host unit (csrc/smp_field.h, smp_field_host.cpp: the tile geometry, the round cap, the
// fallback test, field_parent / field_chain / field_settled), built with ASAN / UBSAN by tests/test_field_cpu.py.
// stdin holds cases, doubles as hex floats:
//   G nx ny n_theta wrap_theta
//     -> "n_tiles", a line "lo0 lo1 lo2 ext0 ext1 ext2" per tile, then per node ascending "tile k a_1 .. a_k": its tile
//        and the tiles a change of it activates
//   S nx ny n_theta wrap_theta ix iy t -> "k a_1 .. a_k": the tiles that run in round 0 for that source, ascending
//   U cost_max pitch dtheta n_theta -> "unique"          K n_free -> "cap"
//   C x0 y0 pitch nx ny theta0 dtheta n_theta wrap_theta a0..a4  fx fy ft  tx ty tt  snap_cells  n_words w_0 ..
//     then N costs
//     -> "status same n_settled_route n_settled_field n_reached cost n_chain", n_chain lines "ix iy t" (field_chain's),
//        then the N parents of field_parent; status is smp_base_route's on the same input and `same` is 1 iff
//        field_chain's chain equals its chain and cost[to] its cost bit for bit (-1 where the route failed).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../squirrel_motion_planner_amd/csrc/smp_field.h"

using namespace smp;

static bool rd(double* v) { return std::scanf("%la", v) == 1; }

int main() {
  char kind;
  while (std::scanf(" %c", &kind) == 1) {
    if (kind == 'G') {
      RouteLattice L{};
      if (std::scanf("%d %d %d %d", &L.nx, &L.ny, &L.nt, &L.wrap) != 4) return 2;
      L.d.pitch = 0.25;
      L.d.dtheta = 0.5;
      const FieldGrid g = field_grid(L);
      std::printf("%lld\n", field_n_tiles(g));
      for (int c = 0; c < g.tz; ++c)
        for (int b = 0; b < g.ty; ++b)
          for (int a = 0; a < g.tx; ++a) {
            int lo[3], ext[3];
            field_tile_range(g, a, b, c, lo, ext);
            std::printf("%d %d %d %d %d %d\n", lo[0], lo[1], lo[2], ext[0], ext[1], ext[2]);
          }
      for (int t = 0; t < L.nt; ++t)
        for (int y = 0; y < L.ny; ++y)
          for (int x = 0; x < L.nx; ++x) {
            const std::vector<int> act = field_activates(g, x, y, t);
            std::printf("%d %zu", field_tile_of(g, x, y, t), act.size());
            for (int v : act) std::printf(" %d", v);
            std::printf("\n");
          }
      continue;
    }
    if (kind == 'S') {
      RouteLattice L{};
      int ix, iy, t;
      if (std::scanf("%d %d %d %d %d %d %d", &L.nx, &L.ny, &L.nt, &L.wrap, &ix, &iy, &t) != 7) return 2;
      L.d.pitch = 0.25;
      L.d.dtheta = 0.5;
      const FieldGrid g = field_grid(L);
      std::vector<long long> on;
      for (long long tile = 0; tile < field_n_tiles(g); ++tile)
        if (field_starts_active(g, ix, iy, t, tile)) on.push_back(tile);
      std::printf("%zu", on.size());
      for (long long v : on) std::printf(" %lld", v);
      std::printf("\n");
      continue;
    }
    if (kind == 'U') {
      RouteLattice L{};
      double cost_max;
      if (!rd(&cost_max) || !rd(&L.d.pitch) || !rd(&L.d.dtheta) || std::scanf("%d", &L.nt) != 1) return 2;
      L.nx = L.ny = 1;
      std::printf("%d\n", field_unique(cost_max, field_grid(L)) ? 1 : 0);
      continue;
    }
    if (kind == 'K') {
      long long n_free;
      if (std::scanf("%lld", &n_free) != 1) return 2;
      std::printf("%lld\n", (long long)field_round_cap(n_free));
      continue;
    }
    if (kind != 'C') return 2;
    smp_base_lattice l{};
    double from[3], to[3];
    int snap_cells;
    long long n_words;
    if (!rd(&l.x0) || !rd(&l.y0) || !rd(&l.pitch) || std::scanf("%d %d", &l.nx, &l.ny) != 2 || !rd(&l.theta0) ||
        !rd(&l.dtheta) || std::scanf("%d %d", &l.n_theta, &l.wrap_theta) != 2)
      return 2;
    for (double& a : l.arm)
      if (!rd(&a)) return 2;
    for (double& v : from)
      if (!rd(&v)) return 2;
    for (double& v : to)
      if (!rd(&v)) return 2;
    if (std::scanf("%d %lld", &snap_cells, &n_words) != 2) return 2;
    std::vector<uint32_t> bits((size_t)n_words);  // (exactly the words of the lattice: a read past them is ASAN's)
    for (uint32_t& w : bits)
      if (std::scanf("%u", &w) != 1) return 2;
    RouteLattice L;
    if (route_lattice(&l, bits.data(), &L) != SMP_OK) return 2;
    std::vector<double> cost((size_t)L.d.n);
    for (double& v : cost)
      if (!rd(&v)) return 2;
    double* rows = nullptr;
    int64_t n_out = 0;
    int32_t* chain = nullptr;
    smp_route_info info;
    const int st = smp_base_route(&l, bits.data(), from, to, snap_cells, &rows, &n_out, &chain, &info);
    if (info.from_node[0] < 0 || info.to_node[0] < 0) return 2;  // (the cases' ends snap)
    const FieldGrid g = field_grid(L);
    const int64_t src = L.node(info.from_node[0], info.from_node[1], info.from_node[2]);
    const int64_t dst = L.node(info.to_node[0], info.to_node[1], info.to_node[2]);
    const std::vector<int32_t> fc = field_chain(L, g, cost.data(), src, dst);
    int64_t n_reached = 0;
    const int64_t n_settled = field_settled(cost.data(), L.d.n, dst, &n_reached);
    int same = -1;
    if (st == SMP_OK)
      same = (int64_t)fc.size() == 3 * info.n_chain && std::memcmp(fc.data(), chain, fc.size() * sizeof(int32_t)) == 0 &&
             std::memcmp(&cost[(size_t)dst], &info.cost, sizeof(double)) == 0;
    std::printf("%d %d %lld %lld %lld %a %zu\n", st, same, (long long)info.n_settled, (long long)n_settled,
                (long long)n_reached, cost[(size_t)dst], fc.size() / 3);
    for (size_t i = 0; i < fc.size(); i += 3) std::printf("%d %d %d\n", fc[i], fc[i + 1], fc[i + 2]);
    for (int64_t n = 0; n < L.d.n; ++n) std::printf("%d\n", field_parent(L, g, cost.data(), n));
    std::free(rows);
    std::free(chain);
  }
  return 0;
}
