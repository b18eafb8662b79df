// Driver of the far-goal stage's host logic (csrc/smp_route.cpp: smp_base_lattice_fit, smp_base_route, handover_index),
// built with ASAN / UBSAN by tests/test_lattice_cpu.py.  stdin holds cases, doubles as hex floats:
//   F ex0 ex1 ey0 ey1 pitch n_theta theta0 a0..a4
//     -> "status x0 y0 pitch nx ny theta0 dtheta n_theta wrap_theta"
//   R x0 y0 pitch nx ny theta0 dtheta n_theta wrap_theta a0..a4  fx fy ft  tx ty tt  snap_cells want_chain handover
//     n_words w_0 .. w_n-1
//     -> "status fx fy ft tx ty tt n_chain n_settled cost n_out j", then n_chain lines "ix iy t" (want_chain = 1) and
//        n_out lines of 8 doubles; j = handover_index of the chain at `handover` (-1 without a chain).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../squirrel_motion_planner_amd/csrc/smp_route.h"

static bool rd(double* v) { return std::scanf("%la", v) == 1; }

int main() {
  char kind;
  while (std::scanf(" %c", &kind) == 1) {
    if (kind == 'F') {
      double ex[2], ey[2], pitch, theta0, arm[5];
      int n_theta;
      if (!rd(&ex[0]) || !rd(&ex[1]) || !rd(&ey[0]) || !rd(&ey[1]) || !rd(&pitch) || std::scanf("%d", &n_theta) != 1 ||
          !rd(&theta0))
        return 2;
      for (double& a : arm)
        if (!rd(&a)) return 2;
      smp_base_lattice l{};
      const int st = smp_base_lattice_fit(ex, ey, pitch, n_theta, theta0, arm, &l);
      std::printf("%d %a %a %a %d %d %a %a %d %d\n", st, l.x0, l.y0, l.pitch, l.nx, l.ny, l.theta0, l.dtheta, l.n_theta,
                  l.wrap_theta);
      continue;
    }
    if (kind != 'R') return 2;
    smp_base_lattice l{};
    double from[3], to[3], handover;
    int snap_cells, want_chain;
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
    if (std::scanf("%d %d", &snap_cells, &want_chain) != 2 || !rd(&handover) || std::scanf("%lld", &n_words) != 1) return 2;
    std::vector<uint32_t> bits((size_t)n_words);  // (exactly the words of the lattice: a read past them is ASAN's)
    for (uint32_t& w : bits)
      if (std::scanf("%u", &w) != 1) return 2;
    double* rows = nullptr;
    int64_t n_out = 0;
    int32_t* chain = nullptr;
    smp_route_info info;
    const int st = smp_base_route(&l, bits.data(), from, to, snap_cells, &rows, &n_out, want_chain ? &chain : nullptr, &info);
    long long j = -1;
    smp::LatticeDev d;
    if (st == SMP_OK && chain && smp::lattice_dev(&l, &d) == SMP_OK) j = smp::handover_index(d, chain, info.n_chain, handover);
    std::printf("%d %d %d %d %d %d %d %lld %lld %a %lld %lld\n", st, info.from_node[0], info.from_node[1],
                info.from_node[2], info.to_node[0], info.to_node[1], info.to_node[2], (long long)info.n_chain,
                (long long)info.n_settled, info.cost, (long long)n_out, j);
    if (chain)
      for (int64_t i = 0; i < info.n_chain; ++i) std::printf("%d %d %d\n", chain[3 * i], chain[3 * i + 1], chain[3 * i + 2]);
    for (int64_t i = 0; i < n_out; ++i) {
      for (int k = 0; k < 8; ++k) std::printf("%a ", rows[8 * i + k]);
      std::printf("\n");
    }
    std::free(rows);
    std::free(chain);
  }
  return 0;
}
