// Table driver of the path tools' host logic (csrc/smp_paths.cpp) for tests/test_paths_cpu.py; built with
// -fsanitize=address,undefined.  Cases come from stdin, doubles in any form scanf's %lf reads (hex floats, nan, inf);
// doubles go out as hex floats.  Every case of the last three modes starts with the density rule's values
//   RULE = rev[0] .. rev[7] step_factor num_traj_segments max_points
//
//   paths_table density    first RULE, then per case a[0..7] b[0..7]; out: M of make_edge, 0 where it refuses
//   paths_table gaps       per case: k valid[0..k-1] first[0..k-2]; out: "n_blocked n_gaps" then "; l r e" per gap
//   paths_table shortcut   per case: RULE k window w[0..k-1][0..7] first[0..n_edges-1];
//                          out: "n_edges n_valid configs_checked first_blocked cost_in cost_out rows" then the rows
//                          (rows = 0: no route), or "refused" where make_edge refuses a candidate
//   paths_table repair     per case: RULE k samples n_gaps w[0..k-1][0..7], per gap "l r e" and samples x (free v[0..7]);
//                          out: the chosen sample per gap, then "; n_free first_blocked cost_out rows" and the rows
//                          (rows = 0: a gap stays open or make_edge refuses a route edge)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../squirrel_motion_planner_amd/csrc/smp_paths.h"

using namespace smp;

static int g_rev[NJ];

static bool read_rule(EdgeRule* r) {
  for (int j = 0; j < NJ; ++j)
    if (std::scanf("%d", &g_rev[j]) != 1) return false;
  r->rev = g_rev;
  return std::scanf("%lf %d %d", &r->step_factor, &r->num_traj_segments, &r->max_points) == 3;
}

static bool read_doubles(double* out, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (std::scanf("%lf", &out[i]) != 1) return false;
  return true;
}

// " rows" and the rows of a route, or " 0"
static void print_rows(const std::vector<EdgeDev>& route, int n_seg) {
  int64_t rows = 0;
  double* out = route.empty() ? nullptr : route_rows(route, n_seg, &rows);
  std::printf(" %lld", (long long)(out ? rows : 0));
  for (int64_t i = 0; out && i < rows * NJ; ++i) std::printf(" %a", out[i]);
  std::free(out);
}

static int run_density() {
  EdgeRule r;
  if (!read_rule(&r)) return 2;
  double ab[2 * NJ];
  while (read_doubles(ab, 2 * NJ)) {
    EdgeDev e;
    std::printf("%d\n", make_edge(r, ab, ab + NJ, &e) ? e.M : 0);
  }
  return 0;
}

static int run_gaps() {
  int k = 0;
  while (std::scanf("%d", &k) == 1) {
    if (k < 2) return 2;
    std::vector<uint8_t> valid((size_t)k);
    std::vector<int> first((size_t)k - 1);
    for (int i = 0; i < k; ++i) {
      int v = 0;
      if (std::scanf("%d", &v) != 1) return 2;
      valid[(size_t)i] = v ? 1 : 0;
    }
    for (int i = 0; i + 1 < k; ++i)
      if (std::scanf("%d", &first[(size_t)i]) != 1) return 2;
    if (!valid[0] || !valid[(size_t)k - 1]) return 2;  // find_gaps' precondition
    int64_t n_blocked = 0;
    const std::vector<Gap> gaps = find_gaps(valid.data(), first.data(), k, &n_blocked);
    std::printf("%lld %zu", (long long)n_blocked, gaps.size());
    for (const Gap& g : gaps) std::printf(" ; %lld %lld %lld", (long long)g.l, (long long)g.r, (long long)g.e);
    std::printf("\n");
  }
  return 0;
}

static int run_shortcut() {
  EdgeRule r;
  while (read_rule(&r)) {
    int k = 0, window = 0;
    if (std::scanf("%d %d", &k, &window) != 2 || k < 2) return 2;
    std::vector<double> w((size_t)k * NJ);
    if (!read_doubles(w.data(), w.size())) return 2;
    const int64_t win = shortcut_window(k, window);
    std::vector<int> first((size_t)shortcut_candidates(k, win));
    for (int& f : first)
      if (std::scanf("%d", &f) != 1) return 2;
    std::vector<EdgeDev> edges;
    if (!shortcut_edges(r, w.data(), k, win, &edges)) {
      std::printf("refused\n");
      continue;
    }
    if (edges.size() != first.size()) return 2;
    smp_shortcut_info s;
    const std::vector<EdgeDev> route = shortcut_route(w.data(), k, win, edges, first, &s);
    std::printf("%lld %lld %lld %lld %a %a", (long long)s.n_edges, (long long)s.n_valid, (long long)s.configs_checked,
                (long long)s.first_blocked, s.cost_in, s.cost_out);
    print_rows(route, r.num_traj_segments);
    std::printf("\n");
  }
  return 0;
}

static int run_repair() {
  EdgeRule r;
  while (read_rule(&r)) {
    int k = 0, samples = 0, n_gaps = 0;
    if (std::scanf("%d %d %d", &k, &samples, &n_gaps) != 3 || k < 2 || samples < 1 || n_gaps < 0) return 2;
    std::vector<double> w((size_t)k * NJ);
    if (!read_doubles(w.data(), w.size())) return 2;
    std::vector<Gap> gaps((size_t)n_gaps);
    std::vector<DetourDev> items((size_t)samples);
    int64_t n_free = 0;
    for (Gap& g : gaps) {
      long long l = 0, rr = 0, e = 0;
      if (std::scanf("%lld %lld %lld", &l, &rr, &e) != 3 || l < 0 || rr <= l || rr >= k) return 2;
      g = Gap{};
      g.l = l; g.r = rr; g.e = e; g.open = true;
      for (DetourDev& it : items) {
        it = DetourDev{};
        if (std::scanf("%d", &it.free) != 1 || !read_doubles(it.v, NJ)) return 2;
      }
      std::printf("%d ", close_gap(&g, &w[(size_t)l * NJ], &w[(size_t)rr * NJ], items.data(), samples, &n_free));
    }
    int64_t first_blocked = -1;  // as smp_repair_path reports it: the first open gap's smallest blocked edge
    for (const Gap& g : gaps)
      if (g.open) { first_blocked = g.e; break; }
    std::vector<EdgeDev> route;
    double cost = 0.0;
    if (first_blocked >= 0 || !repaired_route(r, w.data(), k, gaps, &route, &cost)) {
      route.clear();
      cost = 0.0;
    }
    std::printf("; %lld %lld %a", (long long)n_free, (long long)first_blocked, cost);
    print_rows(route, r.num_traj_segments);
    std::printf("\n");
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && std::strcmp(argv[1], "density") == 0) return run_density();
  if (argc == 2 && std::strcmp(argv[1], "gaps") == 0) return run_gaps();
  if (argc == 2 && std::strcmp(argv[1], "shortcut") == 0) return run_shortcut();
  if (argc == 2 && std::strcmp(argv[1], "repair") == 0) return run_repair();
  std::fprintf(stderr, "usage: paths_table density|gaps|shortcut|repair < cases\n");
  return 2;
}
