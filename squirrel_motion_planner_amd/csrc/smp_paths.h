// Host logic of the path tools, free of HIP (plain C++17, built with the library and on its own by the CPU tests): what
// smp_check_edges, smp_shortcut_path, smp_repair_path and smp_clearance_edges do before and after their launches
// (smp_api_paths.cpp).  It sees plain values, never smp_planner.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/smp_gpu.h"
#include "smp_pass.h"

namespace smp {

// The planner's values the density rule reads: the model's joint_is_revolute, smp_params.step_factor and
// smp_params.num_traj_segments; max_points is SMP_EDGE_MAX_POINTS.
struct EdgeRule {
  const int* rev;
  double step_factor;
  int num_traj_segments, max_points;
};

// The edge a -> b at the density rule (edge_segments).  False for a non-finite coordinate or more than max_points points.
bool make_edge(const EdgeRule& r, const double* a, const double* b, EdgeDev* e);

// The order in which the workgroups draw a table: longest first, equal lengths in table order.
std::vector<int> longest_first(const std::vector<EdgeDev>& edges);

double dist(const double* a, const double* b);  // DH:128-156

// The candidate window of smp_shortcut_path, and its candidates (i, j), i < j <= i + w, in the order of the dynamic
// program: j ascending, then i ascending.  False where make_edge refuses a pair.
inline int64_t shortcut_window(int64_t k, int window) { return (window <= 0 || window > k - 1) ? k - 1 : window; }
inline int64_t shortcut_candidates(int64_t k, int64_t w) { return w * (k - 1) - w * (w - 1) / 2; }
bool shortcut_edges(const EdgeRule& r, const double* waypoints, int64_t k, int64_t w, std::vector<EdgeDev>* edges);

// The cheapest route through the valid candidates (first[e] < 0): dp[j] = min_i dp[i] + dist(w_i, w_j), first strict
// minimum.  Returns the chosen edges from the first waypoint to the last, empty if the last cannot be reached, and
// fills every field of *info but the two times (first_blocked: the first blocked adjacent pair, -1 if a route exists).
std::vector<EdgeDev> shortcut_route(const double* waypoints, int64_t k, int64_t w, const std::vector<EdgeDev>& edges,
                                    const std::vector<int>& first, smp_shortcut_info* info);

// A blocked stretch of a path: (l, r) waypoint indices of its valid anchors, e its smallest blocked edge, v the via of
// the detour that closed it.
struct Gap {
  int64_t l, r, e;
  bool open;
  double v[NJ];
};

// The gaps of a path of k waypoints from their validity and the adjacent edges' first invalid points (first[i] >= 0:
// edge i is blocked); ranges that overlap merge, ranges that only share an anchor stay two gaps.
// Precondition: valid[0] and valid[k - 1] are set -- the walk to a gap's anchors stops nowhere else.  smp_repair_path
// returns SMP_ERR_START_INVALID / SMP_ERR_GOAL_INVALID before it comes here.
std::vector<Gap> find_gaps(const uint8_t* valid, const int* first, int64_t k, int64_t* n_blocked);

// The sample a round chooses among the items of gap g, whose anchors are a and b: the first strict minimum of
// dist(a, v) + dist(v, b) over the free ones, which closes the gap with its via; -1 if none is free.  *n_free grows by
// the free items.
int close_gap(Gap* g, const double* a, const double* b, const DetourDev* items, int samples, int64_t* n_free);

// The route of a repaired path, w_0 ... w_l, v, w_r, ... over the (closed) gaps, as edges at the density rule, and its
// cost.  False where make_edge refuses an edge.
bool repaired_route(const EdgeRule& r, const double* waypoints, int64_t k, const std::vector<Gap>& gaps,
                    std::vector<EdgeDev>* route, double* cost);

// The output rows of a route: every edge's start, then its via nodes (its points n, 2n, ... below M), and the last
// edge's end.  A malloc'd rows x NJ buffer (smp_buffer_free); nullptr, and *rows untouched, if the allocation fails.
double* route_rows(const std::vector<EdgeDev>& route, int num_traj_segments, int64_t* rows);

// The margin checks' threshold on a squared distance (include/smp_gpu.h "Margin checks"): the largest double S with
// fl(fl(sqrt(S)) - r) <= m, for a radius r >= 0 (0 for a primitive) and a margin m > 0, both finite.  sqrt and the
// subtraction are monotone, so a cell at squared distance s has a term <= m iff s <= S: the kernel compares squares and
// takes no square root per cell.  Found from fl((r + m)^2) by steps of one ulp.
double margin_threshold(double r, double m);

}  // namespace smp
