// The far-goal calls from C++: the host-only part of the C ABI (smp_base_lattice_fit, smp_base_route,
// smp_far_opts_default) on a small map of the program's own, then the drop-in shim's two-stage plan
// (include/smp_birrt_star.hpp: smp_node::planFar over BiRRTstarPlanner::run_planner_far) on a scene file; the answers
// are printed for comparison with the restatement and the Python mirror.
//
//   shim_far <model.json> <scene.bt> <iterations> <seed> <pitch> <n_theta> <handover> <margin> <start x8> <goal x8> <env x4>
//
// Prints "opts <pitch> <n_theta> <arm x5> <handover> <margin> <window> <snap>" (the defaults),
//   "fit <status> <nx> <ny> <n_theta> <wrap> <x0> <y0> <dtheta>",
//   "route <status> <n_chain> <n_out> <n_settled> <cost>", one "chain <ix> <iy> <t>" line per chain node and one
//   "rrow <8 values>" line per merged row: a 6 x 5 x 2 lattice whose layer 0 has a wall with no door and whose layer 1
//   is free, from (0, 2, 0) to (5, 2, 0);
// then, with a GPU, "status <ok 0|1>", "far <stage> <n_route_rows> <handover ix iy t> <n_chain> <route cost> <n_nodes>
// <n_free> <n_edges> <n_valid>", "waypoints <n>" and one "row <8 values>" line per pose (%.17g, so the values
// round-trip).  Exit 0 on success, 2 on usage error, 3 when no GPU is usable (the shim throws: there is no CPU fallback).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "smp_birrt_star.hpp"

static void print_row(const char* tag, const double* r) {
  std::printf("%s", tag);
  for (int j = 0; j < 8; ++j) std::printf(" %.17g", r[j]);
  std::printf("\n");
}

static void host_part() {
  smp_far_opts o;
  smp_far_opts_default(&o);
  std::printf("opts %.17g %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g %d %d\n", o.pitch, o.n_theta, o.arm[0], o.arm[1],
              o.arm[2], o.arm[3], o.arm[4], o.handover_distance, o.map_margin, o.window, o.snap_cells);
  const double ex[2] = {-1.0, 0.3}, ey[2] = {0.5, 1.6};
  smp_base_lattice lat;
  const int fs = smp_base_lattice_fit(ex, ey, 0.25, 2, 0.0, o.arm, &lat);
  std::printf("fit %d %d %d %d %d %.17g %.17g %.17g\n", fs, lat.nx, lat.ny, lat.n_theta, lat.wrap_theta, lat.x0, lat.y0,
              lat.dtheta);
  if (fs != SMP_OK) return;
  // 60 nodes: layer 0 without column 3, layer 1 whole
  std::vector<uint32_t> bits(2, 0u);
  for (int n = 0; n < 60; ++n)
    if (n >= 30 || n % 6 != 3) bits[(size_t)(n >> 5)] |= 1u << (n & 31);
  const double from[3] = {lat.x0, lat.y0 + 2 * lat.pitch, 0.0}, to[3] = {lat.x0 + 5 * lat.pitch, lat.y0 + 2 * lat.pitch, 0.0};
  double* rows = nullptr;
  int64_t n_out = 0;
  int32_t* chain = nullptr;
  smp_route_info info;
  const int rs = smp_base_route(&lat, bits.data(), from, to, 0, &rows, &n_out, &chain, &info);
  std::printf("route %d %lld %lld %lld %.17g\n", rs, (long long)info.n_chain, (long long)n_out, (long long)info.n_settled,
              info.cost);
  for (int64_t i = 0; rs == SMP_OK && i < info.n_chain; ++i)
    std::printf("chain %d %d %d\n", chain[3 * i], chain[3 * i + 1], chain[3 * i + 2]);
  for (int64_t i = 0; i < n_out; ++i) print_row("rrow", rows + 8 * i);
  smp_buffer_free(rows);
  smp_buffer_free(chain);
}

int main(int argc, char** argv) {
  if (argc != 1 + 8 + 16 + 4) {
    std::fprintf(stderr, "usage: shim_far model.json scene.bt iterations seed pitch n_theta handover margin "
                         "start[8] goal[8] env[4]\n");
    return 2;
  }
  host_part();
  typedef birrt_star_motion_planning::BiRRTstarPlanner Planner;
  setenv("SMP_ROBOT_MODEL", argv[1], 1);
  setenv("SMP_SEED", argv[4], 1);
  Planner planner;
  try {
    planner.initialize("robotino_robot");
  } catch (const std::exception& e) {
    std::printf("error %s\n", e.what());
    return 3;
  }
  std::ifstream f(argv[2], std::ios::binary);
  const std::string bt((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  planner.setOctreeBinary(reinterpret_cast<const uint8_t*>(bt.data()), bt.size(), 0.05);
  std::vector<double> start(8), goal(8);
  for (int j = 0; j < 8; ++j) { start[j] = std::atof(argv[9 + j]); goal[j] = std::atof(argv[17 + j]); }
  std::vector<double> ex = {std::atof(argv[25]), std::atof(argv[26])}, ey = {std::atof(argv[27]), std::atof(argv[28])};
  planner.reset_planner_and_config();
  planner.setPlanningSceneInfo(ex, ey, "scenario");
  if (!planner.init_planner(start, goal, 1, true, true)) {
    std::printf("status init_failed\n");
    return 0;
  }
  smp_far_opts o;
  smp_far_opts_default(&o);
  const std::vector<double> folded(o.arm, o.arm + 5);
  smp_far_info far;
  const bool ok = smp_node::planFar(planner, false, std::atof(argv[3]), folded, std::atof(argv[8]), std::atof(argv[7]),
                                    &far, std::atof(argv[5]), std::atoi(argv[6]));
  const std::vector<std::vector<double> >& traj = planner.getJointTrajectoryRef();
  std::printf("status %d\n", ok ? 1 : 0);
  std::printf("far %d %lld %d %d %d %lld %.17g %lld %lld %lld %lld\n", far.stage, (long long)far.n_route_rows,
              far.handover_node[0], far.handover_node[1], far.handover_node[2], (long long)far.route.n_chain,
              far.route.cost, (long long)far.map.n_nodes, (long long)far.map.n_free, (long long)far.check.n_edges,
              (long long)far.check.n_valid);
  std::printf("waypoints %zu\n", traj.size());
  for (size_t i = 0; i < traj.size(); ++i) print_row("row", traj[i].data());
  return 0;
}
