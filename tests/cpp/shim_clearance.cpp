// The C++ drop-in shim's clearance calls (include/smp_birrt_star.hpp: getClearance, getEdgeClearance,
// getTrajectoryClearance) on one planned trajectory; the answers are printed for comparison with the Python mirror's.
//
//   shim_clearance <model.json> <scene.bt> <iterations> <seed> <max_dist> <start x8> <goal x8> <env x4>
//
// Prints "status <ok 0|1>", "waypoints <n>" and, when a trajectory was planned,
//   "clearance <map> <self> <map_link> <self_a> <self_b>" of its middle pose,
//   "edge <map> <self> <map_point> <self_point> <map_link> <self_a> <self_b> <n_points>" of the edge from its first to its
//   last pose, and
//   "trajectory <map> <self> <map_edge> <map_point> <self_edge> <self_point> <map_link> <self_a> <self_b> <n_points>"
// (%.17g, so the values round-trip; "-" for no link).  Exit 0 on success, 2 on usage error, 3 when no GPU is usable (the
// shim throws: there is no CPU fallback).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "smp_birrt_star.hpp"

static const char* name(const std::string& s) { return s.empty() ? "-" : s.c_str(); }

int main(int argc, char** argv) {
  if (argc != 1 + 5 + 16 + 4) {
    std::fprintf(stderr, "usage: shim_clearance model.json scene.bt iterations seed max_dist start[8] goal[8] env[4]\n");
    return 2;
  }
  typedef birrt_star_motion_planning::BiRRTstarPlanner Planner;
  setenv("SMP_ROBOT_MODEL", argv[1], 1);
  setenv("SMP_SEED", argv[4], 1);
  const double D = std::atof(argv[5]);
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
  for (int j = 0; j < 8; ++j) { start[j] = std::atof(argv[6 + j]); goal[j] = std::atof(argv[14 + j]); }
  std::vector<double> ex = {std::atof(argv[22]), std::atof(argv[23])}, ey = {std::atof(argv[24]), std::atof(argv[25])};
  planner.reset_planner_and_config();
  planner.setPlanningSceneInfo(ex, ey, "scenario");
  Planner::TrajectoryClearance t;
  std::printf("empty %d\n", planner.getTrajectoryClearance(t, D) ? 1 : 0);  // nothing planned yet
  if (!planner.init_planner(start, goal, 1, true, true)) {
    std::printf("status init_failed\n");
    return 0;
  }
  const bool ok = planner.run_planner(1, false, std::atof(argv[3]), false, 0.0, 0);
  const std::vector<std::vector<double> >& traj = planner.getJointTrajectoryRef();
  std::printf("status %d\nwaypoints %zu\n", ok ? 1 : 0, traj.size());
  if (!ok || traj.size() < 2) return 0;
  const Planner::Clearance c = planner.getClearance(traj[traj.size() / 2], D);
  std::printf("clearance %.17g %.17g %s %s %s\n", c.map, c.self, name(c.map_link), name(c.self_a), name(c.self_b));
  const Planner::EdgeClearance e = planner.getEdgeClearance(traj.front(), traj.back(), D);
  std::printf("edge %.17g %.17g %d %d %s %s %s %d\n", e.map, e.self, e.map_point, e.self_point, name(e.map_link),
              name(e.self_a), name(e.self_b), e.n_points);
  if (!planner.getTrajectoryClearance(t, D)) return 1;
  std::printf("trajectory %.17g %.17g %d %d %d %d %s %s %s %lld\n", t.map, t.self, t.map_edge, t.map_point, t.self_edge,
              t.self_point, name(t.map_link), name(t.self_a), name(t.self_b), t.n_points);
  return 0;
}
