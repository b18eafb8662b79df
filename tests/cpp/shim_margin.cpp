// The C++ drop-in shim's margin calls (include/smp_birrt_star.hpp: isEdgeClear and the margin overloads of
// repairTrajectory and shortcutTrajectory) on one planned trajectory; the answers are printed for comparison with the
// Python mirror's.
//
//   shim_margin <model.json> <scene.bt> <iterations> <seed> <margin_map> <margin_self> <samples> <window>
//               <start x8> <goal x8> <env x4>
//
// Prints "status <ok 0|1>", "waypoints <n>" and, when a trajectory was planned,
//   "clear <ok 0|1> <last_clear_node_idx>" of the edge from its first to its last pose,
//   "repair <ok 0|1> <rows> <n_blocked_edges> <n_gaps> <n_repaired> <n_items> <n_free> <rounds_used> <first_blocked>
//    <cost_in> <cost_out>" and one "row <8 values>" line per pose after the repair,
//   "shortcut <ok 0|1> <rows> <n_edges> <n_valid> <cost_out>" and one "srow <8 values>" line per pose after the shortcut
// (%.17g, so the values round-trip).  Exit 0 on success, 2 on usage error, 3 when no GPU is usable (the shim throws:
// there is no CPU fallback).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "smp_birrt_star.hpp"

static void print_rows(const char* tag, const std::vector<std::vector<double> >& traj) {
  for (size_t i = 0; i < traj.size(); ++i) {
    std::printf("%s", tag);
    for (int j = 0; j < 8; ++j) std::printf(" %.17g", traj[i][(size_t)j]);
    std::printf("\n");
  }
}

int main(int argc, char** argv) {
  if (argc != 1 + 8 + 16 + 4) {
    std::fprintf(stderr, "usage: shim_margin model.json scene.bt iterations seed margin_map margin_self samples window "
                         "start[8] goal[8] env[4]\n");
    return 2;
  }
  typedef birrt_star_motion_planning::BiRRTstarPlanner Planner;
  setenv("SMP_ROBOT_MODEL", argv[1], 1);
  setenv("SMP_SEED", argv[4], 1);
  const double mm = std::atof(argv[5]), ms = std::atof(argv[6]);
  const int samples = std::atoi(argv[7]), window = std::atoi(argv[8]);
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
  const bool ok = planner.run_planner(1, false, std::atof(argv[3]), false, 0.0, 0);
  std::vector<std::vector<double> > traj = planner.getJointTrajectoryRef();
  std::printf("status %d\nwaypoints %zu\n", ok ? 1 : 0, traj.size());
  if (!ok || traj.size() < 2) return 0;
  int last = -1;
  const bool clear = planner.isEdgeClear(traj.front(), traj.back(), last, true, true, mm, ms);
  std::printf("clear %d %d\n", clear ? 1 : 0, last);
  const bool rok = planner.repairTrajectory(traj, true, true, samples, 4, 1ull, mm, ms);
  const smp_repair_info& r = planner.lastRepair();
  std::printf("repair %d %d %lld %lld %lld %lld %lld %d %lld %.17g %.17g\n", rok ? 1 : 0, (int)traj.size(),
              (long long)r.n_blocked_edges, (long long)r.n_gaps, (long long)r.n_repaired, (long long)r.n_items,
              (long long)r.n_free, (int)r.rounds_used, (long long)r.first_blocked, r.cost_in, r.cost_out);
  print_rows("row", traj);
  const bool sok = planner.shortcutTrajectory(traj, true, true, window, mm, ms);
  const smp_shortcut_info& s = planner.lastShortcut();
  std::printf("shortcut %d %d %lld %lld %.17g\n", sok ? 1 : 0, (int)traj.size(), (long long)s.n_edges,
              (long long)s.n_valid, s.cost_out);
  print_rows("srow", traj);
  return 0;
}
