// The C++ drop-in shim's repairTrajectory followed by shortcutTrajectory (include/smp_birrt_star.hpp) on a trajectory
// given on the command line -- the node's sequence between run_planner and normalizeTrajectory; the answers are printed
// for comparison with the Python mirror's.
//
//   shim_repair <model.json> <scene.bt> <samples> <rounds> <seed> <k> <q x8> * k
//
// Prints "repair <ok 0|1> <rows> <n_blocked_edges> <n_gaps> <n_repaired> <n_items> <n_free> <rounds_used>
// <first_blocked> <cost_in> <cost_out>", one "row <8 values>" line per pose of the trajectory after the repair (%.17g,
// so the values round-trip), then "shortcut <ok 0|1> <rows>" and one "srow <8 values>" line per pose after the
// shortcut.  Exit 0 on success, 2 on usage error, 3 when no GPU is usable (the shim throws: there is no CPU fallback).
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
  const int k = argc > 6 ? std::atoi(argv[6]) : -1;
  if (k < 0 || argc != 7 + 8 * k) {
    std::fprintf(stderr, "usage: shim_repair model.json scene.bt samples rounds seed k q[8]*k\n");
    return 2;
  }
  const int samples = std::atoi(argv[3]), rounds = std::atoi(argv[4]);
  const unsigned long long seed = std::strtoull(argv[5], nullptr, 10);
  setenv("SMP_ROBOT_MODEL", argv[1], 1);
  birrt_star_motion_planning::BiRRTstarPlanner planner;
  try {
    planner.initialize("robotino_robot");
  } catch (const std::exception& e) {
    std::printf("error %s\n", e.what());
    return 3;
  }
  std::ifstream f(argv[2], std::ios::binary);
  const std::string bt((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  planner.setOctreeBinary(reinterpret_cast<const uint8_t*>(bt.data()), bt.size(), 0.05);
  std::vector<std::vector<double> > traj((size_t)k, std::vector<double>(8));
  for (int i = 0; i < k; ++i)
    for (int j = 0; j < 8; ++j) traj[(size_t)i][(size_t)j] = std::atof(argv[7 + 8 * i + j]);
  const bool ok = planner.repairTrajectory(traj, true, true, samples, rounds, seed);
  const smp_repair_info& r = planner.lastRepair();
  std::printf("repair %d %d %lld %lld %lld %lld %lld %d %lld %.17g %.17g\n", ok ? 1 : 0, (int)traj.size(),
              (long long)r.n_blocked_edges, (long long)r.n_gaps, (long long)r.n_repaired, (long long)r.n_items,
              (long long)r.n_free, (int)r.rounds_used, (long long)r.first_blocked, r.cost_in, r.cost_out);
  print_rows("row", traj);
  const bool sok = planner.shortcutTrajectory(traj, true, true, 0);
  std::printf("shortcut %d %d\n", sok ? 1 : 0, (int)traj.size());
  print_rows("srow", traj);
  return 0;
}
