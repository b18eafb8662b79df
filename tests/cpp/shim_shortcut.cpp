// The C++ drop-in shim's isEdgeValid and shortcutTrajectory (include/smp_birrt_star.hpp) on a trajectory given on the
// command line; the answers are printed for comparison with the Python mirror's.
//
//   shim_shortcut <model.json> <scene.bt> <window> <k> <q x8> * k
//
// Prints "edge <i> <valid 0|1> <last_valid_node_idx>" for every consecutive pair of poses, then
// "shortcut <ok 0|1> <rows>" and one "row <8 values>" line per pose of the shortened trajectory (%.17g, so the values
// round-trip).  Exit 0 on success, 2 on usage error, 3 when no GPU is usable (the shim throws: there is no CPU
// fallback).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "smp_birrt_star.hpp"

int main(int argc, char** argv) {
  const int k = argc > 4 ? std::atoi(argv[4]) : -1;
  if (k < 0 || argc != 5 + 8 * k) {
    std::fprintf(stderr, "usage: shim_shortcut model.json scene.bt window k q[8]*k\n");
    return 2;
  }
  const int window = std::atoi(argv[3]);
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
    for (int j = 0; j < 8; ++j) traj[(size_t)i][(size_t)j] = std::atof(argv[5 + 8 * i + j]);
  for (int i = 0; i + 1 < k; ++i) {
    int last = -1;
    const bool ok = planner.isEdgeValid(traj[(size_t)i], traj[(size_t)i + 1], last, true, true);
    std::printf("edge %d %d %d\n", i, ok ? 1 : 0, last);
  }
  const bool ok = planner.shortcutTrajectory(traj, true, true, window);
  std::printf("shortcut %d %d\n", ok ? 1 : 0, (int)traj.size());
  for (size_t i = 0; i < traj.size(); ++i) {
    std::printf("row");
    for (int j = 0; j < 8; ++j) std::printf(" %.17g", traj[i][(size_t)j]);
    std::printf("\n");
  }
  return 0;
}
