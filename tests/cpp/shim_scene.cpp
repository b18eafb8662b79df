// The C++ drop-in shim's setOctreeBinary (include/smp_birrt_star.hpp), which builds the planner's scene on the GPU
// (smp_planner_set_scene_bt), checked through isConfigValid against answers computed elsewhere.
//
//   shim_scene <model.json> <scene.bt> <n> <q x8> * n <expected 0|1> * n
//
// Prints "valid <i> <got> <want>" per configuration; exit 0 when all agree, 1 on a mismatch, 2 on usage error, 3 when
// no GPU is usable (the shim throws: there is no CPU fallback).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "smp_birrt_star.hpp"

int main(int argc, char** argv) {
  const int n = argc > 3 ? std::atoi(argv[3]) : -1;
  if (n < 0 || argc != 4 + 9 * n) {
    std::fprintf(stderr, "usage: shim_scene model.json scene.bt n q[8]*n expected*n\n");
    return 2;
  }
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
  int bad = 0;
  for (int i = 0; i < n; ++i) {
    std::vector<double> q(8);
    for (int j = 0; j < 8; ++j) q[j] = std::atof(argv[4 + 8 * i + j]);
    const int want = std::atoi(argv[4 + 8 * n + i]);
    const int got = planner.isConfigValid(q, true, true) ? 1 : 0;
    std::printf("valid %d %d %d\n", i, got, want);
    bad += got != want;
  }
  return bad ? 1 : 0;
}
