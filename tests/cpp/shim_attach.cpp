// The C++ drop-in shim's attached-object calls (include/smp_birrt_star.hpp: attachBox, setSelfFilter, detachObject) in
// the node's order -- attach after the grasp, self filter before the map hand-off, plan, detach after the release --
// on a map that holds the grasped bar's own voxels; the answers are printed for comparison with the Python mirror's.
//
//   shim_attach <model.json> <scene.bt> <iterations> <seed> <pad> <start x8> <goal x8> <env x4>
//
// The object is the tests' bar: half extents (0.03, 0.03, 0.10) centred at (0, 0, 0.15) of hand_palm_link, covered
// within 1 cm.  Prints
//   "attach <ok 0|1>", "refused <ok 0|1>" (a second object under the same name),
//   "uncarved <init ok 0|1>" and "maplinks <names>" (the links touching the map at the start pose, uncarved),
//   "carved <init ok 0|1> <run ok 0|1> <waypoints>" and one "row <8 values>" line per pose (%.17g),
//   "detached <start valid 0|1>" (the bare robot on the uncarved map).
// Exit 0 on success, 2 on usage error, 3 when no GPU is usable (the shim throws: there is no CPU fallback).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <utility>
#include <vector>

#include "smp_birrt_star.hpp"

int main(int argc, char** argv) {
  if (argc != 1 + 5 + 16 + 4) {
    std::fprintf(stderr, "usage: shim_attach model.json scene.bt iterations seed pad start[8] goal[8] env[4]\n");
    return 2;
  }
  typedef birrt_star_motion_planning::BiRRTstarPlanner Planner;
  setenv("SMP_ROBOT_MODEL", argv[1], 1);
  setenv("SMP_SEED", argv[4], 1);
  const double pad = std::atof(argv[5]);
  Planner planner;
  try {
    planner.initialize("robotino_robot");
  } catch (const std::exception& e) {
    std::printf("error %s\n", e.what());
    return 3;
  }
  std::ifstream f(argv[2], std::ios::binary);
  const std::string bt((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  const uint8_t* map = reinterpret_cast<const uint8_t*>(bt.data());
  std::vector<double> start(8), goal(8);
  for (int j = 0; j < 8; ++j) { start[j] = std::atof(argv[6 + j]); goal[j] = std::atof(argv[14 + j]); }
  std::vector<double> ex = {std::atof(argv[22]), std::atof(argv[23])}, ey = {std::atof(argv[24]), std::atof(argv[25])};

  // after the grasp
  const std::vector<double> half = {0.03, 0.03, 0.10};
  const std::vector<double> pose = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0.0, 0.0, 0.15};
  std::printf("attach %d\n", planner.attachBox("hand_palm_link", half, pose, 0.01) ? 1 : 0);
  std::printf("refused %d\n", planner.attachBox("hand_palm_link", half, pose, 0.01) ? 1 : 0);

  // the map as fetched: it holds the bar
  planner.setOctreeBinary(map, bt.size(), 0.05);
  planner.reset_planner_and_config();
  planner.setPlanningSceneInfo(ex, ey, "scenario");
  std::printf("uncarved %d\n", planner.init_planner(start, goal, 1, true, true) ? 1 : 0);
  std::vector<std::pair<std::string, std::string> > self_c;
  std::vector<std::string> map_c;
  planner.getCollisions(start, self_c, map_c);
  std::printf("maplinks");
  for (size_t i = 0; i < map_c.size(); ++i) std::printf(" %s", map_c[i].c_str());
  std::printf("\n");

  // the self filter before the map hand-off, then the plan
  planner.setSelfFilter(start, pad, std::vector<std::string>(1, "attached_object"));
  planner.setOctreeBinary(map, bt.size(), 0.05);
  planner.reset_planner_and_config();
  planner.setPlanningSceneInfo(ex, ey, "scenario");
  const bool init = planner.init_planner(start, goal, 1, true, true);
  const bool ok = init && planner.run_planner(1, false, std::atof(argv[3]), false, 0.0, 0);
  const std::vector<std::vector<double> > traj = ok ? planner.getJointTrajectoryRef() : std::vector<std::vector<double> >();
  std::printf("carved %d %d %zu\n", init ? 1 : 0, ok ? 1 : 0, traj.size());
  for (size_t i = 0; i < traj.size(); ++i) {
    std::printf("row");
    for (int j = 0; j < 8; ++j) std::printf(" %.17g", traj[i][(size_t)j]);
    std::printf("\n");
  }

  // after the release
  planner.detachObject();
  planner.setSelfFilter(std::vector<double>());
  planner.setOctreeBinary(map, bt.size(), 0.05);
  std::printf("detached %d\n", planner.isConfigValid(start, true, true) ? 1 : 0);
  return 0;
}
