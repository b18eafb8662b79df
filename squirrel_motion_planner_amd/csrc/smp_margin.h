// Tables of the margin passes (smp_margin.hip), shared by the kernels and the C ABI: the predicate "every point farther
// than mm from the map and ms from itself" (include/smp_gpu.h "Margin checks") for tiles of configurations, dense edges
// and detour items.
#ifndef SMP_MARGIN_H
#define SMP_MARGIN_H

#include <hip/hip_runtime.h>

#include "smp_pass.h"
#include "smp_types.h"

namespace smp {

// Per call (formed on the host: margin_threshold of smp_paths.cpp, and smp_clearance.h's prefilter thresholds at D = mm).
//   mm, ms: the margins; a part whose margin is 0 is the boolean test of that part (collide_tile);
//   S[s]:   an occupied cell is within mm of sphere s iff the squared distance s2 of the centre to the cell's box is
//           <= S[s], the largest double with fl(fl(sqrt(S)) - r_s) <= mm;
//   Sp:     the same for a primitive, whose term is fl(sqrt(prim_cell_s)): the largest double with fl(sqrt(Sp)) <= mm;
//   T, pT:  ClearCfg's widened prefilter thresholds at D = mm.
struct MarginCfg {
  double mm, ms;
  double S[MAX_SPH];
  double Sp;
  uint32_t T[MAX_SPH];
  uint32_t pT[MAX_PRIM];
  int self, map;  // the parts asked for (map: and a scene is set)
};

// One launch each over n_items items drawn from *counter (zeroed on the stream before the launch); the items, their
// order and their results are those of the plain passes with "colliding" read as "not clear":
//   configs: item t is the tile of configurations 32 t .. min(32 t + 31, n - 1) of q_rows (row-major n x 8),
//            clear[i] = 1 iff configuration i is clear;
//   base map: launch_base_map's tiles of lattice nodes (smp_pass.h), bit c of bits[t] set iff node 32 t + c is clear;
//   edges:   launch_edges' tables, first_invalid[e] = the lowest point of edge e that is not clear, -1 if none;
//   detours: launch_detours' tables and record, free = every point of both legs is clear.
void launch_margin_configs(int grid, hipStream_t st, const RobotDev* rb, SceneDev sc, const MapCfg* mc,
                           const MarginCfg& cfg, const double* q_rows, long long n, int n_items, unsigned* counter,
                           uint8_t* clear);
void launch_margin_base_map(int grid, hipStream_t st, const RobotDev* rb, SceneDev sc, const MapCfg* mc,
                            const MarginCfg& cfg, LatticeDev lat, int n_items, unsigned* counter, uint32_t* bits);
void launch_margin_edges(int grid, hipStream_t st, const RobotDev* rb, SceneDev sc, const MapCfg* mc,
                         const MarginCfg& cfg, const EdgeDev* edges, const int* order, int n, unsigned* counter,
                         int* first_invalid);
void launch_margin_detours(int grid, hipStream_t st, const RobotDev* rb, SceneDev sc, const MapCfg* mc,
                           const MarginCfg& cfg, const GapDev* gaps, DetourArgs args, unsigned* counter, DetourDev* out);
size_t margin_kernels_private_bytes();

}  // namespace smp
#endif  // SMP_MARGIN_H
