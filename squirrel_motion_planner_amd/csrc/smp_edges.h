// Edge table of the batched dense edge checks (smp_edges.hip), shared by the kernel and the C ABI.
#ifndef SMP_EDGES_H
#define SMP_EDGES_H

#include <hip/hip_runtime.h>

#include "smp_types.h"

namespace smp {

constexpr int EDGES_CT = 32;  // configurations per collision tile (the batch checker's CHECK_CT)

// One edge a -> b checked at its points k = 0..M, point k = a[j] + k * ((b[j] - a[j]) / M).
struct EdgeDev {
  double a[NJ], b[NJ];
  int M;    // >= 1 (formed on the host: num_traj_segments * hops of at most one planner step)
  int pad;
};

// Workgroups draw the edges order[0], order[1], ... from *counter (zeroed on the stream before the launch);
// first_invalid[e] = index of edge e's first colliding point, -1 if all M + 1 are free.
void launch_edges(int grid, hipStream_t st, const RobotDev* rb, SceneDev sc, const MapCfg* mc, const EdgeDev* edges,
                  const int* order, int n, int self, int map, unsigned* counter, int* first_invalid);
size_t edges_kernels_private_bytes();

}  // namespace smp
#endif  // SMP_EDGES_H
