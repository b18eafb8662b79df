// Gap table and results of the batched one-via detours (smp_repair.hip), shared by the kernel and the C ABI.
#ifndef SMP_REPAIR_H
#define SMP_REPAIR_H

#include <hip/hip_runtime.h>

#include "smp_types.h"

namespace smp {

constexpr int DETOURS_CT = 32;  // configurations per collision tile (the batch checker's CHECK_CT)

// One gap: the two anchors a detour a -> v -> b joins, and the gap's index in the Philox stream.
struct GapDev {
  double a[NJ], b[NJ];
  unsigned g;
  int pad;
};

// Result of one item (gap, sample); the layout of smp_detour (include/smp_gpu.h).
struct DetourDev {
  double v[NJ];
  int M1, M2;  // segments of the legs a -> v and v -> b; 0 for a leg of more than SMP_EDGE_MAX_POINTS points
  int free;    // 1: every point of both legs is free
  int pad;
};

struct DetourArgs {
  int n_items, samples;  // items = gaps x samples, item i = (i / samples, i % samples)
  int n_seg;             // num_traj_segments
  int max_points;        // SMP_EDGE_MAX_POINTS: a leg of more points makes its item blocked
  int self, map;
  unsigned round;
  unsigned long long seed;
  double step, h;        // step_factor, half width of the round
};

// Workgroups draw the items 0, 1, ... from *counter (zeroed on the stream before the launch); out[i] is item i's.
void launch_detours(int grid, hipStream_t st, const RobotDev* rb, SceneDev sc, const MapCfg* mc, const GapDev* gaps,
                    DetourArgs args, unsigned* counter, DetourDev* out);
size_t repair_kernels_private_bytes();

}  // namespace smp
#endif  // SMP_REPAIR_H
