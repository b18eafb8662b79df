// Tables and records of the clearance queries (smp_clearance.hip), shared by the kernel and the C ABI.
#ifndef SMP_CLEARANCE_H
#define SMP_CLEARANCE_H

#include <hip/hip_runtime.h>

#include "smp_pass.h"
#include "smp_types.h"

namespace smp {

// Per call: the query distance and the widened prefilter thresholds it gives (formed on the host).
// T[s]  = floor(((r_s + D + 1e-6) / res)^2): the box-gap field at the sphere's centre cell above it means the sphere's
//         map term exceeds D.
// pT[p] = the same with the radius sqrt(rxy_p^2 + hz_p^2) of the ball around the primitive's centre that holds it.
// Both stay below the field's clamp (65535): the C ABI refuses a D that reaches it.
struct ClearCfg {
  double D;
  uint32_t T[MAX_SPH];
  uint32_t pT[MAX_PRIM];
  int with_self, with_map;
};

// The C ABI's smp_clearance and smp_edge_clearance (include/smp_gpu.h), written by the kernel as they are.
struct ClearDev {
  double map, self;
  int32_t map_link, self_a, self_b, pad;
};
struct EdgeClearDev {
  double map, self;
  int32_t map_point, self_point, map_link, self_a, self_b, n_points;
};
static_assert(sizeof(ClearDev) == 32 && sizeof(EdgeClearDev) == 40, "the C ABI's records");

// One launch over n_items items drawn from *counter (zeroed on the stream before the launch).
//   edges == nullptr: item t is the tile of configurations 32 t .. min(32 t + 31, n - 1) (PASS_CT each) of q_rows
//                     (row-major n x 8),
//                     out_c[i] per configuration;
//   else:             item t is edge order[t] of the table (n = n_items edges), out_e[e] per edge.
void launch_clearance(int grid, hipStream_t st, const RobotDev* rb, SceneDev sc, const MapCfg* mc, const ClearCfg& cfg,
                      const double* q_rows, long long n, const EdgeDev* edges, const int* order, int n_items,
                      unsigned* counter, ClearDev* out_c, EdgeClearDev* out_e);
size_t clearance_kernels_private_bytes();

}  // namespace smp
#endif  // SMP_CLEARANCE_H
