// What the path passes share (smp_edges.hip, smp_repair.hip, smp_clearance.hip and their host side): the tile size, the
// tables' records, the density rule and, for the kernels, the work loop and the edge walk.  Everything outside the
// __HIPCC__ part is plain C++ that smp_paths.cpp and the CPU tests build without HIP.
#ifndef SMP_PASS_H
#define SMP_PASS_H

#include "smp_math.h"
#include "smp_types.h"

namespace smp {

constexpr int PASS_CT = 32;  // configurations per tile (the batch checker's CHECK_CT)

// One edge a -> b checked at its points k = 0..M, point k = a[j] + k * ((b[j] - a[j]) / M).
struct EdgeDev {
  double a[NJ], b[NJ];
  int M;    // >= 1 (formed on the host: edge_segments)
  int pad;
};

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

// The density rule (include/smp_gpu.h, smp_check_edges): segments M = n_seg * m of the edge whose squared revolute and
// prismatic lengths are sr and sp (each summed for joints ascending, as stepTowardsRandSample does,
// birrt_star.cpp:5712-5868), m hops of at most one planner step.  0 for an edge of more than max_points points or a
// non-finite length.  Host and device form it with these operations in this order (fp64 sqrt, division and ceil are
// correctly rounded on both), so they agree bit for bit.
SMP_HD int edge_segments(double sr, double sp, double step, int n_seg, int max_points) {
  const double x = ceil(fmax(sqrt(sr), sqrt(sp)) / step);
  if (!(x * n_seg <= (double)(max_points - 1))) return 0;
  return n_seg * (x < 1.0 ? 1 : (int)x);
}

// The base lattice as the free-map kernels see it (smp_base_lattice, include/smp_gpu.h "Far goals"): node
// n = (t * ny + iy) * nx + ix is the configuration [x0 + ix * pitch, y0 + iy * pitch, theta0 + t * dtheta, arm].
struct LatticeDev {
  double x0, y0, pitch, theta0, dtheta;
  double arm[NJ - 3];
  int nx, ny;
  long long n;  // nx * ny * n_theta
};

// Coordinate j of node (ix, iy, t): the integer converted, then the product, then the sum, each rounded on its own
// (no contraction, on host and device alike: smp_route.cpp forms the route's rows with it).
SMP_HD double lattice_coord(const LatticeDev& lat, int ix, int iy, int t, int j) {
  if (j == 0) return lat.x0 + (double)ix * lat.pitch;
  if (j == 1) return lat.y0 + (double)iy * lat.pitch;
  if (j == 2) return lat.theta0 + (double)t * lat.dtheta;
  return j == 3 ? lat.arm[0] : j == 4 ? lat.arm[1] : j == 5 ? lat.arm[2] : j == 6 ? lat.arm[3] : lat.arm[4];
}

#if defined(__HIPCC__)

// The launch of base_map_kernel (smp_lattice.hip; the margin variant is smp_margin.h's): item t is the tile of nodes
// 32 t .. min(32 t + 31, n - 1), bits[t] its word -- bit c set iff node 32 t + c is free of the map.
void launch_base_map(int grid, hipStream_t st, const RobotDev* rb, SceneDev sc, const MapCfg* mc, LatticeDev lat,
                     int n_items, unsigned* counter, uint32_t* bits);
size_t lattice_kernels_private_bytes();

// The launches of edges_kernel (smp_edges.hip) and detours_kernel (smp_repair.hip); clearance_kernel's is in
// smp_clearance.h.  Workgroups draw their items from *counter, zeroed on the stream before the launch.
//   edges:   item t is edge order[t]; first_invalid[e] = index of edge e's first colliding point, -1 if all M + 1 are
//            free;
//   detours: item i = (gap i / samples, sample i % samples), out[i] is its result.
struct DetourArgs {
  int n_items, samples;  // items = gaps x samples
  int n_seg;             // num_traj_segments
  int max_points;        // SMP_EDGE_MAX_POINTS: a leg of more points makes its item blocked
  int self, map;
  unsigned round;
  unsigned long long seed;
  double step, h;        // step_factor, half width of the round
};
void launch_edges(int grid, hipStream_t st, const RobotDev* rb, SceneDev sc, const MapCfg* mc, const EdgeDev* edges,
                  const int* order, int n, int self, int map, unsigned* counter, int* first_invalid);
void launch_detours(int grid, hipStream_t st, const RobotDev* rb, SceneDev sc, const MapCfg* mc, const GapDev* gaps,
                    DetourArgs args, unsigned* counter, DetourDev* out);
size_t edges_kernels_private_bytes();
size_t repair_kernels_private_bytes();

// The private segment (scratch) of a kernel, for the stack limit smp_planner_create raises; 0 if it cannot be read.
template <typename K>
size_t kernel_private_bytes(K* kernel) {
  hipFuncAttributes fa;
  if (hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(kernel)) != hipSuccess) return 0;
  return (size_t)fa.localSizeBytes;
}

// The work loop of a pass: the workgroup takes one item at a time from an atomic ticket counter (zeroed on the stream
// before the launch) until the tickets reach n_items.  The counter is only a ticket dispenser: no workgroup reads what
// another wrote, so no release / acquire is needed.
//   work(slot)         the item's work, run by all threads with a wave-uniform slot; it returns what commit stores.
//                      Every thread must pass at least one barrier in it: that is what lets thread 0 draw the next
//                      ticket into the slot the others have read.  What work keeps in LDS across its barriers is safe
//                      from the next item's work behind the barrier of the loop itself;
//   commit(slot, done) thread 0 alone: the stores of the item's result.
// Thread 0's work of one round -- the result of the item just done and the next ticket -- is one block followed by a
// barrier, and the slot reaches the loop condition through readfirstlane.  This shape is not free to change: with a
// ticket drawn at the loop's head and the result stored at its end, hipcc threaded thread 0 from the one block into the
// other across the back edge and let the other 63 lanes of its wavefront run on to the next barrier without it; the
// tiles' wave scans then read a dead lane, an illegal access on the GPU.
template <typename Work, typename Commit>
__device__ __forceinline__ void ticket_loop(unsigned* __restrict__ counter, unsigned n_items, Work&& work,
                                            Commit&& commit) {
  __shared__ unsigned s_slot;
  const int tid = threadIdx.x;
  if (tid == 0) s_slot = atomicAdd(counter, 1u);
  __syncthreads();
  unsigned slot = (unsigned)__builtin_amdgcn_readfirstlane((int)s_slot);
  while (slot < n_items) {
    const auto done = work(slot);
    // (every thread has read s_slot: it passed the barriers of work)
    if (tid == 0) {
      commit(slot, done);
      s_slot = atomicAdd(counter, 1u);
    }
    __syncthreads();
    slot = (unsigned)__builtin_amdgcn_readfirstlane((int)s_slot);
  }
}

// The edge walk.  One coordinate of an edge's step: the quotient first, then the product in edge_tile, no contraction,
// which for one hop is bit for bit connect_nodes' trajectory (oracle/smp_oracle.cpp:511-516).
__device__ __forceinline__ double edge_step(double a, double b, int M) { return (b - a) / (double)M; }

// Points base .. base + nc - 1 of the edge with start ea and step es into the tile, a coordinate per thread: nc is at
// most 64 (one ballot reads a tile), so the workgroup covers the tile in one trip.
__device__ __forceinline__ void edge_tile(double (*ql)[NJ], const double* ea, const double* es, int base, int nc) {
  static_assert(64 * NJ <= BLOCK, "a thread per coordinate of the largest tile");
  const int it = threadIdx.x;
  if (it < nc * NJ) {
    const int c = it / NJ, j = it - c * NJ;
    ql[c][j] = ea[j] + (double)(base + c) * es[j];
  }
}

// Nodes n0 .. n0 + nc - 1 of the lattice into the tile, a coordinate per thread (nc <= PASS_CT, one trip).
__device__ __forceinline__ void lattice_tile(double (*ql)[NJ], const LatticeDev& lat, long long n0, int nc) {
  static_assert(PASS_CT * NJ <= BLOCK, "a thread per coordinate of the tile");
  const int it = threadIdx.x;
  if (it < nc * NJ) {
    const int c = it / NJ, j = it - c * NJ;
    const long long n = n0 + c, row = n / lat.nx;
    ql[c][j] = lattice_coord(lat, (int)(n - row * lat.nx), (int)(row % lat.ny), (int)(row / lat.ny), j);
  }
}

// A free-map tile's word from the mask of its blocked configurations: bit c set iff c < nc and configuration c is free.
__device__ __forceinline__ uint32_t lattice_word(unsigned long long blocked, int nc) {
  const uint32_t all = nc >= 32 ? 0xffffffffu : ((1u << nc) - 1u);
  return ~(uint32_t)blocked & all;
}

#endif  // __HIPCC__

}  // namespace smp
#endif  // SMP_PASS_H
