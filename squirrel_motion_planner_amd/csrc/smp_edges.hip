// Batched dense edge checks (gfx950): isEdgeValid (birrt_star.cpp:6864-6895) for a table of edges of very different
// lengths, each interpolated at the planner's own collision density (DESIGN.md "Path shortcutting").
//
// The host forms every edge's point count (make_edge in smp_paths.cpp: M = num_traj_segments * hops of at most one
// planner step, smp_pass.h's edge_segments) and an order of the table, longest first; the kernel interpolates.  Point k
// of an edge a -> b is a[j] + k * ((b[j] - a[j]) / M) -- the quotient first, then the product, no contraction -- which
// for one hop is bit for bit connect_nodes' trajectory (oracle/smp_oracle.cpp:511-516).
//
// One workgroup takes one edge at a time from an atomic work counter (the M of one call span 20 to a few thousand, so
// a static split would leave most of the machine idle behind the longest edges; longest-first keeps the tail short),
// writes CT consecutive points into LDS, runs the batch checker's collide_tile on them and stops at the first tile
// that holds a colliding point.  A tile checks all of its points, so the lowest colliding index of that tile is the
// edge's true first invalid point.  The work loop and the edge walk are smp_pass.h's (ticket_loop, edge_step,
// edge_tile).
#include <hip/hip_runtime.h>

#include "smp_collide.h"
#include "smp_math.h"
#include "smp_pass.h"
#include "smp_types.h"

namespace smp {

template <int CT>
__global__ void __launch_bounds__(BLOCK) edges_kernel(const RobotDev* __restrict__ rb, SceneDev sc,
                                                      const MapCfg* __restrict__ mc,
                                                      const EdgeDev* __restrict__ edges,
                                                      const int* __restrict__ order, int n, int self, int map,
                                                      unsigned* __restrict__ counter, int* __restrict__ first_invalid) {
  static_assert(CT <= 64, "one ballot finds a tile's first colliding point");
  __shared__ RobotDev s_rb;
  __shared__ MapCfg s_mc;
  __shared__ TileLds<CT> L;
  __shared__ double ql[CT][NJ];
  __shared__ double ea[NJ], es[NJ];  // the edge's start and its step (b - a) / M
  const int tid = threadIdx.x;
  stage_model(rb, mc, &s_rb, &s_mc);  // (ends with a barrier)
  struct Done { int e, first; };
  ticket_loop(
      counter, (unsigned)n,
      [&](unsigned slot) {
        const int e = __builtin_amdgcn_readfirstlane(order[slot]);
        const int M = __builtin_amdgcn_readfirstlane(edges[e].M);
        if (tid < NJ) {
          const double a = edges[e].a[tid], b = edges[e].b[tid];
          ea[tid] = a;
          es[tid] = edge_step(a, b, M);
        }
        __syncthreads();
        int first = -1;
        for (int base = 0; base <= M && first < 0; base += CT) {
          const int nc = min(CT, M + 1 - base);
          edge_tile(ql, ea, es, base, nc);
          __syncthreads();
          collide_tile<CT>(&s_rb, sc, &s_mc, nc, ql, self, map, L);  // (ends with a barrier)
          const unsigned long long hit = __ballot((tid & 63) < nc && L.coll[tid & 63] != 0);  // the same in every wave
          if (hit) first = base + (int)__builtin_ctzll(hit);
          __syncthreads();  // coll and ql are rewritten by the next tile
        }
        return Done{e, first};
      },
      [&](unsigned, const Done& d) { first_invalid[d.e] = d.first; });
}

size_t edges_kernels_private_bytes() { return kernel_private_bytes(&edges_kernel<PASS_CT>); }

void launch_edges(int grid, hipStream_t st, const RobotDev* rb, SceneDev sc, const MapCfg* mc, const EdgeDev* edges,
                  const int* order, int n, int self, int map, unsigned* counter, int* first_invalid) {
  hipLaunchKernelGGL(edges_kernel<PASS_CT>, dim3(grid), dim3(BLOCK), 0, st, rb, sc, mc, edges, order, n, self, map,
                     counter, first_invalid);
}

}  // namespace smp
