// Batched one-via detours (gfx950): for a table of gaps (a, b) and S samples per gap, item (g, s) draws a via
// configuration v around the gap's centre and checks the two legs a -> v and v -> b densely, each at the density rule
// of the dense edge checks (DESIGN.md "Path repair").  smp_repair_path picks, per gap, the cheapest free item.
//
// Everything an item needs is formed on the device: v (eight lanes, Philox draws of smp_math.h, every operation
// rounded on its own), both legs' point counts (fp64 sqrt, division and ceil are correctly rounded on gfx950, as
// step_towards relies on) and the points, a[j] + k * ((b[j] - a[j]) / M) as edges_kernel forms them.  Only free /
// blocked is reported, so the tiles run in the order that meets an obstacle soonest: the leg v -> b from v on, then
// the leg a -> v from v back to a.
//
// One workgroup takes one item at a time in the passes' work loop (ticket_loop, smp_pass.h); the density rule
// (edge_segments) and the edge walk are that header's too.
#include <hip/hip_runtime.h>

#include "smp_collide.h"
#include "smp_math.h"
#include "smp_pass.h"
#include "smp_types.h"

namespace smp {

template <int CT>
__global__ void __launch_bounds__(BLOCK) detours_kernel(const RobotDev* __restrict__ rb, SceneDev sc,
                                                        const MapCfg* __restrict__ mc,
                                                        const GapDev* __restrict__ gaps, DetourArgs A,
                                                        unsigned* __restrict__ counter, DetourDev* __restrict__ out) {
  static_assert(CT <= 64, "one ballot finds a tile's colliding points");
  __shared__ RobotDev s_rb;
  __shared__ MapCfg s_mc;
  __shared__ TileLds<CT> L;
  __shared__ double ql[CT][NJ];
  __shared__ double ea[2][NJ], es[2][NJ];  // start and step of the legs a -> v (0) and v -> b (1): ea[1] is v
  __shared__ double eb[NJ];                // b
  const int tid = threadIdx.x;
  stage_model(rb, mc, &s_rb, &s_mc);  // (ends with a barrier)
  struct Done { int M1, M2, blocked; };
  ticket_loop(
      counter, (unsigned)A.n_items,
      [&](unsigned slot) {
        const unsigned gi = slot / (unsigned)A.samples, s = slot - gi * (unsigned)A.samples;
        if (tid < NJ) {
          const double a = gaps[gi].a[tid], b = gaps[gi].b[tid];
          const double c = 0.5 * (a + b);
          const double u = u01(A.seed, gaps[gi].g, A.round, s, 0u, (uint32_t)tid);
          const double t = 2.0 * u - 1.0;
          double v = c + t * A.h;
          if (tid >= 2) {  // the arm's joint limits; x and y belong to a query's environment, not to the planner
            const double lo = s_rb.q_min[tid], hi = s_rb.q_max[tid];
            v = v < lo ? lo : v;
            v = v > hi ? hi : v;
          }
          ea[0][tid] = a;
          ea[1][tid] = v;
          eb[tid] = b;
        }
        __syncthreads();
        // both legs' densities, the same in every thread (sums for j ascending)
        double sr0 = 0.0, sp0 = 0.0, sr1 = 0.0, sp1 = 0.0;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const double d0 = ea[1][j] - ea[0][j], d1 = eb[j] - ea[1][j];
          if (s_rb.rev[j]) {
            sr0 += d0 * d0;
            sr1 += d1 * d1;
          } else {
            sp0 += d0 * d0;
            sp1 += d1 * d1;
          }
        }
        const int M1 = __builtin_amdgcn_readfirstlane(edge_segments(sr0, sp0, A.step, A.n_seg, A.max_points));
        const int M2 = __builtin_amdgcn_readfirstlane(edge_segments(sr1, sp1, A.step, A.n_seg, A.max_points));
        int blocked = (M1 == 0 || M2 == 0) ? 1 : 0;
        if (!blocked) {
          if (tid < NJ) {
            es[0][tid] = edge_step(ea[0][tid], ea[1][tid], M1);
            es[1][tid] = edge_step(ea[1][tid], eb[tid], M2);
          }
          __syncthreads();
          const int T1 = (M1 + CT) / CT, T2 = (M2 + CT) / CT;  // tiles of M + 1 points
          for (int t = 0; t < T1 + T2 && !blocked; ++t) {
            const int leg = t < T2 ? 1 : 0;
            const int base = leg ? t * CT : (T1 - 1 - (t - T2)) * CT;
            const int nc = min(CT, (leg ? M2 : M1) + 1 - base);
            edge_tile(ql, ea[leg], es[leg], base, nc);
            __syncthreads();
            collide_tile<CT>(&s_rb, sc, &s_mc, nc, ql, A.self, A.map, L);  // (ends with a barrier)
            const unsigned long long hit = __ballot((tid & 63) < nc && L.coll[tid & 63] != 0);  // the same in every wave
            if (hit) blocked = 1;
            __syncthreads();  // coll and ql are rewritten by the next tile
          }
        }
        return Done{M1, M2, blocked};
      },
      [&](unsigned slot, const Done& d) {
        DetourDev* o = out + slot;
#pragma unroll
        for (int j = 0; j < NJ; ++j) o->v[j] = ea[1][j];
        o->M1 = d.M1;
        o->M2 = d.M2;
        o->free = d.blocked ? 0 : 1;
        o->pad = 0;
      });
}

size_t repair_kernels_private_bytes() { return kernel_private_bytes(&detours_kernel<PASS_CT>); }

void launch_detours(int grid, hipStream_t st, const RobotDev* rb, SceneDev sc, const MapCfg* mc, const GapDev* gaps,
                    DetourArgs args, unsigned* counter, DetourDev* out) {
  hipLaunchKernelGGL(detours_kernel<PASS_CT>, dim3(grid), dim3(BLOCK), 0, st, rb, sc, mc, gaps, args, counter, out);
}

}  // namespace smp
