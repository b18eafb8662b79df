// The base's free map (gfx950): the free space of the base with the arm held fixed, as a slice of C-space -- every node
// (ix, iy, t) of a lattice is one configuration, and the batch checker's tile answers each (include/smp_gpu.h "Far
// goals").
//
// One workgroup takes one tile of PASS_CT = 32 consecutive nodes at a time in the passes' work loop (ticket_loop,
// smp_pass.h).  The tile's configurations are formed in LDS from the node number, a coordinate per thread
// (lattice_tile: integer to double, product, sum, each rounded on its own -- no table of configurations is uploaded);
// collide_tile checks them against the map alone; one ballot makes the tile's word, and thread 0 stores it.  A word
// belongs to exactly one ticket, so the store is a plain one; no workgroup reads what another wrote.
// The variant with a map margin is margin_base_map_kernel (smp_margin.hip).
#include <hip/hip_runtime.h>

#include "smp_collide.h"
#include "smp_math.h"
#include "smp_pass.h"
#include "smp_types.h"

namespace smp {

__global__ void __launch_bounds__(BLOCK) base_map_kernel(const RobotDev* __restrict__ rb, SceneDev sc,
                                                         const MapCfg* __restrict__ mc, LatticeDev lat, int n_items,
                                                         unsigned* __restrict__ counter, uint32_t* __restrict__ bits) {
  __shared__ RobotDev s_rb;
  __shared__ MapCfg s_mc;
  __shared__ TileLds<PASS_CT> L;
  __shared__ double ql[PASS_CT][NJ];
  const int tid = threadIdx.x;
  stage_model(rb, mc, &s_rb, &s_mc);  // (ends with a barrier)
  ticket_loop(
      counter, (unsigned)n_items,
      [&](unsigned slot) {
        const long long n0 = (long long)slot * PASS_CT;
        const int nc = __builtin_amdgcn_readfirstlane((int)min((long long)PASS_CT, lat.n - n0));
        lattice_tile(ql, lat, n0, nc);
        __syncthreads();
        collide_tile<PASS_CT>(&s_rb, sc, &s_mc, nc, ql, 0, 1, L);  // (ends with a barrier)
        const unsigned long long hit = __ballot((tid & 63) < nc && L.coll[tid & (PASS_CT - 1)] != 0);  // the same in every wave
        __syncthreads();  // coll and ql are rewritten by the next tile
        return lattice_word(hit, nc);
      },
      [&](unsigned slot, uint32_t word) { bits[slot] = word; });
}

size_t lattice_kernels_private_bytes() { return kernel_private_bytes(&base_map_kernel); }

void launch_base_map(int grid, hipStream_t st, const RobotDev* rb, SceneDev sc, const MapCfg* mc, LatticeDev lat,
                     int n_items, unsigned* counter, uint32_t* bits) {
  hipLaunchKernelGGL(base_map_kernel, dim3(grid), dim3(BLOCK), 0, st, rb, sc, mc, lat, n_items, counter, bits);
}

}  // namespace smp
