// The cost field over the base's free map (gfx950): cost[n] = the least left-to-right fp64 sum of step weights over the
// routes source -> n in smp_base_route's graph, by tile-resident relaxation (smp_field.h; include/smp_gpu.h "Far goals",
// smp_base_cost_field).
//
// A round is one launch of field_round_kernel, one workgroup per tile.  A tile whose activity flag of the round's parity
// is set loads its nodes' and its one-node halo's costs and free bits into LDS, runs Jacobi pull sweeps there until one
// changes nothing (or FIELD_SWEEPS of them), stores the nodes it lowered, and sets the next round's flags: of the
// neighbours whose halo holds a node it lowered, and its own when it stopped at the sweep bound.  Values only ever fall
// from +inf, so the fixed point is smp_base_route's field whatever the order (smp_field.h).
//
// Between workgroups.  Only its owner stores a node.  A halo load may meet the owner's old or new value of the same
// launch; both are upper bounds a route realises, and the owner flags the reader for the next round when it lowers the
// node, so a stale load costs a round and nothing else.  Nothing here relies on one workgroup seeing another's store
// within a launch -- not across XCDs, whose L2s are not coherent, and not within one: what a round needs it gets from the
// launches before it, in stream order.  The cost array is read and written across tiles with 8-byte relaxed agent-scope
// atomics only so that no load is torn; the flags likewise.  No kernel waits on another workgroup: there is no grid
// barrier, no spin and no cooperative launch, and every loop has a compile-time bound.
#include <hip/hip_runtime.h>

#include "smp_field.h"

namespace smp {

namespace {

constexpr int SX = FIELD_BX + 2, SY = FIELD_BY + 2, SZ = FIELD_BT + 2;
constexpr int CELLS = SX * SY * SZ;

__device__ __forceinline__ double load_cost(const double* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void store_cost(double* p, double v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned load_flag(const unsigned* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void store_flag(unsigned* p, unsigned v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ bool free_bit(const uint32_t* bits, long long n) { return (bits[n >> 5] >> (n & 31)) & 1u; }

}  // namespace

__global__ void __launch_bounds__(256) field_init_kernel(FieldGrid g, long long src, double* __restrict__ cost,
                                                         unsigned* __restrict__ active, FieldStats* __restrict__ stats) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long n_nodes = (long long)g.nx * g.ny * g.nt, n_tiles = field_n_tiles(g);
  if (i < n_nodes) cost[i] = i == src ? 0.0 : __builtin_inf();
  if (i < 2 * n_tiles) {
    const long long layer = (long long)g.nx * g.ny;
    const int t = (int)(src / layer), iy = (int)((src - t * layer) / g.nx), ix = (int)(src % g.nx);
    // (parity 0 is the first n_tiles flags; the second n_tiles numbers are no tile's, so parity 1 starts clear)
    active[i] = (i < n_tiles && field_starts_active(g, ix, iy, t, i)) ? 1u : 0u;
  }
  if (i == 0) {
    stats->n_reached = stats->n_settled = stats->max_bits = 0;
    stats->cost_to = __builtin_inf();
    stats->n_chain = 0;
    stats->pad = 0;
  }
}

__global__ void __launch_bounds__(FIELD_THREADS) field_round_kernel(FieldGrid g, const uint32_t* __restrict__ bits,
                                                                    double* cost, unsigned* active, int parity,
                                                                    unsigned* __restrict__ changed) {
  __shared__ double s_c[SZ][SY][SX];
  __shared__ unsigned char s_f[SZ][SY][SX];
  __shared__ unsigned s_dirs;
  const int tid = threadIdx.x, tile = blockIdx.x;
  const long long n_tiles = field_n_tiles(g);
  unsigned* cur = active + (parity ? n_tiles : 0);
  unsigned* nxt = active + (parity ? 0 : n_tiles);
  // Every thread reads the tile's flag itself.  Nothing stores cur[tile] in this launch but this workgroup's thread 0,
  // and it does so at the kernel's end, behind barriers that no wave passes before every wave has arrived, so before
  // every wave has made this load: all waves read the same value, the return is the whole workgroup's, and
  // readfirstlane makes the branch around the barriers a scalar one.
  const int on = __builtin_amdgcn_readfirstlane((int)load_flag(&cur[tile]));
  if (!on) return;
  const int a = tile % g.tx, b = (tile / g.tx) % g.ty, c = tile / (g.tx * g.ty);
  int lo[3], ext[3];
  field_tile_range(g, a, b, c, lo, ext);
  const bool inside = field_wraps_inside(g);

  // the tile and its halo into LDS: a cell outside the lattice, or of a halo layer this tile does not have, is blocked
  for (int i = tid; i < CELLS; i += FIELD_THREADS) {
    const int cz = i / (SY * SX), r = i - cz * (SY * SX), cy = r / SX, cx = r - cy * SX;
    const int gx = lo[0] - 1 + cx, gy = lo[1] - 1 + cy;
    int gz = lo[2] - 1 + cz;
    bool ok = gx >= 0 && gx < g.nx && gy >= 0 && gy < g.ny && cz <= ext[2] + 1;
    if (cz == 0 || cz == ext[2] + 1) {
      if (inside) ok = false;
      else if (g.wrap) gz = (gz + g.nt) % g.nt;
    }
    ok = ok && gz >= 0 && gz < g.nt;
    double v = __builtin_inf();
    bool f = false;
    if (ok) {
      const long long n = field_node(g, gx, gy, gz);
      f = free_bit(bits, n);
      if (f) v = load_cost(&cost[n]);
    }
    s_c[cz][cy][cx] = v;
    s_f[cz][cy][cx] = f ? 1 : 0;
  }
  if (tid == 0) s_dirs = 0;
  __syncthreads();

  // this thread's column: the edges of its free nodes as masks (bits 0..3 the axis steps -y, -x, +x, +y; 4..7 the
  // diagonals (-x,-y), (+x,-y), (-x,+y), (+x,+y); 8, 9 the headings below and above) and the costs they came with
  const int lx = tid % FIELD_BX, ly = tid / FIELD_BX;
  const int X = lx + 1, Y = ly + 1;
  const bool owner = lx < ext[0] && ly < ext[1];
  unsigned mask[FIELD_BT];
  double c0[FIELD_BT];
#pragma unroll
  for (int k = 0; k < FIELD_BT; ++k) {
    const int Z = k + 1;
    unsigned m = 0;
    c0[k] = __builtin_inf();
    if (owner && k < ext[2] && s_f[Z][Y][X]) {
      const int zm = (inside && k == 0) ? ext[2] : Z - 1, zp = (inside && k == ext[2] - 1) ? 1 : Z + 1;
      const bool ym = s_f[Z][Y - 1][X], xm = s_f[Z][Y][X - 1], xp = s_f[Z][Y][X + 1], yp = s_f[Z][Y + 1][X];
      m = (ym ? 1u : 0u) | (xm ? 2u : 0u) | (xp ? 4u : 0u) | (yp ? 8u : 0u);
      if (xm && ym && s_f[Z][Y - 1][X - 1]) m |= 16u;
      if (xp && ym && s_f[Z][Y - 1][X + 1]) m |= 32u;
      if (xm && yp && s_f[Z][Y + 1][X - 1]) m |= 64u;
      if (xp && yp && s_f[Z][Y + 1][X + 1]) m |= 128u;
      if (s_f[zm][Y][X]) m |= 256u;
      if (s_f[zp][Y][X]) m |= 512u;
      m |= 1024u;  // (a free node of this thread, with or without edges)
      c0[k] = s_c[Z][Y][X];
    }
    mask[k] = m;
  }

  int more = 1;
  for (int s = 0; s < FIELD_SWEEPS; ++s) {
    double nv[FIELD_BT];
    unsigned low = 0;
#pragma unroll
    for (int k = 0; k < FIELD_BT; ++k) {
      const unsigned m = mask[k];
      if (!(m & 1023u)) continue;
      const int Z = k + 1;
      const int zm = (inside && k == 0) ? ext[2] : Z - 1, zp = (inside && k == ext[2] - 1) ? 1 : Z + 1;
      const double was = s_c[Z][Y][X];
      double best = was;
      auto pull = [&](unsigned bit, double u, double w) {
        const double v = u + w;
        if ((m & bit) && v < best) best = v;
      };
      pull(1u, s_c[Z][Y - 1][X], g.w_axis);
      pull(2u, s_c[Z][Y][X - 1], g.w_axis);
      pull(4u, s_c[Z][Y][X + 1], g.w_axis);
      pull(8u, s_c[Z][Y + 1][X], g.w_axis);
      pull(16u, s_c[Z][Y - 1][X - 1], g.w_diag);
      pull(32u, s_c[Z][Y - 1][X + 1], g.w_diag);
      pull(64u, s_c[Z][Y + 1][X - 1], g.w_diag);
      pull(128u, s_c[Z][Y + 1][X + 1], g.w_diag);
      pull(256u, s_c[zm][Y][X], g.w_turn);
      pull(512u, s_c[zp][Y][X], g.w_turn);
      nv[k] = best;
      if (best < was) low |= 1u << k;
    }
    __syncthreads();  // every pull of this sweep has read
#pragma unroll
    for (int k = 0; k < FIELD_BT; ++k)
      if ((low >> k) & 1u) s_c[k + 1][Y][X] = nv[k];
    more = __builtin_amdgcn_readfirstlane(__syncthreads_or((int)low));
    if (!more) break;
  }

  // the nodes this run lowered go back, and the neighbours whose halo holds one of them run next round
  unsigned dirs = 0;
  int lowered = 0;
#pragma unroll
  for (int k = 0; k < FIELD_BT; ++k) {
    if (!mask[k]) continue;
    const double fin = s_c[k + 1][Y][X];
    if (fin < c0[k]) {
      store_cost(&cost[field_node(g, lo[0] + lx, lo[1] + ly, lo[2] + k)], fin);
      lowered = 1;
      dirs |= field_dir_mask(ext, lx, ly, k);
    }
  }
  if (dirs) atomicOr(&s_dirs, dirs);
  const int any = __syncthreads_or(lowered);
  if (tid < FIELD_DIRS && ((s_dirs >> tid) & 1u)) {
    const int to = field_dir_tile(g, a, b, c, tid);
    if (to >= 0) store_flag(&nxt[to], 1u);
  }
  if (tid == 0) {
    store_flag(&cur[tile], 0u);  // (this round's flag is used up; the slot is the round after next's)
    if (more) store_flag(&nxt[tile], 1u);  // stopped at the sweep bound: not yet at its own fixed point
    if (any) atomicAdd(changed, 1u);
  }
}

__global__ void __launch_bounds__(256) field_stats_kernel(FieldGrid g, const double* __restrict__ cost, long long to,
                                                          FieldStats* __restrict__ stats) {
  const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long n_nodes = (long long)g.nx * g.ny * g.nt;
  const double ct = to >= 0 ? cost[to] : __builtin_inf();
  const double v = n < n_nodes ? cost[n] : __builtin_inf();
  const bool reached = v < __builtin_inf();
  const bool settled = reached && (v < ct || (v == ct && n <= to));
  unsigned long long mx = reached ? (unsigned long long)__double_as_longlong(v) : 0ull;
  const unsigned long long nr = __popcll(__ballot(reached)), ns = __popcll(__ballot(settled));
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_down(mx, off);
    mx = o > mx ? o : mx;
  }
  if ((threadIdx.x & 63) == 0 && nr) {
    atomicAdd(&stats->n_reached, nr);
    if (ns) atomicAdd(&stats->n_settled, ns);
    atomicMax(&stats->max_bits, mx);
  }
  if (n == to) stats->cost_to = v;
}

__global__ void __launch_bounds__(256) field_parents_kernel(FieldGrid g, const uint32_t* __restrict__ bits,
                                                            const double* __restrict__ cost,
                                                            int32_t* __restrict__ parent) {
  const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long layer = (long long)g.nx * g.ny;
  if (n >= layer * g.nt) return;
  const int t = (int)(n / layer), iy = (int)((n - t * layer) / g.nx), ix = (int)(n % g.nx);
  parent[n] = (int32_t)field_parent_rule(
      g, [&](int x, int y, int z) { return free_bit(bits, field_node(g, x, y, z)); },
      [&](long long u) { return cost[u]; }, ix, iy, t);
}

// One wave; its first lane follows parent[] from `to` until it stands on `from`.
__global__ void __launch_bounds__(64) field_chain_kernel(FieldGrid g, const int32_t* __restrict__ parent, long long from,
                                                         long long to, int32_t* __restrict__ chain,
                                                         FieldStats* __restrict__ stats) {
  if (threadIdx.x != 0) return;
  const long long n_nodes = (long long)g.nx * g.ny * g.nt;
  int count = 0;
  long long v = to;
  if (to != from && parent[to] < 0) {
    stats->n_chain = 0;
    return;
  }
  for (int i = 0; i < SMP_LATTICE_MAX_NODES; ++i) {
    if (count >= n_nodes) {  // (a chain visits a node once: more is no chain)
      count = -1;
      break;
    }
    chain[count++] = (int32_t)v;
    if (v == from) break;
    v = parent[v];
    if (v < 0) {
      count = -1;
      break;
    }
  }
  stats->n_chain = count;
}

size_t field_kernels_private_bytes() {
  size_t need = kernel_private_bytes(&field_init_kernel);
  need = std::max(need, kernel_private_bytes(&field_round_kernel));
  need = std::max(need, kernel_private_bytes(&field_stats_kernel));
  need = std::max(need, kernel_private_bytes(&field_parents_kernel));
  need = std::max(need, kernel_private_bytes(&field_chain_kernel));
  return need;
}

static unsigned blocks_for(long long n) { return (unsigned)((n + 255) / 256); }

void launch_field_init(hipStream_t st, FieldGrid g, long long src, double* cost, unsigned* active, FieldStats* stats) {
  const long long n = std::max((long long)g.nx * g.ny * g.nt, 2 * field_n_tiles(g));
  hipLaunchKernelGGL(field_init_kernel, dim3(blocks_for(n)), dim3(256), 0, st, g, src, cost, active, stats);
}

void launch_field_round(hipStream_t st, FieldGrid g, const uint32_t* bits, double* cost, unsigned* active, int parity,
                        unsigned* changed) {
  hipLaunchKernelGGL(field_round_kernel, dim3((unsigned)field_n_tiles(g)), dim3(FIELD_THREADS), 0, st, g, bits, cost,
                     active, parity, changed);
}

void launch_field_stats(hipStream_t st, FieldGrid g, const double* cost, long long to, FieldStats* stats) {
  hipLaunchKernelGGL(field_stats_kernel, dim3(blocks_for((long long)g.nx * g.ny * g.nt)), dim3(256), 0, st, g, cost, to,
                     stats);
}

void launch_field_parents(hipStream_t st, FieldGrid g, const uint32_t* bits, const double* cost, int32_t* parent) {
  hipLaunchKernelGGL(field_parents_kernel, dim3(blocks_for((long long)g.nx * g.ny * g.nt)), dim3(256), 0, st, g, bits,
                     cost, parent);
}

void launch_field_chain(hipStream_t st, FieldGrid g, const int32_t* parent, long long from, long long to, int32_t* chain,
                        FieldStats* stats) {
  hipLaunchKernelGGL(field_chain_kernel, dim3(1), dim3(64), 0, st, g, parent, from, to, chain, stats);
}

}  // namespace smp
