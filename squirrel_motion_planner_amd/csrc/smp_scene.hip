// Device build of a planner's scene from occupied octomap keys (smp_planner_set_scene_keys, DESIGN.md "Scene
// build"): what scene_from_keys + smp_planner_set_scene derive on one host thread -- occupancy bits, 4x4x4 bricks,
// the 3x3x3 dilation, the exact squared EDT, its byte copy and the primitives' 2-D slab fields -- as integer passes
// over the dense grid, bit for bit the host's arrays.
//
// Exactness.  The host EDT (edt_squared) works in doubles that only ever hold integers or +inf, so integer
// arithmetic gives the same numbers, and it ends with min(f, 65535).  Every pass here saturates at 65535:
// with c(t) = min(t, 65535), c is monotone and c(c(a) + b) = c(a + b) for a, b >= 0, so a minimum over saturated
// sums equals the saturated minimum over the true sums, and a line without any set cell (the host's +inf) stays
// 65535 through every later pass.  The field therefore lives in the planner's uint16 d2 array from the first pass
// on, updated in place (each workgroup owns whole lines and stages them in LDS before it writes).
//
// Per line an outward scan: cell q starts at best = f[q] and looks at f[q - d] + d^2, f[q + d] + d^2 for d = 1, 2,
// ... while d^2 < best; no candidate further out can win, and best <= 65535 bounds d by 255.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "smp_scene.h"

namespace smp {

namespace {

constexpr int SB = 256;  // threads per workgroup (4 wavefronts)
constexpr unsigned SAT = 65535u;
constexpr size_t LDS_MAX = 64 * 1024;  // dynamic LDS a launch may ask for without opting in to more
typedef unsigned long long u64;

extern __shared__ __align__(16) unsigned char scene_smem[];

inline int grid_for(long long items) {
  const long long b = (items + SB - 1) / SB;
  return (int)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

// Occupancy bits from the keys (x-major rows of wx 64-bit words, SceneHost::bits).  Duplicate keys set the same bit.
__global__ __launch_bounds__(SB) void scene_scatter_kernel(const uint16_t* __restrict__ keys, long long n, int kx,
                                                           int ky, int kz, int nx, int ny, int nz, int wx, u64* bits) {
  for (long long i = (long long)blockIdx.x * SB + threadIdx.x; i < n; i += (long long)gridDim.x * SB) {
    const int x = (int)keys[3 * i] - kx, y = (int)keys[3 * i + 1] - ky, z = (int)keys[3 * i + 2] - kz;
    if ((unsigned)x >= (unsigned)nx || (unsigned)y >= (unsigned)ny || (unsigned)z >= (unsigned)nz) continue;
    atomicOr(&bits[((size_t)z * ny + y) * wx + (x >> 6)], 1ull << (x & 63));
  }
}

// 4x4x4 bricks in build_bricks' layout (bit (z&3)*16 + (y&3)*4 + (x&3)); every brick is written.  The number of
// distinct occupied cells is the bricks' popcount: one atomic add per wavefront.
__global__ __launch_bounds__(SB) void scene_bricks_kernel(const u64* __restrict__ bits, int ny, int nz, int wx, int bnx,
                                                          int bny, int bnz, u64* __restrict__ bricks, u64* count) {
  const long long nb = (long long)bnx * bny * bnz;
  unsigned cnt = 0;
  for (long long b = (long long)blockIdx.x * SB + threadIdx.x; b < nb; b += (long long)gridDim.x * SB) {
    const int bi = (int)(b % bnx);
    const long long t = b / bnx;
    const int bj = (int)(t % bny), bk = (int)(t / bny);
    u64 w = 0;
    for (int z = 0; z < 4 && 4 * bk + z < nz; ++z)
      for (int y = 0; y < 4 && 4 * bj + y < ny; ++y) {
        const u64 row = bits[((size_t)(4 * bk + z) * ny + (4 * bj + y)) * wx + (bi >> 4)];
        w |= ((row >> ((bi & 15) * 4)) & 0xFull) << ((z << 4) | (y << 2));
      }
    bricks[b] = w;
    cnt += (unsigned)__popcll(w);
  }
  for (int o = 32; o; o >>= 1) cnt += __shfl_down(cnt, o, 64);
  if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(count, (u64)cnt);
}

// OR of the layers k0[p] .. k1[p] of the occupancy for every primitive p (prim_slabs' projection), as bit rows.
__global__ __launch_bounds__(SB) void scene_project_kernel(const u64* __restrict__ bits, int ny, int nz, int wx,
                                                           int n_prim, const int* __restrict__ k01,
                                                           u64* __restrict__ out) {
  const long long nw = (long long)wx * ny * n_prim;
  for (long long idx = (long long)blockIdx.x * SB + threadIdx.x; idx < nw; idx += (long long)gridDim.x * SB) {
    const int w = (int)(idx % wx);
    const long long t = idx / wx;
    const int j = (int)(t % ny), p = (int)(t / ny);
    int k0 = k01[2 * p], k1 = k01[2 * p + 1];
    k0 = k0 < 0 ? 0 : k0;
    k1 = k1 > nz - 1 ? nz - 1 : k1;
    u64 v = 0;
    for (int k = k0; k <= k1; ++k) v |= bits[((size_t)k * ny + j) * wx + w];
    out[idx] = v;
  }
}

// Box dilation on bit rows: +-1 along x and y, and +-zr along the layer axis (1: the 3x3x3 dilation of the grid; 0:
// the slabs' 3x3, their layers being independent planes), clipped at the grid's faces as box_gap_squared clips it.
__global__ __launch_bounds__(SB) void scene_dilate_kernel(const u64* __restrict__ in, int nx, int ny, int nl, int wx,
                                                          int zr, u64* __restrict__ out) {
  const long long nw = (long long)wx * ny * nl;
  for (long long idx = (long long)blockIdx.x * SB + threadIdx.x; idx < nw; idx += (long long)gridDim.x * SB) {
    const int w = (int)(idx % wx);
    const long long t = idx / wx;
    const int j = (int)(t % ny), l = (int)(t / ny);
    u64 c = 0, lo = 0, hi = 0;  // this word, the word before and the word after, ORed over the neighbouring rows
    for (int dl = -zr; dl <= zr; ++dl) {
      const int ll = l + dl;
      if (ll < 0 || ll >= nl) continue;
      for (int dj = -1; dj <= 1; ++dj) {
        const int jj = j + dj;
        if (jj < 0 || jj >= ny) continue;
        const u64* row = in + ((size_t)ll * ny + jj) * wx;
        c |= row[w];
        if (w > 0) lo |= row[w - 1];
        if (w + 1 < wx) hi |= row[w + 1];
      }
    }
    u64 v = c | (c << 1) | (c >> 1) | (lo >> 63) | (hi << 63);
    if (w == wx - 1 && (nx & 63)) v &= (1ull << (nx & 63)) - 1;
    out[idx] = v;
  }
}

// EDT pass along x straight from the dilated bits: the distance to the nearest set bit of the row, found a word at a
// time in the row's words staged in LDS; 256 cells or more away (or no set bit) saturates.
__global__ __launch_bounds__(SB) void scene_edt_x_kernel(const u64* __restrict__ dil, int nx, int wx, long long rows,
                                                         uint16_t* __restrict__ f) {
  u64* srow = reinterpret_cast<u64*>(scene_smem);
  for (long long r = blockIdx.x; r < rows; r += gridDim.x) {
    __syncthreads();  // the previous row's readers are done
    for (int w = threadIdx.x; w < wx; w += SB) srow[w] = dil[(size_t)r * wx + w];
    __syncthreads();
    for (int i = threadIdx.x; i < nx; i += SB) {
      const int w = i >> 6, b = i & 63;
      int d = 256;
      u64 m = srow[w] >> b;
      if (m) {
        d = __builtin_ctzll(m);
      } else {
        for (int ww = w + 1; ww < wx && (ww << 6) - i < d; ++ww)
          if (srow[ww]) { d = (ww << 6) + __builtin_ctzll(srow[ww]) - i; break; }
      }
      m = srow[w] << (63 - b);
      if (m) {
        const int dl = __builtin_clzll(m);
        d = dl < d ? dl : d;
      } else {
        for (int ww = w - 1; ww >= 0 && i - ((ww << 6) + 63) < d; --ww)
          if (srow[ww]) {
            const int dl = i - ((ww << 6) + 63 - __builtin_clzll(srow[ww]));
            d = dl < d ? dl : d;
            break;
          }
      }
      f[(size_t)r * nx + i] = (uint16_t)(d >= 256 ? SAT : (unsigned)(d * d));
    }
  }
}

// EDT pass along y or z, in place.  A workgroup owns 2^txl neighbouring x columns of one plane: lanes run along x
// for the global loads and stores, the lines (L cells, ls elements apart) are staged in LDS.  fb (last pass of the
// grid only) receives the byte copy min(f, 255).
__global__ __launch_bounds__(SB) void scene_edt_line_kernel(uint16_t* __restrict__ f, int nx, int L, size_t ls,
                                                            size_t ps, int tiles, int txl, uint8_t* __restrict__ fb) {
  uint16_t* s = reinterpret_cast<uint16_t*>(scene_smem);
  const int tile = (int)(blockIdx.x % (unsigned)tiles);
  const size_t base = (size_t)(blockIdx.x / (unsigned)tiles) * ps;
  const int lx = threadIdx.x & ((1 << txl) - 1), r0 = threadIdx.x >> txl, rs = SB >> txl;
  const int x = (tile << txl) + lx;
  if (x < nx)
    for (int q = r0; q < L; q += rs) s[((size_t)q << txl) + lx] = f[base + (size_t)q * ls + x];
  __syncthreads();
  if (x >= nx) return;
  for (int q = r0; q < L; q += rs) {
    unsigned best = s[((size_t)q << txl) + lx];
    for (int d = 1; d < L && (unsigned)(d * d) < best; ++d) {
      const unsigned dd = (unsigned)(d * d);
      if (q - d >= 0) {
        const unsigned v = s[((size_t)(q - d) << txl) + lx] + dd;
        best = v < best ? v : best;
      }
      if (q + d < L) {
        const unsigned v = s[((size_t)(q + d) << txl) + lx] + dd;
        best = v < best ? v : best;
      }
    }
    const size_t c = base + (size_t)q * ls + x;
    f[c] = (uint16_t)best;
    if (fb) fb[c] = (uint8_t)(best < 255u ? best : 255u);
  }
}

// The byte copy min(f, 255) of a finished field (smp_planner_set_robot, when a robot swap makes the copy valid for a
// scene built without it): eight cells per work-item where the count allows, the tail cell by cell.
__global__ __launch_bounds__(SB) void scene_bytes_kernel(const uint16_t* __restrict__ f, long long n,
                                                         uint8_t* __restrict__ fb) {
  const long long n8 = n >> 3;
  for (long long i = (long long)blockIdx.x * SB + threadIdx.x; i < n8; i += (long long)gridDim.x * SB) {
    const uint4 v = reinterpret_cast<const uint4*>(f)[i];
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
    unsigned o[2] = {0u, 0u};
    for (int k = 0; k < 4; ++k) {
      const unsigned lo = w[k] & 0xffffu, hi = w[k] >> 16;
      o[k >> 1] |= ((lo < 255u ? lo : 255u) | ((hi < 255u ? hi : 255u) << 8)) << ((k & 1) * 16);
    }
    reinterpret_cast<uint2*>(fb)[i] = make_uint2(o[0], o[1]);
  }
  if (blockIdx.x == 0)
    for (long long c = (n8 << 3) + threadIdx.x; c < n; c += SB) fb[c] = (uint8_t)(f[c] < 255u ? f[c] : 255u);
}

// log2 of the widest x tile (64 .. 1 columns) whose L-cell lines fit the dynamic LDS; -1 if none does.
int tile_log2(int L) {
  for (int t = 6; t >= 0; --t)
    if (((size_t)L << t) * sizeof(uint16_t) <= LDS_MAX) return t;
  return -1;
}

hipError_t edt_lines(hipStream_t st, uint16_t* f, int nx, int L, size_t ls, size_t ps, long long planes, uint8_t* fb) {
  const int txl = tile_log2(L);
  const int tiles = (nx + (1 << txl) - 1) >> txl;
  hipLaunchKernelGGL(scene_edt_line_kernel, dim3((unsigned)(tiles * planes)), dim3(SB),
                     ((size_t)L << txl) * sizeof(uint16_t), st, f, nx, L, ls, ps, tiles, txl, fb);
  return hipGetLastError();
}

hipError_t edt_x(hipStream_t st, const u64* dil, int nx, int wx, long long rows, uint16_t* f) {
  const unsigned grid = (unsigned)(rows > 65536 * 4 ? 65536 * 4 : rows);
  hipLaunchKernelGGL(scene_edt_x_kernel, dim3(grid), dim3(SB), (size_t)wx * sizeof(u64), st, dil, nx, wx, rows, f);
  return hipGetLastError();
}

}  // namespace

bool scene_build_fits(int nx, int ny, int nz, int n_prim) {
  if (nx <= 0 || ny <= 0 || nz <= 0) return false;
  const int wx = (nx + 63) / 64;
  if ((size_t)wx * sizeof(u64) > LDS_MAX || tile_log2(ny) < 0 || tile_log2(nz) < 0) return false;
  // workgroups of the y and z passes (tiles x planes) as one grid dimension
  const long long lay = nz > n_prim ? nz : n_prim;
  const long long ty = (nx + (1 << tile_log2(ny)) - 1) >> tile_log2(ny), tz = (nx + (1 << tile_log2(nz)) - 1) >> tile_log2(nz);
  return ty * lay < (long long)INT_MAX && tz * ny < (long long)INT_MAX && (long long)ny * lay < (long long)INT_MAX;
}

size_t scene_words(int nx, int ny, int nz, int n_prim) {
  return (size_t)((nx + 63) / 64) * ny * (size_t)(nz > n_prim ? nz : n_prim);
}

hipError_t launch_scene_build(hipStream_t st, const SceneBuildArgs& a) {
  const int nx = a.nx, ny = a.ny, nz = a.nz, wx = (nx + 63) / 64;
  const int bnx = (nx + 3) / 4, bny = (ny + 3) / 4, bnz = (nz + 3) / 4;
  const size_t words = (size_t)wx * ny * nz, plane = (size_t)nx * ny;
  hipError_t e;
  // the buffers hold a previous scene: the bits are ORed into and the count is added to, everything else is
  // written in full by its pass
  if ((e = hipMemsetAsync(a.bits, 0, words * sizeof(u64), st)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(a.count, 0, sizeof(u64), st)) != hipSuccess) return e;
  if (a.n_keys > 0) {
    hipLaunchKernelGGL(scene_scatter_kernel, dim3(grid_for(a.n_keys)), dim3(SB), 0, st, a.keys, a.n_keys, a.kmin[0],
                       a.kmin[1], a.kmin[2], nx, ny, nz, wx, a.bits);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (a.carve) {
    if (a.carve_ev[0] && (e = hipEventRecord(a.carve_ev[0], st)) != hipSuccess) return e;
    if ((e = launch_carve(st, *a.carve)) != hipSuccess) return e;
    if (a.carve_ev[1] && (e = hipEventRecord(a.carve_ev[1], st)) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(scene_bricks_kernel, dim3(grid_for((long long)bnx * bny * bnz)), dim3(SB), 0, st, a.bits, ny, nz,
                     wx, bnx, bny, bnz, a.bricks, a.count);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(scene_dilate_kernel, dim3(grid_for((long long)words)), dim3(SB), 0, st, a.bits, nx, ny, nz, wx, 1,
                     a.dil);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = edt_x(st, a.dil, nx, wx, (long long)ny * nz, a.d2)) != hipSuccess) return e;
  if ((e = edt_lines(st, a.d2, nx, ny, (size_t)nx, plane, nz, nullptr)) != hipSuccess) return e;
  if ((e = edt_lines(st, a.d2, nx, nz, plane, (size_t)nx, ny, a.d2b)) != hipSuccess) return e;
  if (a.n_prim > 0) {
    // the slabs: projection into the (now free) dilation buffer, its 3x3 dilation into the occupancy buffer (the
    // bricks are built, nothing reads the bits any more), then the x and y passes with the primitives as planes
    const long long sw = (long long)wx * ny * a.n_prim;
    hipLaunchKernelGGL(scene_project_kernel, dim3(grid_for(sw)), dim3(SB), 0, st, a.bits, ny, nz, wx, a.n_prim, a.k01,
                       a.dil);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(scene_dilate_kernel, dim3(grid_for(sw)), dim3(SB), 0, st, a.dil, nx, ny, a.n_prim, wx, 0,
                       a.bits);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = edt_x(st, a.bits, nx, wx, (long long)ny * a.n_prim, a.slab)) != hipSuccess) return e;
    if ((e = edt_lines(st, a.slab, nx, ny, (size_t)nx, plane, a.n_prim, nullptr)) != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_scene_bytes(hipStream_t st, const uint16_t* d2, long long n, uint8_t* d2b) {
  hipLaunchKernelGGL(scene_bytes_kernel, dim3(grid_for((n >> 3) + 1)), dim3(SB), 0, st, d2, n, d2b);
  return hipGetLastError();
}

size_t scene_kernels_private_bytes() {
  size_t need = 0;
  hipFuncAttributes fa;
  const void* ks[] = {reinterpret_cast<const void*>(&scene_scatter_kernel), reinterpret_cast<const void*>(&scene_bricks_kernel),
                      reinterpret_cast<const void*>(&scene_project_kernel), reinterpret_cast<const void*>(&scene_dilate_kernel),
                      reinterpret_cast<const void*>(&scene_edt_x_kernel), reinterpret_cast<const void*>(&scene_edt_line_kernel),
                      reinterpret_cast<const void*>(&scene_bytes_kernel)};
  for (const void* k : ks)
    if (hipFuncGetAttributes(&fa, k) == hipSuccess && (size_t)fa.localSizeBytes > need) need = fa.localSizeBytes;
  return need;
}

}  // namespace smp
