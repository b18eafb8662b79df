// Self filter of the device scene build (smp_planner_set_carve / smp_carve_keys): the robot's own volume
// taken out of an occupied key list.  The octomap the node fetches holds the arm's and a grasped object's voxels; a
// key is carved when some selected item of the robot at the pose the map was taken -- a sphere, or an exact box /
// cylinder primitive -- has its clearance map term against that key's single cell at or below pad
// (include/smp_gpu.h "Self filter"; the terms are those of "Clearance queries", from smp_clearance_dev.h).
//
// Two launches.  carve_items_kernel, one workgroup: the body frames at q in the checker's arithmetic, the selected
// items' world data and the union of their boxes inflated by pad.  carve_kernel, over the keys: every workgroup stages
// those items in LDS once (2.9 KB), every work-item reads its key once, rejects it against the inflated box and
// otherwise runs the items until one carves it; a carved key costs one flag store or one atomicAnd on the bit grid.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "smp_carve.h"
#include "smp_clearance_dev.h"

namespace smp {

namespace {

constexpr int CB = 256;  // threads per workgroup of the carve kernel (4 wavefronts)
typedef unsigned long long u64;
static_assert(sizeof(CarveItems) % 8 == 0, "CarveItems is staged in 64-bit words");

struct CarvePose {
  double q[NJ];
  double pad;
  uint32_t links;
};

__global__ __launch_bounds__(128) void carve_items_kernel(const RobotDev* __restrict__ rb, CarvePose P,
                                                          CarveItems* __restrict__ out) {
  __shared__ double fr[MAX_BODY][12];
  __shared__ double ql[NJ];
  __shared__ int sel_s[MAX_SPH], sel_p[MAX_PRIM], n_sel[2];
  const int tid = threadIdx.x;
  if (tid < NJ) ql[tid] = P.q[tid];
  __syncthreads();
  if (tid == 0) {
    frames_to_lds(rb, ql, fr);
    int ns = 0, np = 0;
    for (int s = 0; s < rb->n_sph && s < MAX_SPH; ++s)
      if ((P.links >> rb->sph_clink[s]) & 1u) sel_s[ns++] = s;
    for (int p = 0; p < rb->n_prim && p < MAX_PRIM; ++p)
      if ((P.links >> rb->prim_clink[p]) & 1u) sel_p[np++] = p;
    n_sel[0] = ns;
    n_sel[1] = np;
  }
  __syncthreads();
  const int ns = n_sel[0], np = n_sel[1];
  for (int i = tid; i < ns; i += blockDim.x) {
    const int s = sel_s[i];
    const double* B = fr[rb->sph_body[s]];
    const double* p = &rb->sph_cb[s * 3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const double m = B[r * 3 + 0] * p[0] + B[r * 3 + 1] * p[1] + B[r * 3 + 2] * p[2];
      out->sph[i][r] = m + B[9 + r];
    }
    out->sph[i][3] = rb->sph_r[s];
  }
  for (int i = tid; i < np; i += blockDim.x) {
    const int p = sel_p[i];
    double pw[5];
    prim_world(rb, p, fr[rb->prim_body[p]], pw);
#pragma unroll
    for (int d = 0; d < 5; ++d) out->pw[i][d] = pw[d];
#pragma unroll
    for (int d = 0; d < 3; ++d) out->ph[i][d] = rb->prim_h[p * 3 + d];
    out->pty[i] = rb->prim_type[p];
  }
  __threadfence_block();
  __syncthreads();
  if (tid == 0) {
    // a cell whose box lies outside this box on some axis is farther than pad from every item (1e-6 m over the
    // rounding of the terms)
    double lo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    for (int i = 0; i < ns; ++i)
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        lo[d] = fmin(lo[d], out->sph[i][d] - out->sph[i][3]);
        hi[d] = fmax(hi[d], out->sph[i][d] + out->sph[i][3]);
      }
    for (int i = 0; i < np; ++i) {
      const double ac = fabs(out->pw[i][3]), as = fabs(out->pw[i][4]);
      const bool box = out->pty[i] == 1;
      const double e[3] = {box ? ac * out->ph[i][0] + as * out->ph[i][1] : out->ph[i][0],
                           box ? as * out->ph[i][0] + ac * out->ph[i][1] : out->ph[i][0],
                           box ? out->ph[i][2] : out->ph[i][1]};
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        lo[d] = fmin(lo[d], out->pw[i][d] - e[d]);
        hi[d] = fmax(hi[d], out->pw[i][d] + e[d]);
      }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      out->box[d] = lo[d] - P.pad - 1e-6;
      out->box[3 + d] = hi[d] + P.pad + 1e-6;
    }
    out->n_sph = ns;
    out->n_prim = np;
  }
}

struct CarveGrid {
  int kmin[3];
  int nx, ny, nz;
  double org[3], res, pad;
};

__global__ __launch_bounds__(CB) void carve_kernel(const CarveItems* __restrict__ items,
                                                   const uint16_t* __restrict__ keys, long long n, CarveGrid G,
                                                   uint8_t* __restrict__ flags, u64* __restrict__ bits,
                                                   u64* __restrict__ count) {
  __shared__ CarveItems I;
  for (int w = threadIdx.x; w < (int)(sizeof(CarveItems) / 8); w += CB)
    reinterpret_cast<u64*>(&I)[w] = reinterpret_cast<const u64*>(items)[w];
  __syncthreads();
  SceneDev sc{};
  sc.ox = G.org[0]; sc.oy = G.org[1]; sc.oz = G.org[2]; sc.res = G.res;
  const int ns = I.n_sph, np = I.n_prim, wx = (G.nx + 63) / 64;
  for (long long base = (long long)blockIdx.x * CB; base < n; base += (long long)gridDim.x * CB) {
    const long long i = base + threadIdx.x;
    bool hit = false;
    int ci = 0, cj = 0, ck = 0;
    if (i < n) {
      ci = (int)keys[3 * i] - G.kmin[0]; cj = (int)keys[3 * i + 1] - G.kmin[1]; ck = (int)keys[3 * i + 2] - G.kmin[2];
      const double xlo = sc.ox + (double)ci * sc.res, xhi = sc.ox + (double)(ci + 1) * sc.res;
      const double ylo = sc.oy + (double)cj * sc.res, yhi = sc.oy + (double)(cj + 1) * sc.res;
      const double zlo = sc.oz + (double)ck * sc.res, zhi = sc.oz + (double)(ck + 1) * sc.res;
      const bool near = !(xhi < I.box[0] || xlo > I.box[3] || yhi < I.box[1] || ylo > I.box[4] || zhi < I.box[2] ||
                          zlo > I.box[5]);
      if (near) {
        for (int s = 0; s < ns && !hit; ++s) {
          const double gx = axis_gap(I.sph[s][0], xlo, xhi), gy = axis_gap(I.sph[s][1], ylo, yhi);
          const double gz = axis_gap(I.sph[s][2], zlo, zhi);
          const double d = sqrt(gx * gx + gy * gy + gz * gz);
          const double t = d - I.sph[s][3];
          hit = t <= G.pad;
        }
        for (int p = 0; p < np && !hit; ++p) {
          const double t = sqrt(prim_cell_s(I.pty[p], I.ph[p], I.pw[p], sc, ci, cj, ck));
          hit = t <= G.pad;
        }
      }
    }
    if (hit) {
      if (flags) flags[i] = 1;
      else if ((unsigned)ci < (unsigned)G.nx && (unsigned)cj < (unsigned)G.ny && (unsigned)ck < (unsigned)G.nz)
        atomicAnd(&bits[((size_t)ck * G.ny + cj) * wx + (ci >> 6)], ~(1ull << (ci & 63)));
    }
    const u64 m = __ballot(hit);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(count, (u64)__popcll(m));
  }
}

}  // namespace

hipError_t launch_carve(hipStream_t st, const CarveArgs& a) {
  hipError_t e;
  if ((e = hipMemsetAsync(a.count, 0, sizeof(u64), st)) != hipSuccess) return e;
  if (a.n_keys <= 0) return hipSuccess;
  if (a.flags && (e = hipMemsetAsync(a.flags, 0, (size_t)a.n_keys, st)) != hipSuccess) return e;
  CarvePose P;
  for (int j = 0; j < NJ; ++j) P.q[j] = a.q[j];
  P.pad = a.pad;
  P.links = a.links;
  hipLaunchKernelGGL(carve_items_kernel, dim3(1), dim3(128), 0, st, a.rb, P, a.items);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  CarveGrid G;
  for (int d = 0; d < 3; ++d) { G.kmin[d] = a.kmin[d]; G.org[d] = a.org[d]; }
  G.nx = a.nx; G.ny = a.ny; G.nz = a.nz;
  G.res = a.res;
  G.pad = a.pad;
  const long long blocks = (a.n_keys + CB - 1) / CB;
  hipLaunchKernelGGL(carve_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(CB), 0, st, a.items, a.keys,
                     a.n_keys, G, a.flags, a.bits, a.count);
  return hipGetLastError();
}

size_t carve_kernels_private_bytes() {
  size_t need = 0;
  hipFuncAttributes fa;
  const void* ks[] = {reinterpret_cast<const void*>(&carve_items_kernel), reinterpret_cast<const void*>(&carve_kernel)};
  for (const void* k : ks)
    if (hipFuncGetAttributes(&fa, k) == hipSuccess && (size_t)fa.localSizeBytes > need) need = fa.localSizeBytes;
  return need;
}

}  // namespace smp
