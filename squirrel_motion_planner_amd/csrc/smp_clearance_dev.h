// Device helpers of the clearance sweeps, shared by the clearance queries (smp_clearance.hip) and the margin passes
// (smp_margin.hip): the body frames in the checker's arithmetic, the gap of a coordinate to an interval, the brick box of
// a reach and the squared distance of a primitive to a cell.  include/smp_gpu.h "Clearance queries" states the terms.
#ifndef SMP_CLEARANCE_DEV_H
#define SMP_CLEARANCE_DEV_H

#include <hip/hip_runtime.h>

#include "smp_collide.h"
#include "smp_math.h"
#include "smp_types.h"

namespace smp {

__device__ __forceinline__ double axis_gap(double c, double lo, double hi) {
  return c < lo ? lo - c : (c > hi ? c - hi : 0.0);
}

// body_frames (smp_collide.h) with the frames stored as they are formed: fr[b] = R row-major, then p.
__device__ __forceinline__ void frames_to_lds(const RobotDev* __restrict__ rb, const double* q, double (*fr)[12]) {
  Frame T;
  frame_identity(&T);
  T.p[2] = rb->root_z;
  const int nch = rb->n_chain;
  for (int k = 0; k < nch; ++k) {
    Frame L;
    const int ty = rb->ch_type[k];
    if (ty == 1) {
      rot2(&rb->ch_axis[k * 3], q[rb->ch_joint[k]], L.R);
      L.p[0] = rb->ch_origin[k * 3]; L.p[1] = rb->ch_origin[k * 3 + 1]; L.p[2] = rb->ch_origin[k * 3 + 2];
    } else if (ty == 2) {
      frame_identity(&L);
      const double qq = q[rb->ch_joint[k]];
#pragma unroll
      for (int d = 0; d < 3; ++d) L.p[d] = rb->ch_origin[k * 3 + d] + rb->ch_axis[k * 3 + d] * qq;
    } else {
#pragma unroll
      for (int i = 0; i < 9; ++i) L.R[i] = rb->ch_R[k * 9 + i];
#pragma unroll
      for (int d = 0; d < 3; ++d) L.p[d] = rb->ch_p[k * 3 + d];
    }
    fmul(T, L, &T);
    const int b = rb->ch_body[k];
    if (b >= 0) {
#pragma unroll
      for (int i = 0; i < 9; ++i) fr[b][i] = T.R[i];
      fr[b][9] = T.p[0]; fr[b][10] = T.p[1]; fr[b][11] = T.p[2];
    }
  }
}

struct BrickBox {
  int bi0, bj0, bk0, nbi, nbj, nb;
};
__device__ __forceinline__ BrickBox brick_box(const int* lo, const int* hi) {
  BrickBox R;
  R.bi0 = lo[0] >> 2; R.bj0 = lo[1] >> 2; R.bk0 = lo[2] >> 2;
  R.nbi = max((hi[0] >> 2) - R.bi0 + 1, 0); R.nbj = max((hi[1] >> 2) - R.bj0 + 1, 0);
  R.nb = R.nbi * R.nbj * max((hi[2] >> 2) - R.bk0 + 1, 0);
  return R;
}
__device__ __forceinline__ void brick_at(const BrickBox& R, int b, int& bi, int& bj, int& bk) {
  const int t = b / R.nbi;
  bi = R.bi0 + (b - t * R.nbi); bj = R.bj0 + t % R.nbj; bk = R.bk0 + t / R.nbj;
}
__device__ __forceinline__ uint64_t brick_word(const SceneDev& sc, const BrickBox& R, int b) {
  if (b >= R.nb) return 0;
  int bi, bj, bk;
  brick_at(R, b, bi, bj, bk);
  return sc.bricks[((size_t)bk * sc.bny + bj) * sc.bnx + bi];
}

// Squared distance s of an upright primitive (prim_cell's arguments) to the closed box of cell (i, j, k), 0 if they
// overlap; the primitive's map term against the cell is sqrt(s).  include/smp_gpu.h states the expression order.
__device__ __forceinline__ double prim_cell_s(int ty, const double* __restrict__ h, const double* pw, const SceneDev& sc,
                                              int i, int j, int k) {
  const double zlo = sc.oz + (double)k * sc.res, zhi = sc.oz + (double)(k + 1) * sc.res;
  const double hz = ty == 1 ? h[2] : h[1];
  double dz = zlo - (pw[2] + hz);
  const double dzb = (pw[2] - hz) - zhi;
  dz = dzb > dz ? dzb : dz;
  dz = dz > 0.0 ? dz : 0.0;
  const double xlo = sc.ox + (double)i * sc.res, xhi = sc.ox + (double)(i + 1) * sc.res;
  const double ylo = sc.oy + (double)j * sc.res, yhi = sc.oy + (double)(j + 1) * sc.res;
  if (ty == 2) {
    const double qx = axis_gap(pw[0], xlo, xhi), qy = axis_gap(pw[1], ylo, yhi);
    double dxy = sqrt(qx * qx + qy * qy) - h[0];
    dxy = dxy > 0.0 ? dxy : 0.0;
    return dxy * dxy + dz * dz;
  }
  const double c = pw[3], s = pw[4], ac = fabs(c), as = fabs(s), hw = 0.5 * sc.res;
  const double dx = 0.5 * (xlo + xhi) - pw[0], dy = 0.5 * (ylo + yhi) - pw[1];
  const bool apart = fabs(dx) > hw + (ac * h[0] + as * h[1]) || fabs(dy) > hw + (as * h[0] + ac * h[1]) ||
                     fabs(c * dx + s * dy) > h[0] + hw * (ac + as) || fabs(c * dy - s * dx) > h[1] + hw * (ac + as);
  double dxy2 = 0.0;
  if (apart) {
    dxy2 = HUGE_VAL;
    const double ch0 = c * h[0], sh0 = s * h[0], ch1 = c * h[1], sh1 = s * h[1];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      // a corner of the square against the solid rectangle (sphere_prim's form)
      const double ex = ((v & 1) ? xhi : xlo) - pw[0], ey = ((v & 2) ? yhi : ylo) - pw[1];
      const double lx = fabs(c * ex + s * ey), ly = fabs(c * ey - s * ex);
      const double qx = lx > h[0] ? lx - h[0] : 0.0, qy = ly > h[1] ? ly - h[1] : 0.0;
      const double a = qx * qx + qy * qy;
      dxy2 = a < dxy2 ? a : dxy2;
      // a corner of the rectangle against the square
      const double X = (v & 1) ? (pw[0] + ch0) : (pw[0] - ch0), Y = (v & 1) ? (pw[1] + sh0) : (pw[1] - sh0);
      const double cx = (v & 2) ? X - sh1 : X + sh1, cy = (v & 2) ? Y + ch1 : Y - ch1;
      const double gx = axis_gap(cx, xlo, xhi), gy = axis_gap(cy, ylo, yhi);
      const double b = gx * gx + gy * gy;
      dxy2 = b < dxy2 ? b : dxy2;
    }
  }
  return dxy2 + dz * dz;
}
}  // namespace smp
#endif  // SMP_CLEARANCE_DEV_H
