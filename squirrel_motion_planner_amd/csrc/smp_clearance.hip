// Clearance queries (gfx950): the distance of poses and dense edges to the map and to self-collision, with witnesses
// (include/smp_gpu.h "Clearance queries" holds the definition term by term; DESIGN.md 8c the layout).
//
// The collision tiles stop at the first hit; here every test becomes a minimum with its witness over a reach widened by
// the query distance D.  One workgroup takes one item at a time from an atomic work counter -- a tile of 32 consecutive
// configurations, or one edge of the density rule walked in tiles of 32 points with running minima -- in the passes'
// work loop (ticket_loop, smp_pass.h).  Per tile:
//   1. body frames, one lane per configuration, in the checker's arithmetic (body_frames' loop, storing into LDS);
//   2. lanes over (configuration, sphere) and (configuration, primitive): world centres, and the box-gap field d2 at the
//      centre cell against the widened threshold -- the loads of all items issued together; what passes is listed;
//   3. a wavefront per listed item sweeps the brick words of its widened reach, a word per lane (sweep_bricks: one round
//      trip for the usual reach), skipping zero words and bricks that cannot hold the minimum, and each lane walks the
//      occupied cells of its word (sphere_term, prim_term); a wavefront that runs out of items goes on to the flat self
//      pair lists, lanes over pairs, four configurations per wavefront interleaved;
//   4. (value, index) reductions inside the wavefront; across wavefronts through LDS.
// No workgroup reads what another wrote: the counter is a ticket dispenser, results are ordinary stores.
#include <hip/hip_runtime.h>

#include <limits.h>

#include "smp_clearance.h"
#include "smp_clearance_dev.h"
#include "smp_collide.h"
#include "smp_math.h"
#include "smp_pass.h"
#include "smp_types.h"

namespace smp {

constexpr int CL_ITEMS = MAX_SPH + MAX_PRIM;  // map items of one configuration: sphere s, then MAX_SPH + primitive p
constexpr int CL_CPW = PASS_CT / NWAVE;      // configurations per wavefront in the self test and the reductions
constexpr int CL_MAXU = (PASS_CT * MAX_SPH + BLOCK - 1) / BLOCK;  // (configuration, sphere) items per lane

struct ClearLds {
  double fr[PASS_CT][MAX_BODY][12];   // body frames (R row-major, p)
  double wc[PASS_CT][MAX_SPH][3];     // sphere world centres
  double pw[PASS_CT][MAX_PRIM][5];    // primitive centres and x axes
  double mterm[PASS_CT][CL_ITEMS];    // map term of every item, min(D, .)
  double c_map[PASS_CT], c_self[PASS_CT];  // per configuration: the two minima ...
  int c_link[PASS_CT], c_key[PASS_CT];     // ... the map witness link, the self witness a << 10 | b
  uint16_t cand[PASS_CT * CL_ITEMS];  // items that passed the prefilter: configuration << 8 | item
  uint16_t cand_d2[PASS_CT * CL_ITEMS];  // ... and d2 at their centre cell (65535: none, the centre is off the grid in z)
  unsigned ncand;
};
static_assert(PASS_CT <= 64 && CL_ITEMS <= 128 && CL_ITEMS <= 256, "item codes; two items per lane in the reduction");
static_assert(PASS_CT % NWAVE == 0, "tile size");

// Lexicographic minimum of (v, k) over the 64 lanes of a wavefront (all active); every lane receives it.
__device__ __forceinline__ void wave_min_key(double& v, int& k) {
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const double ov = __shfl_xor(v, o);
    const int ok = __shfl_xor(k, o);
    if (ov < v || (ov == v && ok < k)) { v = ov; k = ok; }
  }
}
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const double ov = __shfl_xor(v, o);
    v = ov < v ? ov : v;
  }
  return v;
}

// The brick's cell nearest to coordinate c along one axis (0..3; o + (4 * b + i) * res are the cells' faces): an end cell
// if c lies outside the brick, else the cell that holds c.  That cell's gap along the axis is the brick's own gap, to the
// bit: its near face is the same expression as the brick's.
__device__ __forceinline__ int nearest_in_brick(double c, double o, double res, int b) {
  if (c < o + (double)(4 * b) * res) return 0;
  int i = 0;
  while (i < 3 && c > o + (double)(4 * b + i + 1) * res) ++i;
  return i;
}

// The brick box of a sweep's reach and its words.  A reach of up to 64 * CL_PRE bricks (a sphere or primitive at the
// usual query distances) is loaded in one round trip, CL_PRE words per lane, and both passes of the sweep read
// registers; a larger one goes round by round (the words come from the cache the second time).
constexpr int CL_PRE = 6;
template <class Pass, class Between>
__device__ __forceinline__ void sweep_bricks(const SceneDev& sc, const BrickBox& R, int lane, Pass pass, Between between) {
  if (R.nb <= 64 * CL_PRE) {
    uint64_t w[CL_PRE];
#pragma unroll
    for (int u = 0; u < CL_PRE; ++u) w[u] = brick_word(sc, R, u * 64 + lane);
#pragma unroll
    for (int u = 0; u < CL_PRE; ++u)
      if (w[u]) pass(0, u * 64 + lane, w[u]);
    between();
#pragma unroll
    for (int u = 0; u < CL_PRE; ++u)
      if (w[u]) pass(1, u * 64 + lane, w[u]);
    return;
  }
  for (int p = 0; p < 2; ++p) {
    for (int b0 = 0; b0 < R.nb; b0 += 64) {
      const uint64_t w = brick_word(sc, R, b0 + lane);
      if (w) pass(p, b0 + lane, w);
    }
    if (p == 0) between();
  }
}

// Upper bound of the distance from a point to the nearest occupied box, from d2 at the point's cell: the field is the
// squared box-to-box gap, in cells, to the nearest occupied cell, so per axis that cell's box is at most a cell farther
// from the point than the gap, and the distance is at most (sqrt(d2) + sqrt(3)) cells; 1e-6 m covers a point within an
// ulp of a cell face.  A sweep's reach shrinks to it, which never changes the result.  65535 (the field's clamp): none.
__device__ __forceinline__ double near_bound(const SceneDev& sc, int d2v) {
  return d2v >= 65535 ? HUGE_VAL : (sqrt((double)d2v) + 1.7320508075688773) * sc.res + 1e-6;
}

// Map term of one sphere by a wavefront: min(D, min over occupied cells of sqrt(s) - r), s = gx*gx + gy*gy + gz*gz of the
// centre's gaps to the cell's box.  sqrt and the subtraction are monotone, so the least term is sqrt(least s) - r to the
// bit: the sweep carries s and takes one square root at its end.
// The brick words of the reach r + D (sphere_reach: a cell of margin, clipped to the grid), one per lane and round, in
// two passes:
//   0. an upper bound of the least s per non-empty brick: the s of its cell nearest to the centre if that cell is
//      occupied (it equals g, the s of the brick's own box, and no cell of the brick is nearer: the brick's box holds its
//      cells' boxes and every operation of s is monotone), else the squared distance to the brick's farthest corner (some
//      occupied cell lies in it); the wave's least such bound, or that of the reach, (r + D)^2, is `ub` (1e-9 added to
//      either: far above the rounding of s);
//   1. a lane drops a brick with g above ub or no less than its best s so far; it takes g for a brick whose nearest cell
//      is occupied (a solid obstacle, the floor below) and walks the occupied cells of the rest.
// Cells outside the reach could only give terms above D.
__device__ __forceinline__ double sphere_term(const SceneDev& sc, const double* ccp, double r, double D, double near,
                                              int lane) {
  const double cc[3] = {ccp[0], ccp[1], ccp[2]};
  int lo[3], hi[3];
  sphere_reach(sc, cc, fmin(r + D, near), lo, hi);  // (an occupied box lies within `near` of the centre: near_bound)
  const BrickBox R = brick_box(lo, hi);
  const double lim = (r + D) + 1e-9;
  double ub = lim * lim, best = HUGE_VAL;
  sweep_bricks(
      sc, R, lane,
      [&](int pass, int b, uint64_t w) {
        int bi, bj, bk;
        brick_at(R, b, bi, bj, bk);
        const double x0 = sc.ox + (double)(4 * bi) * sc.res, x1 = sc.ox + (double)(4 * bi + 4) * sc.res;
        const double y0 = sc.oy + (double)(4 * bj) * sc.res, y1 = sc.oy + (double)(4 * bj + 4) * sc.res;
        const double z0 = sc.oz + (double)(4 * bk) * sc.res, z1 = sc.oz + (double)(4 * bk + 4) * sc.res;
        const double gx = axis_gap(cc[0], x0, x1), gy = axis_gap(cc[1], y0, y1), gz = axis_gap(cc[2], z0, z1);
        const double g = gx * gx + gy * gy + gz * gz;
        if (g > ub || g >= best) return;
        const int nbit = nearest_in_brick(cc[2], sc.oz, sc.res, bk) << 4 |
                         nearest_in_brick(cc[1], sc.oy, sc.res, bj) << 2 | nearest_in_brick(cc[0], sc.ox, sc.res, bi);
        const bool near_occ = (w >> nbit) & 1ull;
        if (pass == 0) {
          double u = g;
          if (!near_occ) {
            const double fx = fmax(fabs(cc[0] - x0), fabs(cc[0] - x1)), fy = fmax(fabs(cc[1] - y0), fabs(cc[1] - y1));
            const double fz = fmax(fabs(cc[2] - z0), fabs(cc[2] - z1));
            u = fx * fx + fy * fy + fz * fz;
          }
          ub = u < ub ? u : ub;
          return;
        }
        if (near_occ) {
          best = g;
          return;
        }
        while (w) {
          const int bit = __builtin_ctzll(w);
          w &= w - 1;
          const int i = 4 * bi + (bit & 3), j = 4 * bj + ((bit >> 2) & 3), k = 4 * bk + (bit >> 4);
          const double ax = axis_gap(cc[0], sc.ox + (double)i * sc.res, sc.ox + (double)(i + 1) * sc.res);
          const double ay = axis_gap(cc[1], sc.oy + (double)j * sc.res, sc.oy + (double)(j + 1) * sc.res);
          const double az = axis_gap(cc[2], sc.oz + (double)k * sc.res, sc.oz + (double)(k + 1) * sc.res);
          const double s2 = ax * ax + ay * ay + az * az;
          best = s2 < best ? s2 : best;
        }
      },
      [&]() { ub = wave_min(ub) + 1e-9; });
  best = wave_min(best);
  const double t = sqrt(best) - r;
  return t < D ? t : D;
}

// Map term of one primitive by a wavefront: min(D, sqrt(min over occupied cells of prim_cell_s)) -- one square root at
// the end, as sphere_term, and the same two passes.  The reach is the primitive's axis-aligned bounds (prim_reach's)
// widened by D, a cell of margin, clipped to the grid.  From below a brick or a cell is bounded by the squared gap g
// between its box and those bounds; from above a non-empty brick bounds the least s by prim_cell_s of its cell nearest to
// the primitive's centre if that cell is occupied, else by the squared distance of the centre (a point of the primitive)
// to its farthest corner.  1e-9 lies between a lower and an upper bound, far above the rounding of either.  In pass 1 a
// cell is evaluated only if its own g can still lower the result: inside a solid obstacle that is its face.
__device__ __forceinline__ double prim_term(const SceneDev& sc, int ty, const double* __restrict__ h, const double* pwp,
                                            double D, double near, int lane) {
  const double pw[5] = {pwp[0], pwp[1], pwp[2], pwp[3], pwp[4]};
  const double ac = fabs(pw[3]), as = fabs(pw[4]);
  const double ex = ty == 1 ? ac * h[0] + as * h[1] : h[0];
  const double ey = ty == 1 ? as * h[0] + ac * h[1] : h[0];
  const double ez = ty == 1 ? h[2] : h[1];
  // (an occupied box lies within `near` of the centre, a point of the primitive: the term is at most that)
  const double W = fmin(D, near);
  int lo[3], hi[3];
  lo[0] = max((int)floor((pw[0] - ex - W - sc.ox) * sc.inv_res) - 1, 0);
  lo[1] = max((int)floor((pw[1] - ey - W - sc.oy) * sc.inv_res) - 1, 0);
  lo[2] = max((int)floor((pw[2] - ez - W - sc.oz) * sc.inv_res) - 1, 0);
  hi[0] = min((int)floor((pw[0] + ex + W - sc.ox) * sc.inv_res) + 1, sc.nx - 1);
  hi[1] = min((int)floor((pw[1] + ey + W - sc.oy) * sc.inv_res) + 1, sc.ny - 1);
  hi[2] = min((int)floor((pw[2] + ez + W - sc.oz) * sc.inv_res) + 1, sc.nz - 1);
  const BrickBox R = brick_box(lo, hi);
  const double lim = D + 1e-9;
  double ub = lim * lim, best = HUGE_VAL;
  // squared gap between the box [x0, x1] x [y0, y1] x [z0, z1] and the primitive's axis-aligned bounds
  auto box_gap = [&](double x0, double x1, double y0, double y1, double z0, double z1) {
    const double gx = fmax(fmax(x0 - (pw[0] + ex), (pw[0] - ex) - x1), 0.0);
    const double gy = fmax(fmax(y0 - (pw[1] + ey), (pw[1] - ey) - y1), 0.0);
    const double gz = fmax(fmax(z0 - (pw[2] + ez), (pw[2] - ez) - z1), 0.0);
    return gx * gx + gy * gy + gz * gz;
  };
  sweep_bricks(
      sc, R, lane,
      [&](int pass, int b, uint64_t w) {
        int bi, bj, bk;
        brick_at(R, b, bi, bj, bk);
        const double x0 = sc.ox + (double)(4 * bi) * sc.res, x1 = sc.ox + (double)(4 * bi + 4) * sc.res;
        const double y0 = sc.oy + (double)(4 * bj) * sc.res, y1 = sc.oy + (double)(4 * bj + 4) * sc.res;
        const double z0 = sc.oz + (double)(4 * bk) * sc.res, z1 = sc.oz + (double)(4 * bk + 4) * sc.res;
        const double cut = (best < ub ? best : ub) + 1e-9;
        if (box_gap(x0, x1, y0, y1, z0, z1) > cut) return;
        if (pass == 0) {
          const int ni = nearest_in_brick(pw[0], sc.ox, sc.res, bi), nj = nearest_in_brick(pw[1], sc.oy, sc.res, bj);
          const int nk = nearest_in_brick(pw[2], sc.oz, sc.res, bk);
          double u;
          if ((w >> (nk << 4 | nj << 2 | ni)) & 1ull) {
            u = prim_cell_s(ty, h, pw, sc, 4 * bi + ni, 4 * bj + nj, 4 * bk + nk);
          } else {
            const double fx = fmax(fabs(pw[0] - x0), fabs(pw[0] - x1)), fy = fmax(fabs(pw[1] - y0), fabs(pw[1] - y1));
            const double fz = fmax(fabs(pw[2] - z0), fabs(pw[2] - z1));
            u = fx * fx + fy * fy + fz * fz;
          }
          ub = u < ub ? u : ub;
          return;
        }
        while (w) {
          const int bit = __builtin_ctzll(w);
          w &= w - 1;
          const int i = 4 * bi + (bit & 3), j = 4 * bj + ((bit >> 2) & 3), k = 4 * bk + (bit >> 4);
          const double g = box_gap(sc.ox + (double)i * sc.res, sc.ox + (double)(i + 1) * sc.res,
                                   sc.oy + (double)j * sc.res, sc.oy + (double)(j + 1) * sc.res,
                                   sc.oz + (double)k * sc.res, sc.oz + (double)(k + 1) * sc.res);
          if (g > (best < ub ? best : ub) + 1e-9) continue;
          const double s2 = prim_cell_s(ty, h, pw, sc, i, j, k);
          best = s2 < best ? s2 : best;
        }
      },
      [&]() { ub = wave_min(ub) + 1e-9; });
  best = wave_min(best);
  const double t = sqrt(best);
  return t < D ? t : D;
}

// Clearance of nc <= PASS_CT configurations q_lds[c], all block threads.  On return (after a block barrier)
// L.c_map / c_link / c_self / c_key hold the results of configurations 0 .. nc - 1.
__device__ __forceinline__ void clearance_tile(const RobotDev* __restrict__ rb, const SceneDev& sc,
                                               const MapCfg* __restrict__ mc, const ClearCfg& cfg, int nc,
                                               const double (*q_lds)[NJ], ClearLds& L) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nsph = __builtin_amdgcn_readfirstlane(rb->n_sph), npr = __builtin_amdgcn_readfirstlane(rb->n_prim);
  const bool do_map = cfg.with_map && mc->has_map;
  const double D = cfg.D;
  // 1. body frames
  if (tid < nc) frames_to_lds(rb, q_lds[tid], L.fr[tid]);
  for (int it = tid; it < nc * CL_ITEMS; it += BLOCK) (&L.mterm[0][0])[it] = D;
  if (tid == 0) L.ncand = 0u;
  __syncthreads();
  // 2. centres and prefilter
  {
    long long cell[CL_MAXU];
#pragma unroll
    for (int u = 0; u < CL_MAXU; ++u) {
      const int it = u * BLOCK + tid;
      cell[u] = -1;
      const int c = it / nsph, s = it - c * nsph;
      if (c < nc) {
        const double* B = L.fr[c][rb->sph_body[s]];
        const double* p = &rb->sph_cb[s * 3];
        double w[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const double m = B[r * 3 + 0] * p[0] + B[r * 3 + 1] * p[1] + B[r * 3 + 2] * p[2];
          w[r] = m + B[9 + r];
        }
        L.wc[c][s][0] = w[0]; L.wc[c][s][1] = w[1]; L.wc[c][s][2] = w[2];
        if (do_map && mc->map_on[s]) {
          // (the quotient, as sphere_hits_map forms it: whether the centre is outside the grid decides the term)
          const double fx = floor((w[0] - sc.ox) / sc.res), fy = floor((w[1] - sc.oy) / sc.res);
          const double fz = floor((w[2] - sc.oz) / sc.res);
          if (fx >= 0 && fx < sc.nx && fy >= 0 && fy < sc.ny && fz >= 0 && fz < sc.nz)
            cell[u] = ((long long)(int)fz * sc.ny + (int)fy) * sc.nx + (int)fx;
        }
      }
    }
    uint32_t dv[CL_MAXU];
#pragma unroll
    for (int u = 0; u < CL_MAXU; ++u) dv[u] = cell[u] >= 0 ? (uint32_t)sc.d2[cell[u]] : 0xffffffffu;
#pragma unroll
    for (int u = 0; u < CL_MAXU; ++u) {
      const int it = u * BLOCK + tid;
      const int c = it / nsph, s = it - c * nsph;
      if (cell[u] >= 0 && dv[u] <= cfg.T[s]) {
        const unsigned pos = atomicAdd(&L.ncand, 1u);
        L.cand[pos] = (uint16_t)(c << 8 | s);
        L.cand_d2[pos] = (uint16_t)dv[u];
      }
    }
    for (int it = tid; it < nc * npr; it += BLOCK) {
      const int c = it / npr, p = it - c * npr;
      double* pw = L.pw[c][p];
      prim_world(rb, p, L.fr[c][rb->prim_body[p]], pw);
      if (do_map && mc->p_map_on[p]) {
        const double fx = floor((pw[0] - sc.ox) / sc.res), fy = floor((pw[1] - sc.oy) / sc.res);
        const double fz = floor((pw[2] - sc.oz) / sc.res);
        if (fx >= 0 && fx < sc.nx && fy >= 0 && fy < sc.ny) {  // (a centre column outside the grid: the term is D)
          uint32_t dp = 65535u;
          if (fz >= 0 && fz < sc.nz) dp = (uint32_t)sc.d2[((long long)(int)fz * sc.ny + (int)fy) * sc.nx + (int)fx];
          if (!(fz >= 0 && fz < sc.nz) || dp <= cfg.pT[p]) {
            const unsigned pos = atomicAdd(&L.ncand, 1u);
            L.cand[pos] = (uint16_t)(c << 8 | (MAX_SPH + p));
            L.cand_d2[pos] = (uint16_t)dp;
          }
        }
      }
    }
  }
  __syncthreads();
  // 3. map sweeps, a wavefront per listed item
  const int ncand = __builtin_amdgcn_readfirstlane((int)L.ncand);
  for (int i = wave; i < ncand; i += NWAVE) {
    const int code = __builtin_amdgcn_readfirstlane((int)L.cand[i]);
    const int c = code >> 8, it = code & 255;
    const double near = near_bound(sc, __builtin_amdgcn_readfirstlane((int)L.cand_d2[i]));
    double t;
    if (it < MAX_SPH) {
      t = sphere_term(sc, L.wc[c][it], rb->sph_r[it], D, near, lane);
    } else {
      const int p = it - MAX_SPH;
      t = prim_term(sc, rb->prim_type[p], &rb->prim_h[p * 3], L.pw[c][p], D, near, lane);
    }
    if (lane == 0) L.mterm[c][it] = t;
  }
  // self: lanes over the flat pair lists, this wavefront's configurations k * NWAVE + wave interleaved
  double sv[CL_CPW];
  int sk[CL_CPW];
#pragma unroll
  for (int k = 0; k < CL_CPW; ++k) { sv[k] = HUGE_VAL; sk[k] = INT_MAX; }
  if (cfg.with_self) {
    const int nsp = rb->n_spairs;
    for (int p = lane; p < nsp; p += 64) {
      const uint32_t ab = rb->sp_ab[p];
      const int a = ab & 0xff, b = ab >> 8;
      const double rr = rb->sph_r[a] + rb->sph_r[b];
      const int la = rb->cl_link[rb->sph_clink[a]], lb = rb->cl_link[rb->sph_clink[b]];
      const int key = min(la, lb) << 10 | max(la, lb);
#pragma unroll
      for (int k = 0; k < CL_CPW; ++k) {
        const int c = k * NWAVE + wave;
        if (c >= nc) continue;
        const double* wa = L.wc[c][a];
        const double* wb = L.wc[c][b];
        const double ex = wa[0] - wb[0], ey = wa[1] - wb[1], ez = wa[2] - wb[2];
        const double d = sqrt(ex * ex + ey * ey + ez * ez) - rr;
        if (d < sv[k] || (d == sv[k] && key < sk[k])) { sv[k] = d; sk[k] = key; }
      }
    }
    const int npp = rb->n_ppairs;
    for (int p = lane; p < npp; p += 64) {
      const uint32_t ps = rb->pp_ps[p];
      const int pr = ps & 0xff, sp = ps >> 8;
      const int ty = rb->prim_type[pr];
      const double* h = &rb->prim_h[pr * 3];
      const double rs = rb->sph_r[sp];
      const int la = rb->cl_link[rb->prim_clink[pr]], lb = rb->cl_link[rb->sph_clink[sp]];
      const int key = min(la, lb) << 10 | max(la, lb);
#pragma unroll
      for (int k = 0; k < CL_CPW; ++k) {
        const int c = k * NWAVE + wave;
        if (c >= nc) continue;
        const double* pw = L.pw[c][pr];
        const double* w = L.wc[c][sp];
        const double dx = w[0] - pw[0], dy = w[1] - pw[1], dz = w[2] - pw[2];
        const double az = fabs(dz);
        double q2;
        if (ty == 1) {
          const double lx = fabs(pw[3] * dx + pw[4] * dy), ly = fabs(pw[3] * dy - pw[4] * dx);
          const double qx = lx > h[0] ? lx - h[0] : 0.0, qy = ly > h[1] ? ly - h[1] : 0.0;
          const double qz = az > h[2] ? az - h[2] : 0.0;
          q2 = qx * qx + qy * qy + qz * qz;
        } else {
          const double rho = sqrt(dx * dx + dy * dy);
          const double qr = rho > h[0] ? rho - h[0] : 0.0, qz = az > h[1] ? az - h[1] : 0.0;
          q2 = qr * qr + qz * qz;
        }
        const double d = sqrt(q2) - rs;
        if (d < sv[k] || (d == sv[k] && key < sk[k])) { sv[k] = d; sk[k] = key; }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < CL_CPW; ++k) {
    wave_min_key(sv[k], sk[k]);
    const int c = k * NWAVE + wave;
    if (lane == 0 && c < nc) { L.c_self[c] = sv[k]; L.c_key[c] = sk[k]; }
  }
  __syncthreads();
  // 4. per configuration: the least map term, the smallest link among equal ones
#pragma unroll
  for (int k = 0; k < CL_CPW; ++k) {
    const int c = k * NWAVE + wave;
    if (c >= nc) continue;  // (wave-uniform)
    double v = HUGE_VAL;
    int link = INT_MAX;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int it = u * 64 + lane;
      int l = -1;
      if (it < nsph) l = rb->cl_link[rb->sph_clink[it]];
      else if (it >= MAX_SPH && it < MAX_SPH + npr) l = rb->cl_link[rb->prim_clink[it - MAX_SPH]];
      if (l >= 0) {
        const double t = L.mterm[c][it];
        if (t < v || (t == v && l < link)) { v = t; link = l; }
      }
    }
    wave_min_key(v, link);
    if (lane == 0) {
      const bool in = v < D;
      L.c_map[c] = in ? v : D;
      L.c_link[c] = in ? link : -1;
    }
  }
  __syncthreads();
}

__global__ void __launch_bounds__(BLOCK) clearance_kernel(const RobotDev* __restrict__ rb, SceneDev sc_in,
                                                          const MapCfg* __restrict__ mc, ClearCfg cfg,
                                                          const double* __restrict__ q_rows, long long n,
                                                          const EdgeDev* __restrict__ edges,
                                                          const int* __restrict__ order, int n_items,
                                                          unsigned* __restrict__ counter, ClearDev* __restrict__ out_c,
                                                          EdgeClearDev* __restrict__ out_e) {
  __shared__ RobotDev s_rb;
  __shared__ MapCfg s_mc;
  __shared__ ClearLds L;
  __shared__ double ql[PASS_CT][NJ];
  __shared__ double ea[NJ], es[NJ];  // the edge's start and its step (b - a) / M
  const int tid = threadIdx.x;
  stage_model(rb, mc, &s_rb, &s_mc);  // (ends with a barrier)
  const SceneDev sc = uniform_scene(sc_in);
  // an edge's record and its running minima (wave 0, the same in all its lanes)
  struct Done {
    int e, M;
    double r_map, r_self;
    int r_mpt, r_mlink, r_spt, r_skey;
  };
  ticket_loop(
      counter, (unsigned)n_items,
      [&](unsigned slot) {
        Done d{0, 0, cfg.D, HUGE_VAL, -1, -1, -1, -1};
        long long q0 = 0;
        if (edges) {
          d.e = __builtin_amdgcn_readfirstlane(order[slot]);
          d.M = __builtin_amdgcn_readfirstlane(edges[d.e].M);
          if (tid < NJ) {
            const double a = edges[d.e].a[tid], b = edges[d.e].b[tid];
            ea[tid] = a;
            es[tid] = edge_step(a, b, d.M);
          }
        } else {
          q0 = (long long)slot * PASS_CT;
          d.M = __builtin_amdgcn_readfirstlane((int)min((long long)PASS_CT, n - q0)) - 1;
        }
        __syncthreads();
        for (int base = 0; base <= d.M; base += PASS_CT) {
          const int nc = __builtin_amdgcn_readfirstlane(min(PASS_CT, d.M + 1 - base));
          if (edges) {
            edge_tile(ql, ea, es, base, nc);
          } else {
            for (int it = tid; it < nc * NJ; it += BLOCK) {
              const int c = it / NJ, j = it - c * NJ;
              ql[c][j] = q_rows[(q0 + c) * NJ + j];
            }
          }
          __syncthreads();
          clearance_tile(&s_rb, sc, &s_mc, cfg, nc, ql, L);  // (ends with a barrier)
          if (!edges) {
            if (tid < nc) {
              ClearDev o;
              o.map = L.c_map[tid];
              o.map_link = L.c_link[tid];
              o.self = L.c_self[tid];
              const int key = L.c_key[tid];
              const bool has = cfg.with_self && key != INT_MAX;
              o.self_a = has ? key >> 10 : -1;
              o.self_b = has ? key & 1023 : -1;
              o.pad = 0;
              out_c[q0 + tid] = o;
            }
          } else if (tid < 64) {
            // the tile's least values and the lowest point attaining each; a later tile must be strictly below
            double v = tid < nc ? L.c_map[tid] : HUGE_VAL;
            int pt = tid < nc ? tid : INT_MAX;
            wave_min_key(v, pt);
            if (v < d.r_map) { d.r_map = v; d.r_mpt = base + pt; d.r_mlink = L.c_link[pt]; }
            v = tid < nc ? L.c_self[tid] : HUGE_VAL;
            pt = tid < nc ? tid : INT_MAX;
            wave_min_key(v, pt);
            if (v < d.r_self) { d.r_self = v; d.r_spt = base + pt; d.r_skey = L.c_key[pt]; }
          }
          __syncthreads();  // ql and the tile's results are rewritten by the next tile
        }
        return d;
      },
      [&](unsigned, const Done& d) {
        if (!edges) return;
        EdgeClearDev o;
        o.map = d.r_map; o.self = d.r_self;
        o.map_point = d.r_mpt; o.self_point = d.r_spt;
        o.map_link = d.r_mlink;
        o.self_a = d.r_spt >= 0 ? d.r_skey >> 10 : -1;
        o.self_b = d.r_spt >= 0 ? d.r_skey & 1023 : -1;
        o.n_points = d.M + 1;
        out_e[d.e] = o;
      });
}

size_t clearance_kernels_private_bytes() { return kernel_private_bytes(&clearance_kernel); }

void launch_clearance(int grid, hipStream_t st, const RobotDev* rb, SceneDev sc, const MapCfg* mc, const ClearCfg& cfg,
                      const double* q_rows, long long n, const EdgeDev* edges, const int* order, int n_items,
                      unsigned* counter, ClearDev* out_c, EdgeClearDev* out_e) {
  hipLaunchKernelGGL(clearance_kernel, dim3(grid), dim3(BLOCK), 0, st, rb, sc, mc, cfg, q_rows, n, edges, order, n_items,
                     counter, out_c, out_e);
}

}  // namespace smp
