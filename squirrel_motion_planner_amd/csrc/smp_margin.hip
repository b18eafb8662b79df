// Margin passes (gfx950): the path passes' predicate with a safety margin -- "is every point farther than mm from the map
// and ms from itself?" -- for tiles of configurations, dense edges and detour items (include/smp_gpu.h "Margin checks"
// holds the definition; DESIGN.md 8d the layout).
//
// It sits between the boolean checks and the clearance queries: the terms are the clearance queries' (the same frames,
// centres and expressions, to the bit), but only their comparison with the margin is wanted, so nothing is minimised and
// every test stops at the first violation.  One workgroup takes one item at a time in the passes' work loop (ticket_loop,
// smp_pass.h).  Per tile of 32 configurations (margin_tile):
//   0. a part whose margin is 0 is the boolean test of that part: collide_tile on the tile, its flags taken over;
//   1. body frames, one lane per configuration, in the checker's arithmetic (frames_to_lds);
//   2. lanes over (configuration, sphere) and (configuration, primitive): world centres, and the clearance queries'
//      prefilter at D = mm -- the box-gap field at the centre cell against the widened threshold; what passes is listed;
//   3. self: lanes over the flat pair lists, four configurations per wavefront interleaved, d <= ms sets the flag;
//   4. map: every listed item's reach r + mm is a box of brick words; an exclusive scan of the boxes' word counts lays
//      the lanes of the whole workgroup over the (item, brick word) pairs.  A lane finds its item by bisection of the
//      offsets, loads its word and tests the word's occupied cells against the item's threshold: a cell violates iff its
//      squared distance s is <= S[item], the largest double whose term is still <= mm (formed on the host), so no cell
//      costs a square root.  A violation is a plain LDS store of 1 to the configuration's flag -- several lanes may
//      store the same value -- and pairs of a flagged configuration are skipped.  The rare item whose box has more than
//      MG_FLAT words (a margin of metres) is swept by one wavefront, a word per lane and round.
// Every configuration of a tile is decided: the lowest flagged index is an edge's answer.
// No workgroup reads what another wrote: the counter is a ticket dispenser, results are ordinary stores.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "smp_clearance_dev.h"
#include "smp_collide.h"
#include "smp_margin.h"
#include "smp_math.h"
#include "smp_pass.h"
#include "smp_types.h"

namespace smp {

constexpr int MG_ITEMS = MAX_SPH + MAX_PRIM;  // map items of one configuration: sphere s, then MAX_SPH + primitive p
constexpr int MG_CAND = PASS_CT * MG_ITEMS;   // listed items of one tile, at most
constexpr int MG_CPW = PASS_CT / NWAVE;       // configurations per wavefront in the self test
constexpr int MG_MAXU = (PASS_CT * MAX_SPH + BLOCK - 1) / BLOCK;  // (configuration, sphere) items per lane
constexpr int MG_PER = (MG_CAND + BLOCK - 1) / BLOCK;             // listed items per lane in the scan
constexpr int MG_FLAT = 4096;  // brick words of one item in the flat layout; MG_CAND * MG_FLAT pairs fit an int

struct MarginLds {
  union {
    TileLds<PASS_CT> tile;               // stage 0: collide_tile's work area
    struct {
      double fr[PASS_CT][MAX_BODY][12];  // body frames (R row-major, p)
      double wc[PASS_CT][MAX_SPH][3];    // sphere world centres
      double pw[PASS_CT][MAX_PRIM][5];   // primitive centres and x axes
    } m;
  } u;
  int flag[PASS_CT];          // 1 = not clear
  uint16_t cand[MG_CAND];     // items that passed the prefilter: configuration << 8 | item
  uint16_t big[MG_CAND];      // ... of which those of more than MG_FLAT brick words
  int off[MG_CAND + 1];       // exclusive scan of the listed items' word counts (0 for the big ones)
  int wsum[NWAVE];
  unsigned ncand, nbig;
};
static_assert(PASS_CT <= 64 && MG_ITEMS <= 256, "item codes");
static_assert(PASS_CT % NWAVE == 0, "tile size");
static_assert((long long)MG_CAND * MG_FLAT < 0x7fffffffLL, "pair indices are ints");

// The cells an item's margin can reach, clipped to the grid, as a box of bricks: a sphere's reach r + mm
// (sphere_reach), a primitive's axis-aligned bounds widened by mm (the clearance sweep's reach), a cell of margin each.
__device__ __forceinline__ BrickBox sphere_box(const SceneDev& sc, const double* wc, double reach) {
  const double cc[3] = {wc[0], wc[1], wc[2]};
  int lo[3], hi[3];
  sphere_reach(sc, cc, reach, lo, hi);
  return brick_box(lo, hi);
}
// ex, ey, ez: the half extents of the primitive's axis-aligned bounds.
__device__ __forceinline__ void prim_extents(int ty, const double* __restrict__ h, const double* pw, double* e) {
  const double ac = fabs(pw[3]), as = fabs(pw[4]);
  e[0] = ty == 1 ? ac * h[0] + as * h[1] : h[0];
  e[1] = ty == 1 ? as * h[0] + ac * h[1] : h[0];
  e[2] = ty == 1 ? h[2] : h[1];
}
__device__ __forceinline__ BrickBox prim_box(const SceneDev& sc, const double* pw, const double* e, double W) {
  int lo[3], hi[3];
  lo[0] = max((int)floor((pw[0] - e[0] - W - sc.ox) * sc.inv_res) - 1, 0);
  lo[1] = max((int)floor((pw[1] - e[1] - W - sc.oy) * sc.inv_res) - 1, 0);
  lo[2] = max((int)floor((pw[2] - e[2] - W - sc.oz) * sc.inv_res) - 1, 0);
  hi[0] = min((int)floor((pw[0] + e[0] + W - sc.ox) * sc.inv_res) + 1, sc.nx - 1);
  hi[1] = min((int)floor((pw[1] + e[1] + W - sc.oy) * sc.inv_res) + 1, sc.ny - 1);
  hi[2] = min((int)floor((pw[2] + e[2] + W - sc.oz) * sc.inv_res) + 1, sc.nz - 1);
  return brick_box(lo, hi);
}

// One map item of a tile, as the lanes of the sweep see it.
struct MarginItem {
  int c, it;      // configuration, item code
  BrickBox R;
};
__device__ __forceinline__ MarginItem margin_item(const RobotDev* __restrict__ rb, const SceneDev& sc, const MarginCfg& cfg,
                                                  const MarginLds& L, int code) {
  MarginItem I;
  I.c = code >> 8;
  I.it = code & 255;
  if (I.it < MAX_SPH) {
    I.R = sphere_box(sc, L.u.m.wc[I.c][I.it], rb->sph_r[I.it] + cfg.mm);
  } else {
    const int p = I.it - MAX_SPH;
    double e[3];
    prim_extents(rb->prim_type[p], &rb->prim_h[p * 3], L.u.m.pw[I.c][p], e);
    I.R = prim_box(sc, L.u.m.pw[I.c][p], e, cfg.mm);
  }
  return I;
}

// Brick word b of item I by one lane: true iff an occupied cell of it lies within the margin.  A brick is dropped on the
// squared gap g of its own box (no cell of it is nearer: the brick's box holds its cells' boxes and every operation of s
// is monotone); for a primitive g is the gap to its axis-aligned bounds, a lower bound with the clearance sweep's slack.
__device__ __forceinline__ bool word_violates(const RobotDev* __restrict__ rb, const SceneDev& sc, const MarginCfg& cfg,
                                              const MarginLds& L, const MarginItem& I, int b) {
  uint64_t w = brick_word(sc, I.R, b);
  if (!w) return false;
  int bi, bj, bk;
  brick_at(I.R, b, bi, bj, bk);
  const double x0 = sc.ox + (double)(4 * bi) * sc.res, x1 = sc.ox + (double)(4 * bi + 4) * sc.res;
  const double y0 = sc.oy + (double)(4 * bj) * sc.res, y1 = sc.oy + (double)(4 * bj + 4) * sc.res;
  const double z0 = sc.oz + (double)(4 * bk) * sc.res, z1 = sc.oz + (double)(4 * bk + 4) * sc.res;
  if (I.it < MAX_SPH) {
    const double* wc = L.u.m.wc[I.c][I.it];
    const double cx = wc[0], cy = wc[1], cz = wc[2];
    const double S = cfg.S[I.it];
    const double gx = axis_gap(cx, x0, x1), gy = axis_gap(cy, y0, y1), gz = axis_gap(cz, z0, z1);
    if (gx * gx + gy * gy + gz * gz > S) return false;
    while (w) {
      const int bit = __builtin_ctzll(w);
      w &= w - 1;
      const int i = 4 * bi + (bit & 3), j = 4 * bj + ((bit >> 2) & 3), k = 4 * bk + (bit >> 4);
      const double ax = axis_gap(cx, sc.ox + (double)i * sc.res, sc.ox + (double)(i + 1) * sc.res);
      const double ay = axis_gap(cy, sc.oy + (double)j * sc.res, sc.oy + (double)(j + 1) * sc.res);
      const double az = axis_gap(cz, sc.oz + (double)k * sc.res, sc.oz + (double)(k + 1) * sc.res);
      if (ax * ax + ay * ay + az * az <= S) return true;
    }
    return false;
  }
  const int p = I.it - MAX_SPH;
  const int ty = rb->prim_type[p];
  const double* h = &rb->prim_h[p * 3];
  const double* pwp = L.u.m.pw[I.c][p];
  const double pw[5] = {pwp[0], pwp[1], pwp[2], pwp[3], pwp[4]};
  double e[3];
  prim_extents(ty, h, pw, e);
  // squared gap between the box [a0, a1] x [b0, b1] x [c0, c1] and the primitive's axis-aligned bounds
  auto box_gap = [&](double a0, double a1, double b0, double b1, double c0, double c1) {
    const double gx = fmax(fmax(a0 - (pw[0] + e[0]), (pw[0] - e[0]) - a1), 0.0);
    const double gy = fmax(fmax(b0 - (pw[1] + e[1]), (pw[1] - e[1]) - b1), 0.0);
    const double gz = fmax(fmax(c0 - (pw[2] + e[2]), (pw[2] - e[2]) - c1), 0.0);
    return gx * gx + gy * gy + gz * gz;
  };
  const double cut = cfg.Sp + 1e-9;
  if (box_gap(x0, x1, y0, y1, z0, z1) > cut) return false;
  while (w) {
    const int bit = __builtin_ctzll(w);
    w &= w - 1;
    const int i = 4 * bi + (bit & 3), j = 4 * bj + ((bit >> 2) & 3), k = 4 * bk + (bit >> 4);
    const double g = box_gap(sc.ox + (double)i * sc.res, sc.ox + (double)(i + 1) * sc.res, sc.oy + (double)j * sc.res,
                             sc.oy + (double)(j + 1) * sc.res, sc.oz + (double)k * sc.res,
                             sc.oz + (double)(k + 1) * sc.res);
    if (g > cut) continue;
    if (prim_cell_s(ty, h, pw, sc, i, j, k) <= cfg.Sp) return true;
  }
  return false;
}

// The margin predicate of nc <= PASS_CT configurations q_lds[c], all block threads.  On return (after a block barrier)
// L.flag[c] is 1 for the configurations 0 .. nc - 1 that are not clear, 0 for the clear ones.
// sc_in is the kernel's own scene argument (collide_tile reads its slab fields), sc its uniform copy.
__device__ __forceinline__ void margin_tile(const RobotDev* __restrict__ rb, const SceneDev& sc_in, const SceneDev& sc,
                                            const MapCfg* __restrict__ mc, const MarginCfg& cfg, int nc,
                                            const double (*q_lds)[NJ], MarginLds& L) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nsph = __builtin_amdgcn_readfirstlane(rb->n_sph), npr = __builtin_amdgcn_readfirstlane(rb->n_prim);
  // the parts with a margin, and those that are the boolean test (all four the same in every thread: kernel arguments
  // and a word of the staged map configuration)
  const bool m_map = cfg.map && cfg.mm > 0.0 && __builtin_amdgcn_readfirstlane(mc->has_map) != 0;
  const bool m_self = cfg.self && cfg.ms > 0.0;
  const int b_map = (cfg.map && !(cfg.mm > 0.0)) ? 1 : 0, b_self = (cfg.self && !m_self) ? 1 : 0;
  // 0. the boolean parts
  if (b_map || b_self) {
    collide_tile<PASS_CT>(rb, sc_in, mc, nc, q_lds, b_self, b_map, L.u.tile);  // (ends with a barrier)
    if (tid < PASS_CT) L.flag[tid] = (tid < nc && L.u.tile.coll[tid] != 0) ? 1 : 0;
  } else if (tid < PASS_CT) {
    L.flag[tid] = 0;
  }
  if (tid == 0) { L.ncand = 0u; L.nbig = 0u; }
  __syncthreads();  // (the work area is rewritten below)
  if (!m_map && !m_self) return;
  // 1. body frames
  if (tid < nc) frames_to_lds(rb, q_lds[tid], L.u.m.fr[tid]);
  __syncthreads();
  // 2. centres and prefilter (clearance_tile's, with D = mm)
  {
    long long cell[MG_MAXU];
#pragma unroll
    for (int u = 0; u < MG_MAXU; ++u) {
      const int it = u * BLOCK + tid;
      cell[u] = -1;
      const int c = it / nsph, s = it - c * nsph;
      if (c < nc) {
        const double* B = L.u.m.fr[c][rb->sph_body[s]];
        const double* p = &rb->sph_cb[s * 3];
        double w[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const double m = B[r * 3 + 0] * p[0] + B[r * 3 + 1] * p[1] + B[r * 3 + 2] * p[2];
          w[r] = m + B[9 + r];
        }
        L.u.m.wc[c][s][0] = w[0]; L.u.m.wc[c][s][1] = w[1]; L.u.m.wc[c][s][2] = w[2];
        if (m_map && mc->map_on[s]) {
          // (the quotient, as sphere_hits_map forms it: whether the centre is outside the grid decides the term)
          const double fx = floor((w[0] - sc.ox) / sc.res), fy = floor((w[1] - sc.oy) / sc.res);
          const double fz = floor((w[2] - sc.oz) / sc.res);
          if (fx >= 0 && fx < sc.nx && fy >= 0 && fy < sc.ny && fz >= 0 && fz < sc.nz)
            cell[u] = ((long long)(int)fz * sc.ny + (int)fy) * sc.nx + (int)fx;
        }
      }
    }
    uint32_t dv[MG_MAXU];
#pragma unroll
    for (int u = 0; u < MG_MAXU; ++u) dv[u] = cell[u] >= 0 ? (uint32_t)sc.d2[cell[u]] : 0xffffffffu;
#pragma unroll
    for (int u = 0; u < MG_MAXU; ++u) {
      const int it = u * BLOCK + tid;
      const int c = it / nsph, s = it - c * nsph;
      if (cell[u] >= 0 && dv[u] <= cfg.T[s]) {
        const unsigned pos = atomicAdd(&L.ncand, 1u);
        L.cand[pos] = (uint16_t)(c << 8 | s);
      }
    }
    for (int it = tid; it < nc * npr; it += BLOCK) {
      const int c = it / npr, p = it - c * npr;
      double* pw = L.u.m.pw[c][p];
      prim_world(rb, p, L.u.m.fr[c][rb->prim_body[p]], pw);
      if (m_map && mc->p_map_on[p]) {
        const double fx = floor((pw[0] - sc.ox) / sc.res), fy = floor((pw[1] - sc.oy) / sc.res);
        const double fz = floor((pw[2] - sc.oz) / sc.res);
        if (fx >= 0 && fx < sc.nx && fy >= 0 && fy < sc.ny) {  // (a centre column outside the grid: the term is free)
          const bool zin = fz >= 0 && fz < sc.nz;
          uint32_t dp = 65535u;
          if (zin) dp = (uint32_t)sc.d2[((long long)(int)fz * sc.ny + (int)fy) * sc.nx + (int)fx];
          if (!zin || dp <= cfg.pT[p]) {
            const unsigned pos = atomicAdd(&L.ncand, 1u);
            L.cand[pos] = (uint16_t)(c << 8 | (MAX_SPH + p));
          }
        }
      }
    }
  }
  __syncthreads();
  // 3. self: lanes over the flat pair lists, this wavefront's configurations k * NWAVE + wave interleaved
  if (m_self) {
    const double ms = cfg.ms;
    const int nsp = rb->n_spairs;
    for (int p = lane; p < nsp; p += 64) {
      const uint32_t ab = rb->sp_ab[p];
      const int a = ab & 0xff, b = ab >> 8;
      const double rr = rb->sph_r[a] + rb->sph_r[b];
#pragma unroll
      for (int k = 0; k < MG_CPW; ++k) {
        const int c = k * NWAVE + wave;
        if (c >= nc) continue;
        const double* wa = L.u.m.wc[c][a];
        const double* wb = L.u.m.wc[c][b];
        const double ex = wa[0] - wb[0], ey = wa[1] - wb[1], ez = wa[2] - wb[2];
        const double d = sqrt(ex * ex + ey * ey + ez * ez) - rr;
        if (d <= ms) L.flag[c] = 1;
      }
    }
    const int npp = rb->n_ppairs;
    for (int p = lane; p < npp; p += 64) {
      const uint32_t ps = rb->pp_ps[p];
      const int pr = ps & 0xff, sp = ps >> 8;
      const int ty = rb->prim_type[pr];
      const double* h = &rb->prim_h[pr * 3];
      const double rs = rb->sph_r[sp];
#pragma unroll
      for (int k = 0; k < MG_CPW; ++k) {
        const int c = k * NWAVE + wave;
        if (c >= nc) continue;
        const double* pw = L.u.m.pw[c][pr];
        const double* w = L.u.m.wc[c][sp];
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
        if (d <= ms) L.flag[c] = 1;
      }
    }
  }
  // 4. map.  Word counts of the listed items, MG_PER consecutive ones per lane, and their exclusive scan.
  const int ncand = __builtin_amdgcn_readfirstlane((int)L.ncand);
  if (ncand > 0) {  // (the same in every thread)
    int cnt[MG_PER];
    int sum = 0;
#pragma unroll
    for (int u = 0; u < MG_PER; ++u) {
      const int i = tid * MG_PER + u;
      cnt[u] = 0;
      if (i < ncand) {
        const int code = L.cand[i];
        const int nb = margin_item(rb, sc, cfg, L, code).R.nb;
        if (nb > MG_FLAT) L.big[atomicAdd(&L.nbig, 1u)] = (uint16_t)code;
        else cnt[u] = nb;
      }
      sum += cnt[u];
    }
    const int incl = wave_incl_scan(sum);
    if (lane == 63) L.wsum[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < NWAVE; ++w) {
      const int v = L.wsum[w];
      before += w < wave ? v : 0;
      total += v;
    }
    total = __builtin_amdgcn_readfirstlane(total);
    int run = before + incl - sum;
#pragma unroll
    for (int u = 0; u < MG_PER; ++u) {
      const int i = tid * MG_PER + u;
      if (i < ncand) L.off[i] = run;
      run += cnt[u];
    }
    if (tid == 0) L.off[ncand] = total;
    __syncthreads();
    // the flat pairs: pair p is word p - off[i] of the last item i with off[i] <= p
    for (int p = tid; p < total; p += BLOCK) {
      int lo = 0, hi = ncand - 1;
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (L.off[mid] <= p) lo = mid; else hi = mid - 1;
      }
      const int code = L.cand[lo];
      if (L.flag[code >> 8]) continue;
      const MarginItem I = margin_item(rb, sc, cfg, L, code);
      if (word_violates(rb, sc, cfg, L, I, p - L.off[lo])) L.flag[I.c] = 1;
    }
    // the big items, a wavefront each
    const int nbig = __builtin_amdgcn_readfirstlane((int)L.nbig);
    for (int i = wave; i < nbig; i += NWAVE) {
      const MarginItem I = margin_item(rb, sc, cfg, L, __builtin_amdgcn_readfirstlane((int)L.big[i]));
      for (int b0 = 0; b0 < I.R.nb; b0 += 64) {
        if (L.flag[I.c]) break;
        if (b0 + lane < I.R.nb && word_violates(rb, sc, cfg, L, I, b0 + lane)) L.flag[I.c] = 1;
      }
    }
  }
  __syncthreads();
}

// Stage shared by the three kernels: the model and the map configuration in LDS, the scene's scalars uniform.
#define SMP_MARGIN_PROLOGUE()                                   \
  __shared__ RobotDev s_rb;                                     \
  __shared__ MapCfg s_mc;                                       \
  __shared__ MarginLds L;                                       \
  __shared__ double ql[PASS_CT][NJ];                            \
  const int tid = threadIdx.x;                                  \
  stage_model(rb, mc, &s_rb, &s_mc); /* (ends with a barrier) */ \
  const SceneDev sc = uniform_scene(sc_in)

// The tile's flags as one mask, the same in every wavefront.
__device__ __forceinline__ unsigned long long tile_mask(const MarginLds& L, int nc) {
  const int l = threadIdx.x & 63;
  return __ballot(l < nc && L.flag[l & (PASS_CT - 1)] != 0);
}

// Tiles of 32 configurations (smp_check_configs_margin).
__global__ void __launch_bounds__(BLOCK) margin_configs_kernel(const RobotDev* __restrict__ rb, SceneDev sc_in,
                                                               const MapCfg* __restrict__ mc, MarginCfg cfg,
                                                               const double* __restrict__ q_rows, long long n,
                                                               int n_items, unsigned* __restrict__ counter,
                                                               uint8_t* __restrict__ clear) {
  SMP_MARGIN_PROLOGUE();
  struct Done { long long q0; int nc; unsigned long long mask; };
  ticket_loop(
      counter, (unsigned)n_items,
      [&](unsigned slot) {
        const long long q0 = (long long)slot * PASS_CT;
        const int nc = __builtin_amdgcn_readfirstlane((int)min((long long)PASS_CT, n - q0));
        for (int it = tid; it < nc * NJ; it += BLOCK) {
          const int c = it / NJ, j = it - c * NJ;
          ql[c][j] = q_rows[(q0 + c) * NJ + j];
        }
        __syncthreads();
        margin_tile(&s_rb, sc_in, sc, &s_mc, cfg, nc, ql, L);  // (ends with a barrier)
        const unsigned long long mask = tile_mask(L, nc);
        __syncthreads();  // ql and the flags are rewritten by the next tile
        return Done{q0, nc, mask};
      },
      [&](unsigned, const Done& d) {
        for (int c = 0; c < d.nc; ++c) clear[d.q0 + c] = (uint8_t)(((d.mask >> c) & 1ull) ? 0 : 1);
      });
}

// The base's free map at a map margin (base_map_kernel's tiles, smp_lattice.hip): item t is the tile of lattice nodes
// 32 t .. and bits[t] its word, bit c set iff node 32 t + c is clear.  cfg asks for the map part alone.
__global__ void __launch_bounds__(BLOCK) margin_base_map_kernel(const RobotDev* __restrict__ rb, SceneDev sc_in,
                                                                const MapCfg* __restrict__ mc, MarginCfg cfg,
                                                                LatticeDev lat, int n_items,
                                                                unsigned* __restrict__ counter,
                                                                uint32_t* __restrict__ bits) {
  SMP_MARGIN_PROLOGUE();
  (void)tid;  // (lattice_tile and tile_mask index by thread themselves)
  ticket_loop(
      counter, (unsigned)n_items,
      [&](unsigned slot) {
        const long long n0 = (long long)slot * PASS_CT;
        const int nc = __builtin_amdgcn_readfirstlane((int)min((long long)PASS_CT, lat.n - n0));
        lattice_tile(ql, lat, n0, nc);
        __syncthreads();
        margin_tile(&s_rb, sc_in, sc, &s_mc, cfg, nc, ql, L);  // (ends with a barrier)
        const unsigned long long mask = tile_mask(L, nc);
        __syncthreads();  // ql and the flags are rewritten by the next tile
        return lattice_word(mask, nc);
      },
      [&](unsigned slot, uint32_t word) { bits[slot] = word; });
}

// Dense edges (edges_kernel's walk): the first tile that holds a point that is not clear ends the edge.
__global__ void __launch_bounds__(BLOCK) margin_edges_kernel(const RobotDev* __restrict__ rb, SceneDev sc_in,
                                                             const MapCfg* __restrict__ mc, MarginCfg cfg,
                                                             const EdgeDev* __restrict__ edges,
                                                             const int* __restrict__ order, int n,
                                                             unsigned* __restrict__ counter,
                                                             int* __restrict__ first_invalid) {
  SMP_MARGIN_PROLOGUE();
  __shared__ double ea[NJ], es[NJ];  // the edge's start and its step (b - a) / M
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
        for (int base = 0; base <= M && first < 0; base += PASS_CT) {
          const int nc = __builtin_amdgcn_readfirstlane(min(PASS_CT, M + 1 - base));
          edge_tile(ql, ea, es, base, nc);
          __syncthreads();
          margin_tile(&s_rb, sc_in, sc, &s_mc, cfg, nc, ql, L);  // (ends with a barrier)
          const unsigned long long hit = tile_mask(L, nc);
          if (hit) first = __builtin_amdgcn_readfirstlane(base + (int)__builtin_ctzll(hit));
          __syncthreads();  // the flags and ql are rewritten by the next tile
        }
        return Done{e, first};
      },
      [&](unsigned, const Done& d) { first_invalid[d.e] = d.first; });
}

// Detour items: detours_kernel's draw, leg order and record.
__global__ void __launch_bounds__(BLOCK) margin_detours_kernel(const RobotDev* __restrict__ rb, SceneDev sc_in,
                                                               const MapCfg* __restrict__ mc, MarginCfg cfg,
                                                               const GapDev* __restrict__ gaps, DetourArgs A,
                                                               unsigned* __restrict__ counter,
                                                               DetourDev* __restrict__ out) {
  SMP_MARGIN_PROLOGUE();
  __shared__ double ea[2][NJ], es[2][NJ];  // start and step of the legs a -> v (0) and v -> b (1): ea[1] is v
  __shared__ double eb[NJ];                // b
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
          const int T1 = (M1 + PASS_CT) / PASS_CT, T2 = (M2 + PASS_CT) / PASS_CT;  // tiles of M + 1 points
          for (int t = 0; t < T1 + T2 && !blocked; ++t) {
            const int leg = t < T2 ? 1 : 0;
            const int base = leg ? t * PASS_CT : (T1 - 1 - (t - T2)) * PASS_CT;
            const int nc = __builtin_amdgcn_readfirstlane(min(PASS_CT, (leg ? M2 : M1) + 1 - base));
            edge_tile(ql, ea[leg], es[leg], base, nc);
            __syncthreads();
            margin_tile(&s_rb, sc_in, sc, &s_mc, cfg, nc, ql, L);  // (ends with a barrier)
            if (tile_mask(L, nc)) blocked = 1;
            __syncthreads();  // the flags and ql are rewritten by the next tile
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

size_t margin_kernels_private_bytes() {
  return std::max(std::max(kernel_private_bytes(&margin_configs_kernel), kernel_private_bytes(&margin_base_map_kernel)),
                  std::max(kernel_private_bytes(&margin_edges_kernel), kernel_private_bytes(&margin_detours_kernel)));
}

void launch_margin_configs(int grid, hipStream_t st, const RobotDev* rb, SceneDev sc, const MapCfg* mc,
                           const MarginCfg& cfg, const double* q_rows, long long n, int n_items, unsigned* counter,
                           uint8_t* clear) {
  hipLaunchKernelGGL(margin_configs_kernel, dim3(grid), dim3(BLOCK), 0, st, rb, sc, mc, cfg, q_rows, n, n_items, counter,
                     clear);
}

void launch_margin_base_map(int grid, hipStream_t st, const RobotDev* rb, SceneDev sc, const MapCfg* mc,
                            const MarginCfg& cfg, LatticeDev lat, int n_items, unsigned* counter, uint32_t* bits) {
  hipLaunchKernelGGL(margin_base_map_kernel, dim3(grid), dim3(BLOCK), 0, st, rb, sc, mc, cfg, lat, n_items, counter,
                     bits);
}

void launch_margin_edges(int grid, hipStream_t st, const RobotDev* rb, SceneDev sc, const MapCfg* mc,
                         const MarginCfg& cfg, const EdgeDev* edges, const int* order, int n, unsigned* counter,
                         int* first_invalid) {
  hipLaunchKernelGGL(margin_edges_kernel, dim3(grid), dim3(BLOCK), 0, st, rb, sc, mc, cfg, edges, order, n, counter,
                     first_invalid);
}

void launch_margin_detours(int grid, hipStream_t st, const RobotDev* rb, SceneDev sc, const MapCfg* mc,
                           const MarginCfg& cfg, const GapDev* gaps, DetourArgs args, unsigned* counter, DetourDev* out) {
  hipLaunchKernelGGL(margin_detours_kernel, dim3(grid), dim3(BLOCK), 0, st, rb, sc, mc, cfg, gaps, args, counter, out);
}

}  // namespace smp
