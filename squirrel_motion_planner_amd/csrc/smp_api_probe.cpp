// C ABI implementation (include/smp_gpu.h), test hooks: the smp_probe_* entry points (state export for the oracle,
// parity and latency probes of the kernels' shared arithmetic and tiles).
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "smp_kernels.h"
#include "smp_planner.h"

using namespace smp;

// The state of the last call's query 0 in the oracle's terms (test infrastructure, DESIGN.md "Large trees": the oracle continues
// the same run from it, orc_resume_*): per tree the child lists (first child, next sibling: the GPU inserts children
// at the head, so the reference's out-edge order is the list reversed) and every node's in-edge (interpolation start
// and target, n x 8 row-major); then the loop scalars (iv: iteration, checked, valid, first_iter, last_iter,
// have_sol, conn_start, tree_A of the next iteration, nB id / parent, nA id / parent, edges / rewires of both trees;
// dv: c_best[3], nB q[8] / cost[3], nA q[8] / cost[3]).
extern "C" int smp_probe_export_tree(smp_planner* p, int which, int32_t* first_child, int32_t* next_sib,
                                     double* e_start, double* e_target) {
  if (!p || p->qb.empty() || which < 0 || which > 1) return SMP_ERR_ARG;
  if (int b_ = busy_check(const_cast<smp_planner*>(p))) return b_;
  HIPCHK(hipSetDevice(p->device));
  QueryBuffers& b = p->qb[0];
  const size_t cap = b.cap;
  const int n = p->last_n[which];
  if (first_child) HIPCHK(hipMemcpy(first_child, b.first_child.p + which * cap, n * sizeof(int), hipMemcpyDeviceToHost));
  if (next_sib) HIPCHK(hipMemcpy(next_sib, b.next_sib.p + which * cap, n * sizeof(int), hipMemcpyDeviceToHost));
  std::vector<double> tmp((size_t)n);
  double* const outs[2] = {e_start, e_target};
  double* const srcs[2] = {b.e_start.p, b.e_target.p};
  for (int o = 0; o < 2; ++o) {
    if (!outs[o]) continue;
    for (int j = 0; j < NJ; ++j) {
      HIPCHK(hipMemcpy(tmp.data(), srcs[o] + which * cap * NJ + (size_t)j * cap, n * sizeof(double), hipMemcpyDeviceToHost));
      for (int i = 0; i < n; ++i) outs[o][(size_t)i * NJ + j] = tmp[i];
    }
  }
  return SMP_OK;
}

extern "C" int smp_probe_export_state(smp_planner* p, int64_t* iv, double* dv) {
  if (!p || p->qb.empty() || !iv || !dv) return SMP_ERR_ARG;
  if (int b_ = busy_check(const_cast<smp_planner*>(p))) return b_;
  HIPCHK(hipSetDevice(p->device));
  QState S;
  HIPCHK(hipMemcpy(&S, p->qb[0].st.p, sizeof(QState), hipMemcpyDeviceToHost));
  iv[0] = S.iter; iv[1] = S.checked; iv[2] = S.valid; iv[3] = S.first_iter; iv[4] = S.last_iter;
  iv[5] = S.have_sol; iv[6] = S.conn_start; iv[7] = S.A;
  iv[8] = S.nB.id; iv[9] = S.nB.parent; iv[10] = S.nA.id; iv[11] = S.nA.parent;
  iv[12] = S.edges[0]; iv[13] = S.edges[1]; iv[14] = S.rewires[0]; iv[15] = S.rewires[1];
  dv[0] = S.cbest[0]; dv[1] = S.cbest[1]; dv[2] = S.cbest[2];
  const NodeRef* nb[2] = {&S.nB, &S.nA};
  for (int k = 0; k < 2; ++k) {
    for (int j = 0; j < NJ; ++j) dv[3 + 11 * k + j] = nb[k]->q[j];
    for (int c = 0; c < 3; ++c) dv[11 + 11 * k + c] = nb[k]->c[c];
  }
  return SMP_OK;
}

// ------------------------------------------------------------------------------------------ parity probes
// The per-primitive slab fields a planner would build for this robot and scene (n_prim x ny x nx), host only.
extern "C" int64_t smp_probe_scene_slabs(const smp_robot* r, const smp_scene* s, uint16_t* out, int64_t cap) {
  if (!r || !s) return SMP_ERR_ARG;
  std::vector<std::vector<uint16_t>> slabs;
  prim_slabs(r->h.dev, s->h, &slabs);
  int64_t n = 0;
  for (auto& v : slabs) {
    if (out && n + (int64_t)v.size() <= cap) std::memcpy(out + n, v.data(), v.size() * sizeof(uint16_t));
    n += (int64_t)v.size();
  }
  return n;
}

// The device model of a robot (tests: the URDF + SRDF path and the JSON path give the same bytes).  Host only.
extern "C" int64_t smp_probe_robot_dev(const smp_robot* r, void* out, int64_t cap) {
  if (!r) return SMP_ERR_ARG;
  if (out && cap >= (int64_t)sizeof(RobotDev)) std::memcpy(out, &r->h.dev, sizeof(RobotDev));
  return (int64_t)sizeof(RobotDev);
}

// Device evaluations of the shared arithmetic (tests only): portable sin/cos, the Philox draw, body FK,
// end-effector z and the fp64 sqrt / division used throughout.
extern "C" int smp_probe_sincos(int device, const double* x, int n, double* s, double* c) {
  if (hipSetDevice(device) != hipSuccess) return SMP_ERR_NO_DEVICE;
  double *dx, *ds, *dc;
  HIPCHK(hipMalloc(&dx, n * sizeof(double))); HIPCHK(hipMalloc(&ds, n * sizeof(double))); HIPCHK(hipMalloc(&dc, n * sizeof(double)));
  HIPCHK(hipMemcpy(dx, x, n * sizeof(double), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(sincos_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, dx, n, ds, dc);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(s, ds, n * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(c, dc, n * sizeof(double), hipMemcpyDeviceToHost));
  (void)hipFree(dx); (void)hipFree(ds); (void)hipFree(dc);
  return SMP_OK;
}

extern "C" int smp_probe_u01(int device, uint64_t seed, uint32_t query, const uint32_t* ctr, int n, double* out) {
  if (hipSetDevice(device) != hipSuccess) return SMP_ERR_NO_DEVICE;
  uint32_t* dc;
  double* d;
  HIPCHK(hipMalloc(&dc, 4 * n * sizeof(uint32_t))); HIPCHK(hipMalloc(&d, n * sizeof(double)));
  HIPCHK(hipMemcpy(dc, ctr, 4 * n * sizeof(uint32_t), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(u01_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, (unsigned long long)seed, query, dc, n, d);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(out, d, n * sizeof(double), hipMemcpyDeviceToHost));
  (void)hipFree(dc); (void)hipFree(d);
  return SMP_OK;
}

extern "C" int smp_probe_fk(smp_planner* p, const double* q, int n, double* frames, double* eez) {
  if (!p) return SMP_ERR_ARG;
  if (int b_ = busy_check(const_cast<smp_planner*>(p))) return b_;
  HIPCHK(hipSetDevice(p->device));
  int nb = p->robot.dev.n_body;
  double *dq, *df, *dz;
  HIPCHK(hipMalloc(&dq, (size_t)n * NJ * sizeof(double)));
  HIPCHK(hipMalloc(&df, (size_t)n * nb * 12 * sizeof(double)));
  HIPCHK(hipMalloc(&dz, (size_t)n * sizeof(double)));
  HIPCHK(hipMemcpy(dq, q, (size_t)n * NJ * sizeof(double), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(fk_kernel, dim3((n + 127) / 128), dim3(128), 0, 0, p->d_rb, dq, n, df, dz);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(frames, df, (size_t)n * nb * 12 * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(eez, dz, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  (void)hipFree(dq); (void)hipFree(df); (void)hipFree(dz);
  return SMP_OK;
}

// Latency probe of the collision tile: check_kernel with `grid` workgroups (grid 1: one workgroup streams
// every tile back to back); ticks[0..3] = block 0's device-clock ticks in tile stages A, B, C-centres, C;
// ticks[4] / ticks[5] = block 0's shader cycles / device-clock ticks over the kernel (effective shader clock);
// ticks[6..] = wave 0's detail clocks (collide_tile: centres + map sweeps, self test; collide_wide (tile < 0), eight:
// prefilter loads, primitives' brick loads, primitive sweeps, staged spheres' slots and brick loads, sphere sweeps, self
// test, the tile's end after wave 0's, work in between).  `ticks` holds 16 entries.
extern "C" int smp_probe_check_latency(smp_planner* p, const double* q_soa, int64_t n, int check_self, int check_map,
                                       int grid, int tile, double* ms, unsigned long long* ticks, double* clock_hz) {
  if (!p || n <= 0 || !q_soa || grid <= 0) return SMP_ERR_ARG;
  if (int b_ = busy_check(const_cast<smp_planner*>(p))) return b_;
  HIPCHK(hipSetDevice(p->device));
  HIPCHK(p->d_cq.reserve((size_t)n * NJ));
  HIPCHK(p->d_valid.reserve((size_t)n));
  unsigned long long* dprof = nullptr;
  HIPCHK(hipMalloc(&dprof, 16 * sizeof(unsigned long long)));
  HIPCHK(hipMemset(dprof, 0, 16 * sizeof(unsigned long long)));
  HIPCHK(hipMemcpy(p->d_cq.p, q_soa, (size_t)n * NJ * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipEventRecord(p->ev0, p->stream));
  launch_check(tile, grid, p->stream, p->d_rb, p->sc, p->d_mc, p->d_cq.p, (long long)n, check_self,
               check_map && p->have_scene, p->d_valid.p, dprof);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(p->ev1, p->stream));
  HIPCHK(hipStreamSynchronize(p->stream));
  float f = 0;
  HIPCHK(hipEventElapsedTime(&f, p->ev0, p->ev1));
  *ms = f;
  HIPCHK(hipMemcpy(ticks, dprof, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  (void)hipFree(dprof);
  *clock_hz = p->wall_rate_hz;
  return SMP_OK;
}

// Validity flags of n configurations checked in tiles of the given shape (launch_check: 8 / 16 / 32 = the batch
// checker's collide_tile, -1 / -2 / -4 / -8 = the job tiles' collide_wide with that many configurations): the parity
// test of the job-tile shapes against the batch checker (tests/test_gpu_parity.py).
extern "C" int smp_probe_check_shape(smp_planner* p, const double* q_soa, int64_t n, int check_self, int check_map,
                                     int tile, int grid, uint8_t* valid) {
  if (!p || n <= 0 || !q_soa || !valid || grid <= 0) return SMP_ERR_ARG;
  if (int b_ = busy_check(const_cast<smp_planner*>(p))) return b_;
  if (!(tile == 8 || tile == 16 || tile == 32 || tile == -1 || tile == -2 || tile == -4 || tile == -8)) return SMP_ERR_ARG;
  HIPCHK(hipSetDevice(p->device));
  HIPCHK(p->d_cq.reserve((size_t)n * NJ));
  HIPCHK(p->d_valid.reserve((size_t)n));
  HIPCHK(hipMemcpyAsync(p->d_cq.p, q_soa, (size_t)n * NJ * sizeof(double), hipMemcpyHostToDevice, p->stream));
  launch_check(tile, grid, p->stream, p->d_rb, p->sc, p->d_mc, p->d_cq.p, (long long)n, check_self,
               check_map && p->have_scene, p->d_valid.p, nullptr);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(valid, p->d_valid.p, (size_t)n, hipMemcpyDeviceToHost, p->stream));
  HIPCHK(hipStreamSynchronize(p->stream));
  return SMP_OK;
}

extern "C" int smp_probe_sqrt_div(int device, const double* a, const double* b, int n, double* sq, double* dv) {
  if (hipSetDevice(device) != hipSuccess) return SMP_ERR_NO_DEVICE;
  double *da, *db, *ds, *dd;
  HIPCHK(hipMalloc(&da, n * sizeof(double))); HIPCHK(hipMalloc(&db, n * sizeof(double)));
  HIPCHK(hipMalloc(&ds, n * sizeof(double))); HIPCHK(hipMalloc(&dd, n * sizeof(double)));
  HIPCHK(hipMemcpy(da, a, n * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(db, b, n * sizeof(double), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(sqrt_div_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, da, db, n, ds, dd);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(sq, ds, n * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(dv, dd, n * sizeof(double), hipMemcpyDeviceToHost));
  (void)hipFree(da); (void)hipFree(db); (void)hipFree(ds); (void)hipFree(dd);
  return SMP_OK;
}

// Tree-scan probe (near_probe_kernel): nearest and near_set<20> of m queries against one tree of n nodes
// (q_soa [NJ][n], cost [n]); lo / hi: m x 20 ids (-1 padded); ticks[2]: device-clock ticks of all nearest /
// near_set calls (clock_hz ticks per second); ticks[2..13]: the workgroup's profiling slots 20..31 (SMP_NEAR_PROF
// builds: near_set step clocks and path counts).
extern "C" int smp_probe_near(int device, const double* q_soa, const double* cost, int n, const double* queries,
                              const int* excl, int m, double r, int reps, int* nn, int* nk, int* lo, int* hi,
                              unsigned long long* ticks, double* clock_hz) {
  // reps < 0: the distributed scans' slice functions over the whole tree (tools/slice_probe.py)
  if (n <= 0 || m <= 0 || reps == 0 || !q_soa || !cost || !queries || !excl) return SMP_ERR_ARG;
  if (hipSetDevice(device) != hipSuccess) return SMP_ERR_NO_DEVICE;
  double *dq, *dc, *dqq;
  int *dx, *dnn, *dnk, *dlo, *dhi;
  unsigned long long* dt;
  HIPCHK(hipMalloc(&dq, (size_t)n * NJ * sizeof(double)));
  HIPCHK(hipMalloc(&dc, (size_t)n * sizeof(double)));
  HIPCHK(hipMalloc(&dqq, (size_t)m * NJ * sizeof(double)));
  HIPCHK(hipMalloc(&dx, (size_t)m * sizeof(int)));
  HIPCHK(hipMalloc(&dnn, (size_t)m * sizeof(int)));
  HIPCHK(hipMalloc(&dnk, (size_t)m * sizeof(int)));
  HIPCHK(hipMalloc(&dlo, (size_t)m * 20 * sizeof(int)));
  HIPCHK(hipMalloc(&dhi, (size_t)m * 20 * sizeof(int)));
  HIPCHK(hipMalloc(&dt, 14 * sizeof(unsigned long long)));
  HIPCHK(hipMemcpy(dq, q_soa, (size_t)n * NJ * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dc, cost, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dqq, queries, (size_t)m * NJ * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dx, excl, (size_t)m * sizeof(int), hipMemcpyHostToDevice));
  // the tree's fp32 copy (TreeDev::qf: the planner writes it with every node)
  std::vector<float> qf((size_t)n * NJ);
  for (size_t k = 0; k < qf.size(); ++k) qf[k] = (float)q_soa[k];
  float* dqf;
  HIPCHK(hipMalloc(&dqf, qf.size() * sizeof(float)));
  HIPCHK(hipMemcpy(dqf, qf.data(), qf.size() * sizeof(float), hipMemcpyHostToDevice));
  // modes 4 / 5 (the helpers' inlined slice forms) run in a kernel of their own, so that neither kernel's register
  // allocation carries the other's code
  const bool inl = reps < 0 && 1 + ((-reps) >> 20) >= 4;
  hipLaunchKernelGGL(inl ? near_probe_inl_kernel : near_probe_kernel, dim3(1), dim3(BLOCK), 0, 0, dq, dc, n, n, dqq, dx,
                     m, r, reps, dnn, dnk, dlo, dhi, dt, (const float*)dqf);
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(nn, dnn, (size_t)m * sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(nk, dnk, (size_t)m * sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(lo, dlo, (size_t)m * 20 * sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(hi, dhi, (size_t)m * 20 * sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(ticks, dt, 14 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  (void)hipFree(dq); (void)hipFree(dc); (void)hipFree(dqq); (void)hipFree(dx); (void)hipFree(dnn);
  (void)hipFree(dnk); (void)hipFree(dlo); (void)hipFree(dhi); (void)hipFree(dt); (void)hipFree(dqf);
  int dev_clock_khz = 0;
  HIPCHK(hipDeviceGetAttribute(&dev_clock_khz, hipDeviceAttributeWallClockRate, device));
  *clock_hz = dev_clock_khz * 1000.0;
  return SMP_OK;
}
