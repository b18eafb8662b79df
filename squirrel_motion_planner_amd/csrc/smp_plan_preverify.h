// SMP_PRE_VERIFY builds (debugging; tools/preverify_probe.py): every decision pre_commit takes from a record is
// recomputed the full way and compared.  Relies on the scans, edge batches, via chains and tree updates.
// Included by smp_kernels.hip only, once, ahead of pre_commit.
#pragma once

namespace smp {

#ifdef SMP_PRE_VERIFY
// Debugging build: every record-committed decision is recomputed the full way and compared; g_pv[0] counts checks,
// g_pv[1] holds the first mismatch: iteration | kind << 40 (1 nearest, 2 expand edge, 3 connect nearest, 4 connect
// edge, 5 x_new / edge costs) | block << 48; read by smp_debug_preverify.
__device__ unsigned long long g_pv[4];
__device__ void pv_fail(int kind) {
  if (threadIdx.x == 0)
    atomicCAS(&g_pv[1], 0ull, (unsigned long long)g_L.S.iter | ((unsigned long long)kind << 40) |
                                  ((unsigned long long)blockIdx.x << 48));
}
__device__ void pre_verify_expand(const Ctx& C, int A) {
  const PreRec& P = g_L.prer;
  double d;
  int full = nearest_scan(C, A, g_L.xr, 0, &d);
  full = d < 10000.0 ? full : 0;
  if (threadIdx.x == 0) atomicAdd(&g_pv[0], 1ull);
  if (uni(full != (P.nn_d < 10000.0 ? P.nn_id : 0))) pv_fail(1);
  if (threadIdx.x == 0) {
    NodeRef nn;
    load_node(C, A, full, &nn);
    for (int j = 0; j < NJ; ++j) { g_L.ext[j] = g_L.xr[j]; }
    step_towards((&g_rb), nn.q, g_L.ext, g_L.S.step);
    for (int j = 0; j < NJ; ++j) { g_L.eg_start[0][j] = nn.q[j]; g_L.eg_target[0][j] = g_L.ext[j]; }
    for (int k = 0; k < 3; ++k) g_L.eg_base[0][k] = nn.c[k];
    g_L.eg_need[0] = 1;
    g_L.rec_grp = -1;
  }
  for (int e = 1 + threadIdx.x; e < MAXE; e += BLOCK) g_L.eg_need[e] = 0;
  __syncthreads();
  edge_costs(C, 1);
  edge_validity(C, 1, false, P_XEXPAND);
  bool bad_costs = false;
  for (int j = 0; j < NJ; ++j) bad_costs |= g_L.eg_end[0][j] != P.end[j] || g_L.eg_start[0][j] != P.nn_q[j];
  for (int k = 0; k < 3; ++k) bad_costs |= g_L.eg_cost[0][k] != P.nn_c[k] + P.acc[k];
  if (uni(g_L.eg_first[0] != P.first)) pv_fail(2);
  if (uni(bad_costs)) pv_fail(5);
  __syncthreads();
}
__device__ void pre_verify_connect(const Ctx& C, int B, int cid) {
  const PreRec& P = g_L.prer;
  double d;
  int full = nearest_scan(C, B, g_L.xn.q, 0, &d);
  full = d < 10000.0 ? full : 0;
  if (uni(full != cid)) pv_fail(3);
  if (threadIdx.x == 0) {
    NodeRef xc;
    load_node(C, B, full, &xc);
    for (int j = 0; j < NJ; ++j) { g_L.eg_start[0][j] = xc.q[j]; g_L.eg_target[0][j] = g_L.xn.q[j]; }
    for (int k = 0; k < 3; ++k) g_L.eg_base[0][k] = xc.c[k];
    g_L.eg_need[0] = 1;
    g_L.rec_grp = -1;
  }
  for (int e = 1 + threadIdx.x; e < MAXE; e += BLOCK) g_L.eg_need[e] = 0;
  __syncthreads();
  edge_costs(C, 1);
  edge_validity(C, 1, false, P_XCONNECT);
  if (uni(P.pre_ok && P.need && g_L.eg_first[0] != P.cn_first)) pv_fail(4);
  __syncthreads();
  if (!uni(P.pre_ok)) return;
  // the connect outcome the full path would take (connect_graphs without a solution): flag, via chain, last node
  if (threadIdx.x == 0) {
    QState& S = g_L.S;
    double sol[3];
    for (int k = 0; k < 3; ++k) sol[k] = g_L.eg_cost[0][k] + g_L.xn.c[k];
    const int need = sol[0] < S.cbest[0];
    int flag = 0;
    if (need) {
      const int f = g_L.eg_first[0];
      if (f > S.n_pts) flag = 1;
      else {
        const int lv = f == 0 ? 0 : f - 1;
        if (lv != 0) { for (int j = 0; j < NJ; ++j) g_L.ext[j] = g_L.eg_start[0][j] + lv * g_L.eg_step[0][j]; flag = 2; }
      }
    }
    bool bad = need != P.need || flag != P.flag;
    for (int k = 0; k < 3; ++k) bad |= sol[k] != P.sol[k];
    if (bad) pv_fail(8);
    g_L.flag = flag;
    g_L.n_via = 0;
    g_L.nn_t = S.n[B];
    load_node(C, B, cid, &g_L.cur);
  }
  __syncthreads();
  const int flag = uni(g_L.flag);
  if (!flag) return;
  via_chain(C, flag == 1 ? g_L.xn.q : g_L.ext);
  if (threadIdx.x == 0) {
    const int par = (int)(g_L.S.iter & (SCOUT_SLOTS - 1));
    const ScoutBoard* sb = C.Q.scbs[g_L.asked[par] - 1];
    const int off = g_L.S.n[B] - P.XB;
    bool bad = g_L.n_via != P.nv;
    for (int k = 0; k < g_L.n_via && k < P.nv && !bad; ++k) {
      const ViaNode& a = C.Q.via[k];
      const ViaNode& b = sb->pre_via[par][k];
      for (int j = 0; j < NJ; ++j)
        bad |= a.q[j] != __longlong_as_double((long long)ld_agent((const unsigned long long*)&b.q[j])) ||
               a.e_start[j] != __longlong_as_double((long long)ld_agent((const unsigned long long*)&b.e_start[j])) ||
               a.e_target[j] != __longlong_as_double((long long)ld_agent((const unsigned long long*)&b.e_target[j]));
      for (int c = 0; c < 3; ++c) bad |= a.c[c] != __longlong_as_double((long long)ld_agent((const unsigned long long*)&b.c[c]));
      const int bid = ld_agent(&b.id), bpar = ld_agent(&b.parent);
      bad |= a.id != (bid >= P.XB ? bid + off : bid) || a.parent != (bpar >= P.XB ? bpar + off : bpar);
    }
    if (bad) pv_fail(6);
    bool bs = false;
    for (int j = 0; j < NJ; ++j) bs |= g_L.sel.q[j] != P.sel_q[j] || g_L.sel_start[j] != P.sel_start[j] || g_L.sel_target[j] != P.sel_target[j];
    for (int k = 0; k < 3; ++k) bs |= g_L.sel.c[k] != P.sel_c[k];
    bs |= g_L.sel.id != (P.sel_id >= P.XB ? P.sel_id + off : P.sel_id);
    bs |= g_L.sel.parent != (P.sel_parent >= P.XB ? P.sel_parent + off : P.sel_parent);
    if (bs) pv_fail(7);
    g_L.n_via = 0;
  }
  __syncthreads();
}
#define PRE_VERIFY_EXPAND(C, A) pre_verify_expand(C, A)
#define PRE_VERIFY_CONNECT(rec, C, B, cid) if (rec) pre_verify_connect(C, B, cid)
#else
#define PRE_VERIFY_EXPAND(C, A)
#define PRE_VERIFY_CONNECT(rec, C, B, cid)
#endif

}  // namespace smp
