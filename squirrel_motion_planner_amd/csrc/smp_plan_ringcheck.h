// SMP_RING_CHECK builds (debugging; tools/divergence_probe.py): the leader recomputes every sample it takes from the
// ring or a record and compares; the sampler leaves the parameters of each slot's sample.  Counts in prof[28..30] and
// g_ringchk, printed by smp_ringchk_dump.  Relies on the job protocol's agent-scope loads and stores; calls the sampling
// functions that follow it.  Included by smp_kernels.hip only, once, ahead of its sampling section.
#pragma once

namespace smp {

#ifdef SMP_RING_CHECK
__device__ unsigned long long g_ringchk[64];
__device__ unsigned long long g_ringdbg[SMP_RING][16];  // sampler: parameters of the slot's sample
extern "C" void smp_ringchk_dump() {
  unsigned long long v[64];
  if (hipMemcpyFromSymbol(v, HIP_SYMBOL(g_ringchk), sizeof(v)) == hipSuccess) {
    double d[64];
    __builtin_memcpy(d, v, sizeof(d));
    std::fprintf(stderr, "[smp] ring check: uniform(it) %llu, it-1 %llu, it+1 %llu, other %llu; first mismatch it %llu\n",
                 v[0], v[1], v[2], v[3], v[4]);
    std::fprintf(stderr, "[smp]   ring  :");
    for (int j = 0; j < 8; ++j) std::fprintf(stderr, " %.17g", d[24 + j]);
    std::fprintf(stderr, "\n[smp]   leader:");
    for (int j = 0; j < 8; ++j) std::fprintf(stderr, " %.17g", d[32 + j]);
    std::fprintf(stderr, "\n[smp]   sampler h0 %.17g Crev0 %.17g Crev7 %.17g ctr0 %.17g qmin2 %.17g qmax2 %.17g rev %llx\n",
                 d[40], d[41], d[42], d[43], d[44], d[45], v[46]);
    std::fprintf(stderr, "[smp]   leader  h0 %.17g Crev0 %.17g Crev7 %.17g ctr0 %.17g qmin2 %.17g qmax2 %.17g rev %llx\n",
                 d[48], d[49], d[50], d[51], d[52], d[53], v[54]);
  }
}
__device__ __forceinline__ int sample_uniform(const QState& S, uint32_t it, SmpLds& W, double* out);
__device__ __forceinline__ int sample_conf(const QState& S, uint32_t it, SmpLds& W, double* out);
// sample_read, a sample taken from the ring or a record (g_L.xr): recomputed here and compared.  All threads.
__device__ __forceinline__ void ring_check_sample(QState& S, const uint32_t it) {
  __shared__ double chk_xr[NJ];
  __shared__ int chk_bad;
  sample_conf(S, it, g_L.u.smp, chk_xr);
  if (threadIdx.x == 0) {
    int bad = 0;
    for (int j = 0; j < NJ; ++j) bad |= __double_as_longlong(chk_xr[j]) != __double_as_longlong(g_L.xr[j]);
    chk_bad = bad;
    S.prof[P_RING_CHECKS]++;
    if (bad) { S.prof[P_RING_BAD]++; if (!S.prof[P_RING_FIRST]) S.prof[P_RING_FIRST] = (unsigned long long)it + 1; }
    if (bad && g_ringchk[21] == 0) {
      const RobotDev* rb = (&g_rb);
      g_ringchk[21] = 1;
      g_ringchk[4] = (unsigned long long)it;
      for (int j = 0; j < NJ; ++j) {
        g_ringchk[24 + j] = (unsigned long long)__double_as_longlong(g_L.xr[j]);
        g_ringchk[32 + j] = (unsigned long long)__double_as_longlong(chk_xr[j]);
      }
      for (int k = 0; k < 7; ++k) g_ringchk[40 + k] = ld_agent(&g_ringdbg[it % SMP_RING][8 + k]);
      const double lv[6] = {S.h0[1], S.Crev[0], S.Crev[7], S.ctr_rev[0], rb->q_min[2], rb->q_max[2]};
      for (int k = 0; k < 6; ++k) g_ringchk[48 + k] = (unsigned long long)__double_as_longlong(lv[k]);
      unsigned long long rv = 0;
      for (int j = 0; j < NJ; ++j) rv |= (unsigned long long)(rb->rev[j] != 0) << j;
      g_ringchk[54] = rv;
    }
  }
  __syncthreads();
  if (uni(chk_bad)) {  // which sample the ring held: prof[20] the uniform one of this iteration, [21] iteration
    // it - 1's, [22] it + 1's (current parameters), [23] none of them
    int cls = 23;
    for (int v = 0; v < 3 && cls == 23; ++v) {
      if (v == 0) sample_uniform(S, it, g_L.u.smp, chk_xr);
      else sample_conf(S, v == 1 ? it - 1 : it + 1, g_L.u.smp, chk_xr);
      if (threadIdx.x == 0) {
        int same = 1;
        for (int j = 0; j < NJ; ++j) same &= __double_as_longlong(chk_xr[j]) == __double_as_longlong(g_L.xr[j]);
        chk_bad = same;
      }
      __syncthreads();
      if (uni(chk_bad)) cls = 20 + v;
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      g_ringchk[cls - 20]++;
    }
    __syncthreads();
  }
}
// The sampler, after the sample of iteration `it`: the parameters it was drawn with, for the leader's report.
__device__ __forceinline__ void ring_check_params(const SamplerLds& L, const long long it) {
  if (threadIdx.x == 0) {
    unsigned long long* d = g_ringdbg[it % SMP_RING];
    st_agent(&d[0], (unsigned long long)it); st_agent(&d[1], (unsigned long long)L.ver);
    st_agent(&d[2], (unsigned long long)L.S.have_sol);
    for (int k = 0; k < 3; ++k) st_agent(&d[3 + k], (unsigned long long)__double_as_longlong(L.S.cbest[k]));
    st_agent(&d[6], (unsigned long long)L.S.informed);
    const RobotDev* rb = (&g_rb);
    const double lv[6] = {L.S.h0[1], L.S.Crev[0], L.S.Crev[7], L.S.ctr_rev[0], rb->q_min[2], rb->q_max[2]};
    for (int k = 0; k < 6; ++k) st_agent(&d[8 + k], (unsigned long long)__double_as_longlong(lv[k]));
    unsigned long long rv = 0;
    for (int j = 0; j < NJ; ++j) rv |= (unsigned long long)(rb->rev[j] != 0) << j;
    st_agent(&d[14], rv);
  }
}
#else  // the product build: both calls are empty
__device__ __forceinline__ void ring_check_sample(QState&, uint32_t) {}
__device__ __forceinline__ void ring_check_params(const SamplerLds&, long long) {}
#endif

}  // namespace smp
