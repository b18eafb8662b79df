// C ABI implementation (include/smp_gpu.h "Far goals"): the cost field of a base lattice on the device and the route
// read off it -- smp_base_cost_field, smp_base_route_gpu (kernels: smp_field.hip; the tile geometry, the round cap, the
// fallback test and the host forms: smp_field.h; snapping, weights and the call's buffers: smp_route.h).
//
// The round loop.  A round is one launch; the host enqueues FIELD_BATCH of them, each with its own changed counter, and
// reads the counters once per batch.  The first round whose counter is 0 is the fixed point's certificate; the rounds
// enqueued after it found no flag set and cost an empty launch each.  field_round_cap bounds the loop.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "smp_field.h"
#include "smp_planner.h"
#include "smp_route.h"

using namespace smp;

namespace {

// Rounds per batch.  A batch that overshoots the fixed point pays an empty launch per round too many, one that falls
// short a host round trip; DESIGN.md 8g has the measurement, made on variant builds (make EXTRA=-DSMP_FIELD_BATCH=8).
#ifndef SMP_FIELD_BATCH
#define SMP_FIELD_BATCH 16
#endif
constexpr int FIELD_BATCH = SMP_FIELD_BATCH;
static_assert(FIELD_BATCH >= 1 && FIELD_BATCH <= 1024, "rounds per batch");

double ms_since(std::chrono::steady_clock::time_point t) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}

// A reservation that fails for want of memory is the call's SMP_ERR_CAPACITY.
#define RESERVE(buf, n)                                   \
  do {                                                    \
    const hipError_t re_ = (buf).reserve(n);               \
    if (re_ == hipErrorOutOfMemory) {                     \
      (void)hipGetLastError();                            \
      return SMP_ERR_CAPACITY;                            \
    }                                                     \
    HIPCHK(re_);                                          \
  } while (0)

// The field from node src on the device, left in p->d_fcost; then the small kernels: the record for node `to` (to < 0:
// none), the parents when asked for or needed, the chain src -> to when to >= 0.  *stats is the downloaded record.
int field_run(smp_planner* p, const RouteLattice& L, const FieldGrid& g, int64_t src, int64_t to, bool want_parents,
              smp_field_info* I, FieldStats* stats) {
  HIPCHK(hipSetDevice(p->device));
  const int64_t n_nodes = L.d.n, n_words = (n_nodes + 31) / 32, n_tiles = field_n_tiles(g);
  int64_t n_free = 0;
  for (int64_t i = 0; i < n_words; ++i) n_free += __builtin_popcount(L.bits[i]);
  constexpr int batch = FIELD_BATCH;
  RESERVE(p->d_fbits, (size_t)n_words);
  RESERVE(p->d_fcost, (size_t)n_nodes);
  RESERVE(p->d_factive, (size_t)(2 * n_tiles));
  RESERVE(p->d_fchanged, (size_t)FIELD_BATCH);
  RESERVE(p->d_fstats, 1);
  if (want_parents || to >= 0) RESERVE(p->d_fparent, (size_t)n_nodes);
  if (to >= 0) RESERVE(p->d_fchain, (size_t)n_nodes);
  HIPCHK(hipMemcpyAsync(p->d_fbits.p, L.bits, (size_t)n_words * sizeof(uint32_t), hipMemcpyHostToDevice, p->stream));
  launch_field_init(p->stream, g, src, p->d_fcost.p, p->d_factive.p, p->d_fstats.p);
  HIPCHK(hipGetLastError());
  const int64_t cap = field_round_cap(n_free);
  int64_t rounds_run = 0;
  bool done = false;
  unsigned h_changed[FIELD_BATCH];
  while (!done) {
    if (rounds_run >= cap) {
      fprintf(stderr, "smp_gpu: the cost field did not settle in %lld rounds\n", (long long)cap);
      (void)hipStreamSynchronize(p->stream);
      return SMP_ERR_HIP;
    }
    HIPCHK(hipMemsetAsync(p->d_fchanged.p, 0, sizeof(unsigned) * batch, p->stream));
    HIPCHK(hipEventRecord(p->ev0, p->stream));
    for (int i = 0; i < batch; ++i)
      launch_field_round(p->stream, g, p->d_fbits.p, p->d_fcost.p, p->d_factive.p, (int)((rounds_run + i) & 1),
                         p->d_fchanged.p + i);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(p->ev1, p->stream));
    HIPCHK(hipMemcpyAsync(h_changed, p->d_fchanged.p, sizeof(unsigned) * batch, hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, p->ev0, p->ev1));
    I->kernel_ms += ms;
    I->launches += batch;
    for (int i = 0; i < batch && !done; ++i) {
      I->tile_runs += h_changed[i];
      if (h_changed[i] == 0) {
        I->rounds = (int)(rounds_run + i + 1);
        done = true;
      }
    }
    rounds_run += batch;
  }
  HIPCHK(hipEventRecord(p->ev0, p->stream));
  launch_field_stats(p->stream, g, p->d_fcost.p, to, p->d_fstats.p);
  if (want_parents || to >= 0) launch_field_parents(p->stream, g, p->d_fbits.p, p->d_fcost.p, p->d_fparent.p);
  if (to >= 0) launch_field_chain(p->stream, g, p->d_fparent.p, src, to, p->d_fchain.p, p->d_fstats.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(p->ev1, p->stream));
  HIPCHK(hipMemcpyAsync(stats, p->d_fstats.p, sizeof(FieldStats), hipMemcpyDeviceToHost, p->stream));
  HIPCHK(hipStreamSynchronize(p->stream));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, p->ev0, p->ev1));
  I->kernel_ms += ms;
  I->n_reached = (int64_t)stats->n_reached;
  return SMP_OK;
}

double max_cost(const FieldStats& s) {
  double v;
  std::memcpy(&v, &s.max_bits, sizeof(v));
  return v;
}

}  // namespace

extern "C" void smp_field_tile_shape(int tile[3]) {
  if (!tile) return;
  tile[0] = FIELD_BX;
  tile[1] = FIELD_BY;
  tile[2] = FIELD_BT;
}

extern "C" int smp_base_cost_field(smp_planner* p, const smp_base_lattice* lat, const uint32_t* free_bits,
                                   const int32_t source[3], double* cost, int32_t* parent, smp_field_info* info) {
  const auto t_begin = std::chrono::steady_clock::now();
  smp_field_info I;
  std::memset(&I, 0, sizeof(I));
  if (info) *info = I;
  if (!p || !lat || !free_bits || !source) return SMP_ERR_ARG;
  RouteLattice L;
  if (int st = route_lattice(lat, free_bits, &L)) return st;
  if (source[0] < 0 || source[0] >= L.nx || source[1] < 0 || source[1] >= L.ny || source[2] < 0 || source[2] >= L.nt ||
      !L.free_at(source[0], source[1], source[2]))
    return SMP_ERR_ARG;
  if (int b_ = busy_check(p)) return b_;
  const FieldGrid g = field_grid(L);
  const int64_t src = L.node(source[0], source[1], source[2]);
  I.n_nodes = L.d.n;
  FieldStats stats;
  int st = field_run(p, L, g, src, -1, parent != nullptr, &I, &stats);
  if (st == SMP_OK && !field_unique(max_cost(stats), g)) {
    // the least weight no longer moves the largest cost: the host search's order decides, so the host search answers
    std::vector<double> dp;
    std::vector<int32_t> par;
    int64_t n_settled = 0;
    route_search(L, src, -1, &dp, &par, &n_settled);
    if (cost) std::memcpy(cost, dp.data(), sizeof(double) * (size_t)L.d.n);
    if (parent) std::memcpy(parent, par.data(), sizeof(int32_t) * (size_t)L.d.n);
    I.n_reached = n_settled;
    I.fell_back = 1;
  } else if (st == SMP_OK) {
    if (cost && hipMemcpy(cost, p->d_fcost.p, sizeof(double) * (size_t)L.d.n, hipMemcpyDeviceToHost) != hipSuccess)
      st = SMP_ERR_HIP;
    if (st == SMP_OK && parent &&
        hipMemcpy(parent, p->d_fparent.p, sizeof(int32_t) * (size_t)L.d.n, hipMemcpyDeviceToHost) != hipSuccess)
      st = SMP_ERR_HIP;
  }
  p->last_check_ms = I.kernel_ms;
  I.total_ms = ms_since(t_begin);
  if (info) *info = I;
  return st;
}

extern "C" int smp_base_route_gpu(smp_planner* p, const smp_base_lattice* lat, const uint32_t* free_bits,
                                  const double from[3], const double to[3], int snap_cells, double** out_rows,
                                  int64_t* n_out, int32_t** out_chain, smp_route_info* info, smp_field_info* finfo) {
  const auto t_begin = std::chrono::steady_clock::now();
  if (out_rows) *out_rows = nullptr;
  if (n_out) *n_out = 0;
  if (out_chain) *out_chain = nullptr;
  smp_route_info r;
  std::memset(&r, 0, sizeof(r));
  for (int k = 0; k < 3; ++k) r.from_node[k] = r.to_node[k] = -1;
  if (info) *info = r;
  smp_field_info I;
  std::memset(&I, 0, sizeof(I));
  if (finfo) *finfo = I;
  if (!p || !lat || !free_bits || !from || !to || !out_rows || !n_out) return SMP_ERR_ARG;
  RouteLattice L;
  if (int st = route_lattice(lat, free_bits, &L)) return st;
  if (int st = route_ends(L, from, to, snap_cells, &r)) {
    if (info) *info = r;
    return st;
  }
  if (info) *info = r;
  if (int b_ = busy_check(p)) return b_;
  const FieldGrid g = field_grid(L);
  const int64_t src = L.node(r.from_node[0], r.from_node[1], r.from_node[2]);
  const int64_t dst = L.node(r.to_node[0], r.to_node[1], r.to_node[2]);
  I.n_nodes = L.d.n;
  FieldStats stats;
  int st = field_run(p, L, g, src, dst, false, &I, &stats);
  auto leave = [&](int rc) {
    p->last_check_ms = I.kernel_ms;
    I.total_ms = ms_since(t_begin);
    if (finfo) *finfo = I;
    if (info) *info = r;
    return rc;
  };
  if (st != SMP_OK) return leave(st);
  if (!field_unique(max_cost(stats), g)) {
    I.fell_back = 1;
    const int rc = smp_base_route(lat, free_bits, from, to, snap_cells, out_rows, n_out, out_chain, &r);
    return leave(rc);
  }
  r.n_settled = (int64_t)stats.n_settled;
  if (stats.n_chain < 0) return leave(SMP_ERR_HIP);
  if (stats.n_chain == 0) return leave(SMP_ERR_NO_SOLUTION);
  std::vector<int32_t> nodes((size_t)stats.n_chain);
  if (hipMemcpy(nodes.data(), p->d_fchain.p, sizeof(int32_t) * nodes.size(), hipMemcpyDeviceToHost) != hipSuccess)
    return leave(SMP_ERR_HIP);
  r.cost = stats.cost_to;
  r.n_chain = stats.n_chain;
  const int64_t layer = (int64_t)L.nx * L.ny;
  std::vector<int32_t> chain;
  chain.reserve(nodes.size() * 3);
  for (size_t i = nodes.size(); i-- > 0;) {  // (walked goal first)
    const int64_t v = nodes[i];
    const int t = (int)(v / layer);
    chain.push_back((int32_t)(v % L.nx));
    chain.push_back((int32_t)((v - (int64_t)t * layer) / L.nx));
    chain.push_back(t);
  }
  return leave(route_output(L, chain, out_rows, n_out, out_chain));
}
