// What smp_kernels.hip offers the host files (smp_api*.cpp): its kernels, their launchers, the smp_debug_* readers of
// the debugging builds, and the source-site word of trace and bounds records.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "smp_plan.h"
#include "smp_types.h"

namespace smp {

// A source site of smp_kernels.hip or of one of the smp_plan_*.h headers it includes, in one word: file << SITE_LINE_BITS
// | line, the file's number being the place of its name in SITE_FILES.  SMP_SITE forms the word of the line it stands on
// and fails to compile in a file that is not listed or past the line field's range.  The trace log (SMP_TRACE) and
// smp_debug_bounds (SMP_BOUNDS) carry such words; tools/trace_probe.py reads SITE_FILES from here.
constexpr int SITE_LINE_BITS = 13, SITE_FILE_BITS = 5;
constexpr int SITE_FILE_BARRIERS = (1 << SITE_FILE_BITS) - 1;  // trace log: the line field is a barrier count
constexpr const char* SITE_FILES[] = {"smp_kernels.hip", "smp_plan_prof.h", "smp_plan_ringcheck.h", "smp_plan_preverify.h"};
constexpr int SITE_NFILES = sizeof(SITE_FILES) / sizeof(SITE_FILES[0]);
static_assert(SITE_NFILES <= SITE_FILE_BARRIERS, "file numbers of a site word");
constexpr int site_file_id(const char* path) {  // the place of path's last component in SITE_FILES, -1 = not listed
  const char* base = path;
  for (const char* p = path; *p; ++p)
    if (*p == '/') base = p + 1;
  for (int f = 0; f < SITE_NFILES; ++f) {
    const char *a = SITE_FILES[f], *b = base;
    while (*a && *a == *b) { ++a; ++b; }
    if (*a == *b) return f;
  }
  return -1;
}
template <int FILE, int LINE>
constexpr int site_word() {
  static_assert(FILE >= 0, "SMP_SITE in a file that SITE_FILES does not list");
  static_assert(LINE < (1 << SITE_LINE_BITS), "SMP_SITE past the line field of a site word");
  return FILE << SITE_LINE_BITS | LINE;
}
#define SMP_SITE (smp::site_word<smp::site_file_id(__FILE__), __LINE__>())
inline const char* site_file(int site) {
  const int f = site >> SITE_LINE_BITS;
  return f >= 0 && f < SITE_NFILES ? SITE_FILES[f] : "?";
}
inline int site_line(int site) { return site & ((1 << SITE_LINE_BITS) - 1); }

// batch check, collision listing
size_t check_kernels_private_bytes();
void launch_check(int ct, int grid, hipStream_t st, const RobotDev* rb, SceneDev sc, const MapCfg* mc, const double* q,
                  long long n, int self, int map, uint8_t* valid, unsigned long long* prof);
void launch_collisions(hipStream_t st, const RobotDev* rb, SceneDev sc, const MapCfg* mc, const double* q, int map,
                       uint8_t* link_map, uint8_t* pair_self);
// planner and paths
__global__ void plan_kernel(const RobotDev* rb, SceneDev sc, const MapCfg* mc, QueryDev* qs, int nq, int scout_base,
                            int helper_base, int iters);
__global__ void boards_reset_kernel(const QueryDev* qs, int ns);
__global__ void path_kernel(QueryDev* qs, int* counts);
__global__ void path_edges_kernel(const QueryDev* qs, int q, int ns, int ng, double* out);
// parity and near probes
__global__ void sincos_kernel(const double* x, int n, double* s, double* c);
__global__ void u01_kernel(unsigned long long seed, unsigned query, const uint32_t* ctr, int n, double* out);
__global__ void fk_kernel(const RobotDev* rb, const double* q, int n, double* frames, double* eez);
__global__ void sqrt_div_kernel(const double* a, const double* b, int n, double* sq, double* dv);
__global__ void near_probe_kernel(const double* tq, const double* tcost, int cap, int n, const double* queries,
                                  const int* excl, int m, double r, int reps, int* nn, int* nk, int* lo, int* hi,
                                  unsigned long long* ticks, const float* tqf);
__global__ void near_probe_inl_kernel(const double* tq, const double* tcost, int cap, int n, const double* queries,
                                      const int* excl, int m, double r, int reps, int* nn, int* nk, int* lo, int* hi,
                                      unsigned long long* ticks, const float* tqf);

}  // namespace smp

// Readers of the debugging builds' device records; each returns nonzero in a build without its switch.
extern "C" int smp_debug_tlog(unsigned long long* out, int cap, int reset);   // SMP_TRACE
extern "C" int smp_debug_scanprof(unsigned long long* out, int reset);        // SMP_SCAN_PROF
extern "C" int smp_debug_preverify(unsigned long long* out, int reset);       // SMP_PRE_VERIFY
extern "C" int smp_debug_bounds(int* out);                                    // SMP_BOUNDS: out[0] a site word
#ifdef SMP_RING_CHECK
extern "C" void smp_ringchk_dump();
#endif
