// The planner's measuring and checking code: trace log, phase clocks, the profiling variants' clocks and counters, the
// bounds check.  Nothing here plans: every macro is empty (or a plain clock read) in the product build.
// Relies on g_L (the planner's LDS object) and smp_kernels.h (the source-site word).
// Included by smp_kernels.hip only, once, behind its LDS layouts (which hold no barrier) and ahead of the planner's
// first function, so that a trace build counts every barrier of the planner.
#pragma once

namespace smp {

// ------------------------------------------------------------------------------------- profiling slots
// QState::prof[32], thread 0 of a workgroup.  Slots 0..19 are the phase clocks and counters of every build (the leader's;
// a scout keeps its own QState copy and clocks its pass stages 0..6 into the same numbers, SC_PHASE).
enum { P_SAMPLE, P_NN, P_EXPAND, P_NEAR, P_CHOOSE, P_REWIRE, P_CONNECT, P_TILES, P_NTILES, P_COSTS, P_VIA, P_NVIA,
       P_TFK, P_TCHAIN, P_TCENTRE, P_TTEST, P_XEXPAND, P_XCHOOSE, P_XREWIRE, P_XCONNECT };
// Slots 20..31 by owner.  tools/perf_probe.py, slice_probe.py and near_probe.py read them by number.
//   slot   leader, product build     leader, one variant at a time                       scout (every build)
//   20-24  -                         SMP_NEAR_PROF: near_set's steps 1..5                -
//   25     -                         -                                                   -
//   26     -                         SMP_NEAR_PROF: calls that left the register path    passes redone on newer sizes
//   27     -                         SMP_NEAR_PROF: calls finished                       -
//   28     pre_commit: committed     DETAIL rewire commit  | VIA wave 0's steps | WAIT nn + expand | JOB pickup ticks   idle ticks
//   29     pre_commit: no record     DETAIL cost_update    | VIA norms and sums | WAIT near + choose | JOB pickups      publish ticks
//   30     pre_commit: newer nearest DETAIL connect replay | VIA costs, state   | WAIT rewire | JOB tile-finish ticks   passes
//   31     pre_commit: connect redone DETAIL insert_via    | VIA batches x 100  | WAIT connect | -                      busy ticks
// A collision job that times out (status -5) overwrites 28, 29 and 31 with its tiles left, its tiles and its number, in
// every build.  SMP_RING_CHECK counts in 28..30 (bad samples, first bad iteration + 1, checks) on top of pre_commit's
// counters, which it does not switch off.  The near probe kernel hands &prof[20] to slice_near_hist (its pf[0..9]).
enum {
  P_NEAR_STEP = 20, P_NEAR_STREAM = 26, P_NEAR_DONE = 27, P_PROBE = 20,
  P_SC_REDONE = 26, P_SC_IDLE = 28, P_SC_PUBLISH = 29, P_SC_PASSES = 30, P_SC_BUSY = 31,
  P_PRE_COMMIT = 28,
  P_JOBTO_LEFT = 28, P_JOBTO_TILES = 29, P_JOBTO_SEQ = 31,
  P_DET_REWIRE = 28, P_DET_COSTUPD = 29, P_DET_CONNECT = 30, P_DET_INSVIA = 31,
  P_VIA_STEPS = 28, P_VIA_NORMS = 29, P_VIA_COSTS = 30, P_VIA_BATCHES = 31,
  P_WAIT_EXPAND = 28, P_WAIT_CHOOSE = 29, P_WAIT_REWIRE = 30, P_WAIT_CONNECT = 31,
  P_JOB_PICKUP = 28, P_JOB_PICKUPS = 29, P_JOB_FINISH = 30,
  P_RING_BAD = 28, P_RING_FIRST = 29, P_RING_CHECKS = 30,
};
// One variant owns the leader's slots 28..31.  SMP_PROF_TAIL_CLAIMED: pre_commit's outcome counters are off (also under
// SMP_NEAR_PROF, whose build has always kept them off).
#if defined(SMP_DETAIL_PROF) + defined(SMP_VIA_PROF) + defined(SMP_WAIT_PROF) + defined(SMP_JOB_PROF) + \
    defined(SMP_RING_CHECK) > 1
#error "profiling slots 28..31: at most one of SMP_DETAIL_PROF, SMP_VIA_PROF, SMP_WAIT_PROF, SMP_JOB_PROF, SMP_RING_CHECK"
#endif
#if defined(SMP_DETAIL_PROF) || defined(SMP_VIA_PROF) || defined(SMP_WAIT_PROF) || defined(SMP_JOB_PROF) || \
    defined(SMP_NEAR_PROF)
#define SMP_PROF_TAIL_CLAIMED
#endif
// Outcome counters of pre_commit (committed / no usable record / a newer nearest node / connect completed by
// connect_graphs).
#ifdef SMP_PROF_TAIL_CLAIMED
#define PRE_COUNT(k)
#else
#define PRE_COUNT(k) if (threadIdx.x == 0) g_L.S.prof[P_PRE_COMMIT + (k)]++
#endif

// ------------------------------------------------------------------------------------- trace log
// SMP_TRACE builds (tools/trace_probe.py): thread 0 of the leader and of the scouts appends (role, source site, device
// clock) records for the iterations [SMP_TRACE_IT0, SMP_TRACE_IT1) of query 0; smp_debug_tlog reads them.  A record:
// role << 62 | (iteration - IT0) << 54 | site << 36 | clock (36 bits: 11 minutes of the 100 MHz wall clock), the site
// as smp_kernels.h forms it (file << SITE_LINE_BITS | line).
#ifdef SMP_TRACE
#ifndef SMP_TRACE_IT0
#define SMP_TRACE_IT0 3000
#endif
#ifndef SMP_TRACE_IT1
#define SMP_TRACE_IT1 3040
#endif
constexpr unsigned TLOG_CAP = 1u << 18, TLOG_ROLE = TLOG_CAP / 4;  // records per role (0 leader, 1-2 scouts)
__device__ unsigned long long g_tlog[TLOG_CAP];
__device__ unsigned g_tlog_n[4];
constexpr int TR_CLOCK_BITS = 36;
static_assert(TR_CLOCK_BITS + SITE_LINE_BITS + SITE_FILE_BITS == 54, "a record's site and clock fill the bits below the iteration");
static_assert(SMP_TRACE_IT1 - SMP_TRACE_IT0 <= 256, "a record's iteration field has 8 bits");
// No atomics: each workgroup keeps its role's record count in LDS (loaded at launch start by tlog_begin) and
// stores it back after every record (plain stores, nothing waited on), so tracing adds ~0.1 us per record.
#define TR_RECORD(site)                                                                                       \
  if (threadIdx.x == 0 && g_L.tit >= SMP_TRACE_IT0 && g_L.tit < SMP_TRACE_IT1 && g_L.tn < TLOG_ROLE) {        \
    g_tlog[g_L.trole * TLOG_ROLE + g_L.tn] =                                                                   \
        ((unsigned long long)g_L.trole << 62) | ((unsigned long long)((g_L.tit - SMP_TRACE_IT0) & 0xff) << 54) | \
        ((unsigned long long)(site) << TR_CLOCK_BITS) | (wall_clock64() & ((1ull << TR_CLOCK_BITS) - 1));     \
    g_tlog_n[g_L.trole] = ++g_L.tn;                                                                            \
  }
#define TR() TR_RECORD(SMP_SITE)
// The barriers of a leader iteration, counted by thread 0 (every __syncthreads() below this line) and logged at the
// iteration's end as a record of the file SITE_FILE_BARRIERS whose line field is the count (trace_probe.py prints them
// apart).
constexpr int TR_BAR_MAX = 383;
static_assert(TR_BAR_MAX < (1 << SITE_LINE_BITS), "the barrier count lies in a record's line field");
#define __syncthreads()                 \
  do {                                  \
    if (threadIdx.x == 0) ++g_L.tbar;   \
    __syncthreads();                    \
  } while (0)
#define TR_BARRIERS() TR_RECORD(SITE_FILE_BARRIERS << SITE_LINE_BITS | min(g_L.tbar, TR_BAR_MAX))
// thread 0: the iteration (pass) the following records belong to; a workgroup's role at launch start
#define TR_ITERATION() if (threadIdx.x == 0) { g_L.tit = g_L.S.iter; g_L.tbar = 0; }
#define TR_PASS(it) if (threadIdx.x == 0) g_L.tit = it
#define TR_ROLE(role, it0, slot) g_L.trole = role; g_L.tit = it0; g_L.tn = g_tlog_n[slot]
#else
#define TR()
#define TR_BARRIERS()
#define TR_ITERATION()
#define TR_PASS(it)
#define TR_ROLE(role, it0, slot)
#endif

// ------------------------------------------------------------------------------------- phase clocks
// Thread 0, device wall clock (s_memrealtime ticks): where an iteration spends its time.
#define PROF_BEGIN() unsigned long long _pt = threadIdx.x == 0 ? wall_clock64() : 0
#define PROF_END(k) if (threadIdx.x == 0) { g_L.S.prof[k] += wall_clock64() - _pt; }

// SMP_DETAIL_PROF: thread-0 clocks of serial sections into prof[28..31] (perf_probe.py SMP_DETAIL_PROF=1)
#ifdef SMP_DETAIL_PROF
#define DETAIL_BEGIN(v) const unsigned long long v = threadIdx.x == 0 ? wall_clock64() : 0
#define DETAIL_END(v, k) if (threadIdx.x == 0) g_L.S.prof[k] += wall_clock64() - v
#else
#define DETAIL_BEGIN(v)
#define DETAIL_END(v, k)
#endif

// SMP_NEAR_PROF: near_set's clocks of the barrier-separated steps into prof[20..24]; path counts in prof[26], prof[27].
// A trace build logs the steps instead.
#ifdef SMP_NEAR_PROF
#define NEAR_CLOCK_BEGIN() unsigned long long _tn = 0
#define NEAR_CLOCK(k)                                                                    \
  if (threadIdx.x == 0) {                                                                \
    const unsigned long long _t = wall_clock64();                                        \
    if (k > 0) g_L.S.prof[P_NEAR_STEP - 1 + k] += _t - _tn;                              \
    _tn = _t;                                                                            \
  }
#define NEAR_COUNT(k) if (threadIdx.x == 0) g_L.S.prof[k]++
#elif defined(SMP_TRACE)
#define NEAR_CLOCK_BEGIN()
#define NEAR_CLOCK(k) TR()
#define NEAR_COUNT(k)
#else
#define NEAR_CLOCK_BEGIN()
#define NEAR_CLOCK(k)
#define NEAR_COUNT(k)
#endif

// SMP_VIA_PROF: thread-0 clocks of the leader's via chains.  via_chain: wave 0's steps to the barrier into prof[28],
// batches (x 100) into prof[31]; via_costs: norms and sums to the barrier into prof[29], costs and state to the barrier
// into prof[30].
#ifdef SMP_VIA_PROF
#define VIA_BATCH_BEGIN() const unsigned long long _v0 = threadIdx.x == 0 ? wall_clock64() : 0
#define VIA_BATCH_STEPPED() \
  if (threadIdx.x == 0) { g_L.S.prof[P_VIA_STEPS] += wall_clock64() - _v0; g_L.S.prof[P_VIA_BATCHES] += 100; }
#define VIA_CLK_BEGIN() unsigned long long _v0 = threadIdx.x == 0 ? wall_clock64() : 0
#define VIA_CLK(k) if (threadIdx.x == 0) { const unsigned long long _v1 = wall_clock64(); g_L.S.prof[k] += _v1 - _v0; _v0 = _v1; }
#else
#define VIA_BATCH_BEGIN()
#define VIA_BATCH_STEPPED()
#define VIA_CLK_BEGIN()
#define VIA_CLK(k)
#endif

// SMP_WAIT_PROF: the leader's waits for a record stage (spec_stage, since t0) into prof[28..31] by stage: nn / expand,
// near / choose, rewire, connect.
#ifdef SMP_WAIT_PROF
#define WAIT_CLOCK(s, t0)  \
  if (threadIdx.x == 0)    \
    g_L.S.prof[s <= SC_EXPAND ? P_WAIT_EXPAND : s <= SC_CHOOSE ? P_WAIT_CHOOSE : s == SC_DONE ? P_WAIT_REWIRE : P_WAIT_CONNECT] += wall_clock64() - t0
#else
#define WAIT_CLOCK(s, t0)
#endif

// SMP_JOB_PROF (tools/perf_probe.py with SMP_JOB_PROF=1): a job's way through the helpers, summed in JobBoard::dbg --
// [0] the publication's clock, [1] / [2] pickup delays and their count, [3] tile-finish delays, [4..7] the tile stage
// clocks (JobLds::tprof) -- and added to the leader's prof[28..30] and prof[P_TFK ..] when its launch ends.
#ifdef SMP_JOB_PROF
#define JOBPROF_PUBLISHED(jb) if (threadIdx.x == 0) st_agent(&jb->dbg[0], wall_clock64())
#define JOBPROF_TILE_CLOCKS(J, tp)                                      \
  if (threadIdx.x == 0) for (int i = 0; i < 4; ++i) J.tprof[i] = 0;     \
  unsigned long long* tp = J.tprof
#define JOBPROF_PICKUP(jb, w, nt)                                       \
  if (threadIdx.x == 0 && w - 1 < nt) {                                 \
    const unsigned long long tpk = ld_agent(&jb->dbg[0]);               \
    atomicAdd(&jb->dbg[1], wall_clock64() - tpk);                       \
    atomicAdd(&jb->dbg[2], 1ull);                                       \
  }
#define JOBPROF_TILE_DONE(jb) if (threadIdx.x == 0) atomicAdd(&jb->dbg[3], wall_clock64() - ld_agent(&jb->dbg[0]))
#define JOBPROF_TILES_OUT(jb, J, w, nt) \
  if (threadIdx.x == 0 && w - 1 < nt) for (int i = 0; i < 4; ++i) atomicAdd(&jb->dbg[4 + i], J.tprof[i])
#define JOBPROF_COLLECT(C)                                                                                          \
  if (C.Q.jb) {                                                                                                     \
    g_L.S.prof[P_JOB_PICKUP] += ld_agent(&C.Q.jb->dbg[1]);                                                          \
    g_L.S.prof[P_JOB_PICKUPS] += ld_agent(&C.Q.jb->dbg[2]);                                                         \
    g_L.S.prof[P_JOB_FINISH] += ld_agent(&C.Q.jb->dbg[3]);                                                          \
    for (int i = 0; i < 4; ++i) g_L.S.prof[P_TFK + i] += ld_agent(&C.Q.jb->dbg[4 + i]); /* helper tile stages */    \
  }
#else
#define JOBPROF_PUBLISHED(jb)
#define JOBPROF_TILE_CLOCKS(J, tp) unsigned long long* tp = nullptr
#define JOBPROF_PICKUP(jb, w, nt)
#define JOBPROF_TILE_DONE(jb)
#define JOBPROF_TILES_OUT(jb, J, w, nt)
#define JOBPROF_COLLECT(C)
#endif

// SMP_SCAN_PROF builds (tools/scan_probe.py): clocks of the distributed scans, summed over every scan of the leader and
// the scouts, read by smp_debug_scanprof: [0] scans, [1] write-back + publication, [2] own slice, [3] collection,
// [4] merge, [5] stolen slices, [6] collection rounds, [7] helper slices, [8] helper pickup (publication -> acquire),
// [9] helper acquire, [10] helper slice, [11] publication -> helper result stored, [12] near scans, [13] their
// collection, [14] participants, [15] nodes, [16] near scans' own slice, [17] near merge, [18] near helper slices,
// [19] their slice clocks.  JobBoard::dbg[8] carries the publication's clock to the helpers.
#ifdef SMP_SCAN_PROF
__device__ unsigned long long g_scanprof[24];
#define SCANPROF_ADD(k, v) atomicAdd(&g_scanprof[k], (unsigned long long)(v))
#define SCANPROF_CLOCK(v) const unsigned long long v = wall_clock64()
#define SCANPROF_COUNTERS(a, b) int a = 0, b = 0
#define SCANPROF_INC(v) ++v
// scan_helper: before its acquire hp0, after it hp1, now = the slice done
#define SCANPROF_HELPER(C, near, hp0, hp1)                                                                       \
  if (threadIdx.x == 0) {                                                                                        \
    const unsigned long long hp2 = wall_clock64(), pub = ld_agent(&C.Q.jb->dbg[8]);                              \
    SCANPROF_ADD(7, 1); SCANPROF_ADD(8, hp0 - pub); SCANPROF_ADD(9, hp1 - hp0); SCANPROF_ADD(10, hp2 - hp1);     \
    SCANPROF_ADD(11, hp2 - pub);                                                                                 \
    if (near) { SCANPROF_ADD(18, 1); SCANPROF_ADD(19, hp2 - hp1); }                                              \
  }
// scan_run: entry sp0, publication sp1 (handed to the helpers), own slice done sp2, now = collection done
#define SCANPROF_PUBLISHED(C, sp1) if (threadIdx.x == 0) st_agent(&C.Q.jb->dbg[8], sp1)
#define SCANPROF_RUN(near, P, nodes, sp0, sp1, sp2, steals, rounds)                                              \
  if (threadIdx.x == 0) {                                                                                        \
    const unsigned long long sp3 = wall_clock64();                                                               \
    SCANPROF_ADD(0, 1); SCANPROF_ADD(1, sp1 - sp0); SCANPROF_ADD(2, sp2 - sp1); SCANPROF_ADD(3, sp3 - sp2);      \
    SCANPROF_ADD(5, steals); SCANPROF_ADD(6, rounds); SCANPROF_ADD(14, P); SCANPROF_ADD(15, nodes);              \
    if (near) { SCANPROF_ADD(12, 1); SCANPROF_ADD(13, sp3 - sp2); SCANPROF_ADD(16, sp2 - sp1); }                 \
    g_L.spc_t = sp3;                                                                                             \
  }
// the merge after a scan's collection: nearest_dist, near_set_dist
#define SCANPROF_MERGED() if (threadIdx.x == 0) SCANPROF_ADD(4, wall_clock64() - g_L.spc_t)
#define SCANPROF_NEAR_MERGED() \
  if (threadIdx.x == 0) { SCANPROF_ADD(4, wall_clock64() - g_L.spc_t); SCANPROF_ADD(17, wall_clock64() - g_L.spc_t); }
#else
#define SCANPROF_ADD(k, v)
#define SCANPROF_CLOCK(v)
#define SCANPROF_COUNTERS(a, b)
#define SCANPROF_INC(v)
#define SCANPROF_HELPER(C, near, hp0, hp1)
#define SCANPROF_PUBLISHED(C, sp1)
#define SCANPROF_RUN(near, P, nodes, sp0, sp1, sp2, steals, rounds)
#define SCANPROF_MERGED()
#define SCANPROF_NEAR_MERGED()
#endif

// SMP_CONN_PROF (tools/perf_probe.py with SMP_CONN_PROF=1): the scout's counts and thread-0 clocks of PlanLds::cprof
// (the words are listed there), stored to ScoutBoard::cprof two per word when the scout leaves.
#ifdef SMP_CONN_PROF
#define CONNPROF_CLOCK(v) const unsigned long long v = threadIdx.x == 0 ? wall_clock64() : 0
#define CONNPROF_RESET() for (int k = 0; k < 12; ++k) g_L.cprof[k] = 0
#define CONNPROF_STORE(C) \
  for (int k = 0; k < 6; ++k) st_agent(&C.Q.scb->cprof[k], (unsigned long long)g_L.cprof[2 * k] | (unsigned long long)g_L.cprof[2 * k + 1] << 32)
// conn_window (thread 0): rewire jobs with a connect record to follow, those that find cgo there
#define CONNPROF_WINDOW(C)                  \
  g_L.cprof[0] += g_L.two_scouts != 0;      \
  g_L.cprof[1] += g_L.two_scouts && (unsigned)(ld_agent(&C.Q.scb->cgo) >> 32) == (unsigned)(g_L.sc_k + 1)
// scout_iteration: the second near set since n0; the expand and rewire stages' edge_validity since e0 / r0
#define CONNPROF_NEAR2(n0) if (threadIdx.x == 0) { g_L.cprof[2]++; g_L.cprof[3] += (unsigned)(wall_clock64() - n0); }
#define CONNPROF_EXPAND(e0, opt) if (threadIdx.x == 0 && opt) { g_L.cprof[10] += (unsigned)(wall_clock64() - e0); g_L.cprof[11]++; }
#define CONNPROF_REWIRE(r0) if (threadIdx.x == 0) { g_L.cprof[8] += (unsigned)(wall_clock64() - r0); g_L.cprof[9]++; }
// scout_connect that sent a record: entry c0, cgo seen c1, scan done c2
#define CONNPROF_CONNECT(c0, c1, c2)                                                                                            \
  if (threadIdx.x == 0) {                                                                                                       \
    g_L.cprof[4]++;                                                                                                             \
    g_L.cprof[5] += (unsigned)(wall_clock64() - c0); g_L.cprof[6] += (unsigned)(c1 - c0); g_L.cprof[7] += (unsigned)(c2 - c1);  \
  }
#else
#define CONNPROF_CLOCK(v)
#define CONNPROF_RESET()
#define CONNPROF_STORE(C)
#define CONNPROF_WINDOW(C)
#define CONNPROF_NEAR2(n0)
#define CONNPROF_EXPAND(e0, opt)
#define CONNPROF_REWIRE(r0)
#define CONNPROF_CONNECT(c0, c1, c2)
#endif

// ------------------------------------------------------------------------------------- bounds check
// SMP_BOUNDS builds (debugging): out-of-range node ids are recorded in g_dbg (first one: source site, id, block,
// tree) and replaced by 0 instead of being dereferenced; smp_debug_bounds() reads the record.
#ifdef SMP_BOUNDS
__device__ int g_dbg[8];
#define BCHK(id, lim, site, t)                                                                          \
  if ((unsigned)(id) >= (unsigned)(lim)) {                                                             \
    if (atomicCAS(&g_dbg[0], 0, (site)) == 0) { g_dbg[1] = (id); g_dbg[2] = blockIdx.x; g_dbg[3] = (t); g_dbg[4] = (lim); } \
    id = 0;                                                                                            \
  }
#else
#define BCHK(id, lim, site, t)
#endif

}  // namespace smp
