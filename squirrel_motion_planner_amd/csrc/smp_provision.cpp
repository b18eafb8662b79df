// Provisioning of a planning call (smp_provision.h): the environment knobs and the scouts / helpers rule.  No HIP.
#include "smp_provision.h"

#include <algorithm>
#include <cstdlib>

namespace smp {

PlanKnobs read_plan_knobs(int helpers, int nq) {
  PlanKnobs k;
  // SMP_HOST_PROF: microseconds from smp_plan entry to each host stage of the first launch (experiments)
  k.host_prof = std::getenv("SMP_HOST_PROF") != nullptr;
  k.debug = std::getenv("SMP_DEBUG") != nullptr;
  k.debug_scouts = std::getenv("SMP_DEBUG_SCOUTS") != nullptr;  // per-scout passes and XCD (experiments)
  k.bounds = std::getenv("SMP_BOUNDS") != nullptr;
  // configurations per job tile: by job size (smp_plan.h job_tile_ct); SMP_TILE_CT = 1 / 2 / 4 / 8 fixes it (experiments)
  k.tile_ct = 0;
  if (const char* e = std::getenv("SMP_TILE_CT")) {
    const int v = std::atoi(e);
    if (v == 1 || v == 2 || v == 4 || v == 8) k.tile_ct = v;
  }
  // scans of trees of at least this many nodes are split over the helpers (DESIGN.md "Scans of large trees");
  // SMP_SCAN_MIN overrides it (experiments and tests; 0: never)
  k.scan_min = 12288;
  if (const char* e = std::getenv("SMP_SCAN_MIN")) k.scan_min = std::max(0, std::atoi(e));
  // participants of one split scan: a nearest result is 3 granules, a near result 122 -- fewer, longer slices for
  // near: one per 2^scan_nshift nodes (4096), 8 to 32 (SMP_SCAN_PNN / SMP_SCAN_PNEAR cap them, SMP_SCAN_NSHIFT sets
  // the shift)
  k.scan_pnn = 64;
  k.scan_pnear = PROV_SCAN_PNEAR;
  if (const char* e = std::getenv("SMP_SCAN_PNN")) k.scan_pnn = std::atoi(e);
  if (const char* e = std::getenv("SMP_SCAN_PNEAR")) k.scan_pnear = std::atoi(e);
  k.scan_nshift = 12;
  if (const char* e = std::getenv("SMP_SCAN_NSHIFT")) k.scan_nshift = std::min(20, std::max(6, std::atoi(e)));
  k.scan_ps0 = 0;
  if (const char* e = std::getenv("SMP_SCAN_PS0")) k.scan_ps0 = std::min(4, std::max(0, std::atoi(e)));
  k.scan_pnn = std::min(PROV_SCAN_P, std::max(2, k.scan_pnn));
  k.scan_pnear = std::min(PROV_SCAN_PNEAR, std::max(2, k.scan_pnear));
  k.helper_cap = 200;  // SMP_HELPER_CAP: experiments with other helper caps
  if (const char* e = std::getenv("SMP_HELPER_CAP")) k.helper_cap = std::max(1, std::atoi(e));
  k.lead_div = 3;  // SMP_LEAD_DIV: the leader's share of the helpers (C2: 1/3 3.82, 1/5 3.75, 1/8 3.73 M configs/s)
  if (const char* e = std::getenv("SMP_LEAD_DIV")) k.lead_div = std::max(1, std::atoi(e));
  // SMP_PRE_HELPERS: helpers of each pre-solution-only scout (its jobs: expand + connect edge, 42 configurations).  12
  // (round 6; ct 4 tiles instead of 8): time to first path median 1.68 -> 1.61 ms over the 20 seeds on one box, C2 equal
  // (57.5 / 57.7 us per iteration); 16 1.61 ms but C2 69.0 against 68.4 us at 30000 iterations
  k.pre_helpers = 12;
  if (const char* e = std::getenv("SMP_PRE_HELPERS")) k.pre_helpers = std::max(0, std::atoi(e));
  // before the first solution a scout starts record k when the leader reaches k - pre_delay (DESIGN.md "Pre-solution
  // commits"); SMP_PRE_DELAY overrides it for experiments (0: at the request)
  k.pre_delay = 3;
  if (const char* e = std::getenv("SMP_PRE_DELAY")) k.pre_delay = std::atoi(e);
  k.early_ask = 0;  // SMP_EARLY_ASK=1: after the first solution, iteration k + 2 is asked for before k's rewires (DESIGN.md "Early asks")
  if (const char* e = std::getenv("SMP_EARLY_ASK")) k.early_ask = std::atoi(e);
  // SMP_PRE_REFRESH: a pre-solution scout rechecks its nearest on the leader's newer sizes after its expand job (bit 0)
  // and / or before it publishes (bit 1), starting the pass over (at most twice) when a newer node is nearer
  // (DESIGN.md "Pre-solution refresh"; bit 0 alone measured best)
  k.pre_refresh = 1;
  if (const char* e = std::getenv("SMP_PRE_REFRESH")) k.pre_refresh = std::atoi(e);
  k.conn_check = 0;  // SMP_CONN_CHECK=1: connect's edges checked by the scouts with their SC_CONN scans (experiments)
  if (const char* e = std::getenv("SMP_CONN_CHECK")) k.conn_check = std::atoi(e);
  k.pre_commit = 1;  // SMP_PRE_COMMIT=0: every iteration runs the full path (experiments)
  if (const char* e = std::getenv("SMP_PRE_COMMIT")) k.pre_commit = std::atoi(e);
  k.rebalance = helpers == 0 ? 1 : 0;  // SMP_REBALANCE=0: keep the first launch's provisioning (experiments)
  if (const char* e = std::getenv("SMP_REBALANCE")) k.rebalance = k.rebalance && std::atoi(e) != 0;
  // SMP_REBALANCE_DIV: a launch ends once 1/rb_div of its queries finished (C3, 64 queries: 2 / 4 / 8 all 10.1-10.3
  // M configs/s; C5, 8 queries: 0.49 / 0.61 / 0.62 M)
  // several queries run in time slices (SMP_SLICE_MS, default 50; 0: chunks of 256 .. 4096 iterations): a launch
  // ends at its slice or when a quarter of its queries finished, never waiting for the slowest query's chunk --
  // C5's queries differ 5x in iteration time (tools/batch_probe.py)
  k.slice_ms = 50.0;
  if (const char* e = std::getenv("SMP_SLICE_MS")) k.slice_ms = std::max(0.0, std::atof(e));
  k.rebalance_div = 4;
  if (const char* e = std::getenv("SMP_REBALANCE_DIV")) k.rebalance_div = std::max(1, std::atoi(e));
  k.xcd_margin = 1;
  if (const char* e = std::getenv("SMP_XCD_MARGIN")) k.xcd_margin = std::max(0, std::atoi(e));
  k.pre_scouts = 1;
  k.pre_lead_div = 5;  // SMP_PRE_LEAD_DIV: the leader's share of a pre-solution query's helpers (1 / n)
  if (const char* e = std::getenv("SMP_PRE_LEAD_DIV")) k.pre_lead_div = std::max(1, std::atoi(e));
  if (const char* e = std::getenv("SMP_PRE_SCOUTS")) k.pre_scouts = std::atoi(e);
  // a seconds budget bounds the host's wait for a launch at 4x the budget + this slack (SMP_WAIT_SLACK_S: tests)
  k.wait_slack_s = 60.0;
  if (const char* e = std::getenv("SMP_WAIT_SLACK_S")) k.wait_slack_s = std::atof(e);
  // a single query runs its whole budget in one launch (the loop state is resumable, but a relaunch costs the host
  // round trip, the board reset and the scouts' restart: C2, 5 launches of 256 .. 4096 iterations, ~1 ms each);
  // several queries start at 256 iterations and double, so that finished ones free their CUs early (rebalance)
  k.chunk0 = nq == 1 || k.slice_ms > 0 ? (1 << 30) : 256;
  if (const char* e = std::getenv("SMP_CHUNK0")) k.chunk0 = std::max(1, std::atoi(e));  // experiments
  // post-solution scout passes (DESIGN.md §5 "Round 13"): a tree_B of up to this many nodes is scanned for connect
  // under the pass's rewire job instead of after it (0: off).  The window's scan stays on the scout's workgroup at any
  // size, and a local scan grows with the tree while the job's window does not.  Measured: at C2's 3-4 k nodes the
  // scout's rewire stage 8.8 -> 9.7 us per pass and the iteration 49.2 -> 47.6 us; at 13.8 k nodes (20000 iterations)
  // the iteration 58.1 us with the gate at 2048, 56.4 at 8192 and 54.1 without a gate.  So 8192 is not the optimum at
  // those sizes: it is the largest size up to which the suite holds the window to the oracle (the 1e5- and 3e5-iteration
  // runs pass through it); above it parity was only probed, not tested, and far above scan_min a local scan outlasts
  // any job.
  k.scout_conn_ov_max = 8192;
  if (const char* e = std::getenv("SMP_SCOUT_CONN_OV_MAX")) k.scout_conn_ov_max = std::max(0, std::atoi(e));
  k.conn_prof = std::getenv("SMP_CONN_PROF") != nullptr;  // SMP_CONN_PROF builds: the scouts' connect clocks per launch
  return k;
}

// The nh helpers of a query with nsq scouts: h_lead for the leader, h_s[s] for scout s, one for the sampler.  After
// the first solution scouts 0 and 1 check choose-parent / rewire candidate batches (many tiles); scouts 2 and 3 only
// work before it, one edge per job (3 tiles); the leader's own jobs (edges no record had) are rare.
static void split(int nh, int ns_base, const PlanKnobs& k, int nsq, int& h_lead, int* h_s) {
  h_lead = 0;
  for (int s = 0; s < PROV_MAX_SCOUTS; ++s) h_s[s] = 0;
  if (nh < 1) return;  // (nh < 4 has no scouts: nothing to split)
  if (nsq > ns_base) {  // a query's pre-solution scouts: their records carry its iterations, one in four each
    const int avail = nh - 1;
    h_lead = avail / k.pre_lead_div;
    const int per = (avail - h_lead) / nsq;
    for (int s = 0; s < nsq; ++s) h_s[s] = per;
    h_s[0] += avail - h_lead - per * nsq;
  } else if (nsq > 0) {
    const int avail = nh - 1;  // minus the sampler
    h_lead = nsq >= 2 ? avail / k.lead_div : avail / 2;
    int rest = avail - h_lead;
    for (int s = 2; s < nsq; ++s) { h_s[s] = std::min(k.pre_helpers, rest); rest -= h_s[s]; }
    if (nsq >= 2) { h_s[0] = rest - rest / 2; h_s[1] = rest / 2; } else { h_s[0] = rest; }
  }
}

// Workgroups per query (one per CU): the leader, its scouts and the helpers (DESIGN.md "Helpers", "Scouts").
// Scouts: smp_params.scout of them (1: automatic -- 4 from 64 CUs per query (scouts 2 and 3 take every other
// iteration before the first solution and retire after it: time to first path 2.1 -> 1.7 ms on C2), 2 from 18,
// 1 from 6).  Helpers: the leader's tile helpers, each scout's, and the run-ahead sampler (the last one); up to 200
// with scouts (C2: 127 -> 200 helpers 3.65 -> 3.75 M configs/s with four scouts; 250 no longer all fit and stall).
// Every workgroup of a query (leader, scouts, helpers) polls the others, so all of them must be resident at once:
// the budget is the device's co-resident capacity for these kernels (occupancy x CUs), not a fixed count.  With
// automatic helpers the provisioning is redone for the queries still running whenever a launch ends with some of
// them finished (DESIGN.md "Many queries").
void provision(const ProvisionIn& in, const PlanKnobs& k, const char* have_sol, int n_act, Provision* out) {
  const int nh_req = in.helpers;
  const bool want_scout = in.scout != 0;
  const int slots = in.slots;
  const int cap_s = k.helper_cap;
  int nh = 0, ns = 0, ns_base = 0;
  const int na = std::max(1, n_act);
  const int cpq = std::max(1, slots / na);
  nh = nh_req;
  ns = 0;
  if (nh == 0) {
    if (want_scout) ns = cpq >= 64 ? 4 : cpq >= 18 ? 2 : cpq >= 6 ? 1 : 0;
    if (want_scout && in.scout > 1) ns = std::min(in.scout, PROV_MAX_SCOUTS);
    nh = want_scout ? std::min(cap_s, std::max(0, cpq - 1 - ns)) : std::min(63, std::max(0, cpq - 1));
  } else if (nh > 0 && want_scout) {
    ns = nh >= 16 ? 2 : nh >= 4 ? 1 : 0;
  }
  if (want_scout && in.scout > 1) ns = std::min(in.scout, PROV_MAX_SCOUTS);  // explicit count
  if (nh < 0) nh = 0;
  if (nh < 4) ns = 0;
  // per query: where the automatic count is two, a query still without a path takes four (scouts 2 and 3 take every
  // other pre-solution iteration and retire at the first path; C5 query 1 alone, 59 helpers: 25.5 -> 14.0 us per
  // iteration); ns is then the launch's largest count (grid, boards, XCD budget).  SMP_PRE_SCOUTS=0: uniform
  ns_base = ns;
  if (k.pre_scouts && nh_req == 0 && in.scout == 1 && ns == 2)
    for (int i = 0; i < n_act; ++i)
      if (!have_sol[i]) { ns = 4; break; }
  // per XCD: the workgroups of a launch are dealt round-robin over the 8 XCDs (blocks b and b + 8 share one), and a
  // workgroup dealt to a full XCD waits there -- a persistent helper that never starts leaves its tiles to the
  // leader's timeout on every job.  plan_kernel puts query q's leader and scouts on XCD slot q % 8, so the fullest
  // XCD holds (1 + ns) ceil(na / 8) of them; the helpers, dealt evenly, get what that XCD leaves, less
  // SMP_XCD_MARGIN CUs (default 1: the two launches race for the CUs).  C5, 8 queries rebalanced to 6 and 4:
  // 39 / 59 helpers each (some never resident) 0.65 M configs/s, 26 each 1.12 M.
  // (a device of one XCD has no such round-robin: no cap)
  const int nx = in.num_xcd;
  if (nx > 1 && in.num_cus >= nx) {
    const int per_xcd = in.num_cus / nx / std::max(1, in.slot_share);
    const int plan_max = (1 + ns) * ((na + nx - 1) / nx);
    const int free_xcd = std::max(0, per_xcd - plan_max - k.xcd_margin);
    const int hcap = nx * free_xcd / na;
    // (an explicit request beyond it gets no more than the automatic count either)
    if (nh > hcap) nh = std::max(0, nh_req > 0 ? std::min(hcap, cap_s) : hcap);
    // scouts need helpers of their own (and the boards' reset needs nh > 0): below four, none (as above)
    if (nh < 4) { ns = 0; ns_base = 0; }
  }
  // an explicit request larger than what can be resident is clamped to the automatic count: a helper that never
  // starts would leave its tiles to the leader's 8 us timeout on every job (helper sweeps: 250 helpers beside four
  // scouts no longer all start on 256 CUs and stall)
  if (1 + ns + nh > cpq) {
    nh = std::max(0, want_scout ? std::min(cap_s, cpq - 1 - ns) : std::min(63, cpq - 1));
    if (nh < 4) { ns = 0; ns_base = 0; nh = std::max(0, std::min(nh, cpq - 1)); }
  }
  out->nh = nh;
  out->ns = ns;
  out->ns_base = ns_base;
  out->q.resize(n_act);
  for (int i = 0; i < n_act; ++i) {
    const int nsq = ns > ns_base && have_sol[i] ? ns_base : ns;
    int h_lead = 0, h_s[PROV_MAX_SCOUTS];
    split(nh, ns_base, k, nsq, h_lead, h_s);
    QueryProvision& q = out->q[i];
    q.sampler = nh >= 2;              // with two or more helpers, the last one runs ahead sampling
    q.nworkers = nsq > 0 ? 1 + h_lead : (nh >= 2 ? nh : 1 + nh);
    q.nscouts = nsq;
    for (int s = 0; s < PROV_MAX_SCOUTS; ++s) q.sworkers_s[s] = s < ns ? 1 + h_s[s] : 1;
  }
}

}  // namespace smp
