// Provisioning of a planning call, free of HIP (plain C++17, built with the library and on its own by the CPU tests):
// the SMP_* environment knobs of the call read into one record, and the rule that decides how many scouts and helpers
// each query of a launch gets (DESIGN.md "Helpers", "Scouts", "Many queries").
#pragma once
#include <vector>

namespace smp {

// smp_plan.h's MAX_SCOUTS, SCAN_P and SCAN_PNEAR (that header needs a HIP compiler; smp_api_plan.cpp asserts that
// these agree with it)
constexpr int PROV_MAX_SCOUTS = 8;
constexpr int PROV_SCAN_P = 64;
constexpr int PROV_SCAN_PNEAR = 32;

// The SMP_* knobs of one smp_plan_batch call (experiments and tests).  read_plan_knobs reads the environment once per
// call; nothing else of the call does.
struct PlanKnobs {
  int tile_ct;      // SMP_TILE_CT: configurations per job tile fixed at 1 / 2 / 4 / 8 (0: by job size)
  int scan_min;     // SMP_SCAN_MIN: scans of trees of at least this many nodes are split over the helpers (0: never)
  int scan_pnn;     // SMP_SCAN_PNN / SMP_SCAN_PNEAR: caps on the participants of a split nearest / near scan, within
  int scan_pnear;   // [2, SCAN_P] / [2, SCAN_PNEAR]
  int scan_nshift;  // SMP_SCAN_NSHIFT: one near-scan participant per 2^scan_nshift nodes
  int scan_ps0;     // SMP_SCAN_PS0
  int helper_cap;   // SMP_HELPER_CAP: most helpers of a query with scouts
  int lead_div;     // SMP_LEAD_DIV: the leader's share of the helpers (1 / n)
  int pre_lead_div; // SMP_PRE_LEAD_DIV: the leader's share of a pre-solution query's helpers (1 / n)
  int pre_helpers;  // SMP_PRE_HELPERS: helpers of each pre-solution-only scout
  int pre_delay;    // SMP_PRE_DELAY
  int early_ask;    // SMP_EARLY_ASK
  int pre_refresh;  // SMP_PRE_REFRESH
  int conn_check;   // SMP_CONN_CHECK
  int pre_commit;   // SMP_PRE_COMMIT
  int pre_scouts;   // SMP_PRE_SCOUTS
  int rebalance;    // SMP_REBALANCE: on iff the helpers are automatic; the variable can only turn it off
  int rebalance_div;  // SMP_REBALANCE_DIV
  double slice_ms;    // SMP_SLICE_MS
  int xcd_margin;     // SMP_XCD_MARGIN
  double wait_slack_s;  // SMP_WAIT_SLACK_S
  int chunk0;           // SMP_CHUNK0: iterations of the first launch
  bool host_prof, debug, debug_scouts, bounds;  // SMP_HOST_PROF, SMP_DEBUG, SMP_DEBUG_SCOUTS, SMP_BOUNDS: set at all
  bool conn_prof;         // SMP_CONN_PROF: print the scouts' connect clocks per launch (SMP_CONN_PROF builds)
  int scout_conn_ov_max;  // SMP_SCOUT_CONN_OV_MAX: nodes up to which a scout scans tree_B for connect under its rewire job
};

// helpers: smp_params.helpers; nq: queries of the call.
PlanKnobs read_plan_knobs(int helpers, int nq);

struct ProvisionIn {
  int slots;       // co-resident workgroups this planner may use (already divided by slot_share)
  int num_cus, num_xcd, slot_share;
  int helpers, scout;  // smp_params
};

struct QueryProvision {
  int nscouts, nworkers, sampler;
  int sworkers_s[PROV_MAX_SCOUTS];  // [0, ns) are decided; the rest is 1
};

struct Provision {
  int nh = 0, ns = 0, ns_base = 0;  // of the launch: helpers per query, most scouts of a query, scouts after a first path
  std::vector<QueryProvision> q;    // per active query, in the order of have_sol
};

// have_sol[k]: the k-th of the n_act queries to launch has a path already.
void provision(const ProvisionIn& in, const PlanKnobs& k, const char* have_sol, int n_act, Provision* out);

}  // namespace smp
