// Table driver of the provisioning unit (csrc/smp_provision.cpp) for tests/test_provision_cpu.py; built with
// -fsanitize=address,undefined.
//
//   provision_table            cases from stdin, one per line:
//                                slots num_cus num_xcd slot_share helpers scout n have_sol_0 .. have_sol_n-1
//                              one line out per case: "nh ns ns_base", then per query
//                                "; nscouts nworkers sampler sworkers_s[0] .. sworkers_s[ns-1]"
//                              The knobs are those of this process' environment.
//   provision_table knobs H N  the PlanKnobs read from the environment for smp_params.helpers = H and N queries, one
//                              "name value" per line
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../squirrel_motion_planner_amd/csrc/smp_provision.h"

using namespace smp;

static int print_knobs(int helpers, int nq) {
  const PlanKnobs k = read_plan_knobs(helpers, nq);
  std::printf("tile_ct %d\nscan_min %d\nscan_pnn %d\nscan_pnear %d\nscan_nshift %d\nscan_ps0 %d\n", k.tile_ct, k.scan_min,
              k.scan_pnn, k.scan_pnear, k.scan_nshift, k.scan_ps0);
  std::printf("helper_cap %d\nlead_div %d\npre_lead_div %d\npre_helpers %d\npre_delay %d\nearly_ask %d\n", k.helper_cap,
              k.lead_div, k.pre_lead_div, k.pre_helpers, k.pre_delay, k.early_ask);
  std::printf("pre_refresh %d\nconn_check %d\npre_commit %d\npre_scouts %d\nrebalance %d\nrebalance_div %d\n",
              k.pre_refresh, k.conn_check, k.pre_commit, k.pre_scouts, k.rebalance, k.rebalance_div);
  std::printf("slice_ms %.17g\nxcd_margin %d\nwait_slack_s %.17g\nchunk0 %d\n", k.slice_ms, k.xcd_margin, k.wait_slack_s,
              k.chunk0);
  std::printf("host_prof %d\ndebug %d\ndebug_scouts %d\nbounds %d\n", (int)k.host_prof, (int)k.debug,
              (int)k.debug_scouts, (int)k.bounds);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && std::strcmp(argv[1], "knobs") == 0) return print_knobs(std::atoi(argv[2]), std::atoi(argv[3]));
  if (argc != 1) {
    std::fprintf(stderr, "usage: provision_table [knobs HELPERS NQ]\n");
    return 2;
  }
  ProvisionIn in;
  int n = 0;
  std::vector<char> have_sol;
  Provision pv;
  while (std::scanf("%d %d %d %d %d %d %d", &in.slots, &in.num_cus, &in.num_xcd, &in.slot_share, &in.helpers, &in.scout,
                    &n) == 7) {
    if (n < 0) return 2;
    have_sol.resize(n);
    for (int i = 0; i < n; ++i) {
      int f = 0;
      if (std::scanf("%d", &f) != 1) return 2;
      have_sol[i] = f ? 1 : 0;
    }
    const PlanKnobs k = read_plan_knobs(in.helpers, n);
    provision(in, k, have_sol.data(), n, &pv);
    std::printf("%d %d %d", pv.nh, pv.ns, pv.ns_base);
    for (int i = 0; i < n; ++i) {
      const QueryProvision& q = pv.q[i];
      std::printf(" ; %d %d %d", q.nscouts, q.nworkers, q.sampler);
      for (int s = 0; s < pv.ns; ++s) std::printf(" %d", q.sworkers_s[s]);
    }
    std::printf("\n");
  }
  return 0;
}
