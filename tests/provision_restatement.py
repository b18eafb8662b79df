"""Python restatement of the planner's provisioning rule: how many scouts and helpers each query of a launch gets
(DESIGN.md "Helpers", "Scouts", "Many queries"), shared by test_provision_cpu.py.

It follows the rule as the planning driver stated it before it became csrc/smp_provision.cpp (the `provision` lambda of
smp_plan_batch and its `split`), clamp by clamp: the automatic scout count by workgroups per query, the helper cap, the
pre-solution scouts, the per-XCD budget, the co-residency clamp and the split of the helpers between the leader, the
scouts and the sampler.  Every division is C's: of non-negative integers here, so Python's // agrees."""

MAX_SCOUTS = 8  # smp_plan.h

# the SMP_* knobs the rule reads, at their defaults
KNOBS = dict(helper_cap=200, lead_div=3, pre_lead_div=5, pre_helpers=12, pre_scouts=1, xcd_margin=1)


def split(nh, ns_base, knobs, nsq):
    """(h_lead, h_s): the helpers of the leader and of each scout of a query with nsq scouts."""
    h_lead = 0
    h_s = [0] * MAX_SCOUTS
    if nh < 1:
        return h_lead, h_s
    if nsq > ns_base:  # pre-solution scouts
        avail = nh - 1
        h_lead = avail // knobs["pre_lead_div"]
        per = (avail - h_lead) // nsq
        for s in range(nsq):
            h_s[s] = per
        h_s[0] += avail - h_lead - per * nsq
    elif nsq > 0:
        avail = nh - 1  # minus the sampler
        h_lead = avail // knobs["lead_div"] if nsq >= 2 else avail // 2
        rest = avail - h_lead
        for s in range(2, nsq):
            h_s[s] = min(knobs["pre_helpers"], rest)
            rest -= h_s[s]
        if nsq >= 2:
            h_s[0] = rest - rest // 2
            h_s[1] = rest // 2
        else:
            h_s[0] = rest
    return h_lead, h_s


def provision(slots, num_cus, num_xcd, slot_share, helpers, scout, have_sol, knobs=None):
    """(nh, ns, ns_base, [(nscouts, nworkers, sampler, sworkers_s[0..ns)) per query]); have_sol: one flag per active
    query."""
    kn = dict(KNOBS)
    kn.update(knobs or {})
    cap_s = kn["helper_cap"]
    nh_req = helpers
    want_scout = scout != 0
    na = max(1, len(have_sol))
    cpq = max(1, slots // na)
    nh = nh_req
    ns = 0
    if nh == 0:
        if want_scout:
            ns = 4 if cpq >= 64 else 2 if cpq >= 18 else 1 if cpq >= 6 else 0
        if want_scout and scout > 1:
            ns = min(scout, MAX_SCOUTS)
        nh = min(cap_s, max(0, cpq - 1 - ns)) if want_scout else min(63, max(0, cpq - 1))
    elif nh > 0 and want_scout:
        ns = 2 if nh >= 16 else 1 if nh >= 4 else 0
    if want_scout and scout > 1:
        ns = min(scout, MAX_SCOUTS)
    if nh < 0:
        nh = 0
    if nh < 4:
        ns = 0
    ns_base = ns
    if kn["pre_scouts"] and nh_req == 0 and scout == 1 and ns == 2:
        if not all(have_sol):
            ns = 4
    nx = num_xcd
    if nx > 1 and num_cus >= nx:
        per_xcd = num_cus // nx // max(1, slot_share)
        plan_max = (1 + ns) * ((na + nx - 1) // nx)
        free_xcd = max(0, per_xcd - plan_max - kn["xcd_margin"])
        hcap = nx * free_xcd // na
        if nh > hcap:
            nh = max(0, min(hcap, cap_s) if nh_req > 0 else hcap)
        if nh < 4:
            ns = 0
            ns_base = 0
    if 1 + ns + nh > cpq:
        nh = max(0, min(cap_s, cpq - 1 - ns) if want_scout else min(63, cpq - 1))
        if nh < 4:
            ns = 0
            ns_base = 0
            nh = max(0, min(nh, cpq - 1))
    queries = []
    for sol in have_sol:
        nsq = ns_base if ns > ns_base and sol else ns
        h_lead, h_s = split(nh, ns_base, kn, nsq)
        sampler = 1 if nh >= 2 else 0
        nworkers = 1 + h_lead if nsq > 0 else (nh if nh >= 2 else 1 + nh)
        queries.append((nsq, nworkers, sampler, [1 + h_s[s] for s in range(ns)]))
    return nh, ns, ns_base, queries
