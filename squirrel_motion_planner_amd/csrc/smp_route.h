// Host logic of the far-goal stage, free of HIP (plain C++17, built with the library and on its own by the CPU tests):
// the base lattice's checks, the route search over a free map and what smp_plan_far does with a chain between its
// launches (include/smp_gpu.h "Far goals").  It sees plain values, never smp_planner.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/smp_gpu.h"
#include "smp_pass.h"

namespace smp {

// The lattice as the kernels and the route search read it.  SMP_ERR_ARG for a NULL argument, a non-finite field,
// pitch <= 0 or a count < 1; SMP_ERR_CAPACITY for more than SMP_LATTICE_MAX_NODES nodes.
int lattice_dev(const smp_base_lattice* lat, LatticeDev* d);

inline bool lattice_free(const uint32_t* bits, int64_t n) { return (bits[n >> 5] >> (n & 31)) & 1u; }

// The rows of the chain's first n nodes (n x 3: ix, iy, t; n >= 1) with runs of equal step merged: a node is kept
// where the step changes, plus both ends; each row is the node's configuration (lattice_coord).
std::vector<double> chain_rows(const LatticeDev& lat, const int32_t* chain, int64_t n);

// The handover of smp_plan_far: with the chain c_0 .. c_m (n = m + 1 nodes), acc = 0 and j = m; while j > 0 and
// acc < distance, the planar length of the step c_j -> c_j-1 is added and j decremented.  Returns j.
int64_t handover_index(const LatticeDev& lat, const int32_t* chain, int64_t n, double distance);

}  // namespace smp
