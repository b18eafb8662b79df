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

// What the route searches share (smp_base_route here, the device field's calls in smp_api_field.cpp).
// The lattice with its free map, as a search reads it.
struct RouteLattice {
  LatticeDev d;
  int nx, ny, nt, wrap;
  const uint32_t* bits;
  int64_t node(int ix, int iy, int t) const { return ((int64_t)t * ny + iy) * nx + ix; }
  bool free_at(int ix, int iy, int t) const {
    return ix >= 0 && ix < nx && iy >= 0 && iy < ny && lattice_free(bits, node(ix, iy, t));
  }
};
// The three step weights: axis = pitch, diag = sqrt(pitch * pitch + pitch * pitch), turn = fabs(dtheta).
struct RouteWeights {
  double axis, diag, turn;
};
RouteWeights route_weights(const LatticeDev& d);
// lattice_dev's checks, then the search's view of the lattice.
int route_lattice(const smp_base_lattice* lat, const uint32_t* free_bits, RouteLattice* L);
// The snapping of smp_base_route: r->from_node and r->to_node, (-1, -1, -1) for the end that fails (and for to_node
// when from fails: the caller presets it); SMP_ERR_ARG, SMP_ERR_START_INVALID or SMP_ERR_GOAL_INVALID.
int route_ends(const RouteLattice& L, const double from[3], const double to[3], int snap_cells, smp_route_info* r);
// smp_base_route's Dijkstra from src: dp and parent of every node (+inf and -1 where not relaxed), *n_settled the nodes
// popped.  It stops when dst is settled and returns true; dst < 0 (or never reached) runs the heap empty: false.
bool route_search(const RouteLattice& L, int64_t src, int64_t dst, std::vector<double>* dp, std::vector<int32_t>* parent,
                  int64_t* n_settled);
// The call's buffers from a chain (start first; ix, iy, t per node): the merged rows and, with out_chain, the chain.
// SMP_ERR_CAPACITY when they cannot be had.
int route_output(const RouteLattice& L, const std::vector<int32_t>& chain, double** out_rows, int64_t* n_out,
                 int32_t** out_chain);

}  // namespace smp
