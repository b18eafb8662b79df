// Self filter of the device scene build (smp_carve.hip): launch interface for smp_api.cpp and smp_scene.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "smp_types.h"

namespace smp {

// The selected items of the robot at the pose the map was taken, in world coordinates (device; written by the FK
// pre-launch, staged in LDS by every workgroup of the carve kernel).
struct CarveItems {
  int n_sph, n_prim;
  double box[6];                // the union of the items' boxes, inflated by pad: lo x, y, z, hi x, y, z
  double sph[MAX_SPH][4];       // centre, radius
  double pw[MAX_PRIM][5];       // centre, x axis (prim_world)
  double ph[MAX_PRIM][3];       // half extents (prim_h)
  int pty[MAX_PRIM];            // 1 box, 2 cylinder
};

struct CarveArgs {
  const RobotDev* rb;           // device model
  double q[NJ];                 // the robot's pose when the map was taken
  double pad;
  uint32_t links;               // bit c: collision link c is carved
  CarveItems* items;            // device scratch
  const uint16_t* keys;         // device, n_keys x 3
  long long n_keys;
  int kmin[3];                  // key of cell (0, 0, 0)
  double org[3], res;           // cell (i, j, k) is the box [org + i * res, org + (i + 1) * res] per axis
  // one of the two outputs: a flag per key (smp_carve_keys), or the carved keys' bits cleared in the build's bit grid
  uint8_t* flags;
  unsigned long long* bits;
  int nx, ny, nz;
  unsigned long long* count;    // device, one word, zeroed by the launch: carved keys
};
static_assert(MAX_CLINK <= 32, "the carved collision links in one 32-bit mask");

// Enqueues the FK pre-launch and the carve kernel on `st`; no synchronisation.
hipError_t launch_carve(hipStream_t st, const CarveArgs& a);
size_t carve_kernels_private_bytes();

}  // namespace smp
