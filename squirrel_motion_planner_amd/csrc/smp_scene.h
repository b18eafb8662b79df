// Device scene build (smp_scene.hip): launch interface for smp_api.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "smp_carve.h"

namespace smp {

struct SceneBuildArgs {
  const uint16_t* keys;  // device, n_keys x 3
  long long n_keys;
  int kmin[3];           // key of cell (0, 0, 0)
  int nx, ny, nz;
  unsigned long long* bits;   // scratch, scene_words() words each: occupancy bits / dilated bits
  unsigned long long* dil;
  unsigned long long* count;  // scratch, one word: distinct occupied cells
  unsigned long long* bricks; // outputs (the planner's scene arrays)
  uint16_t* d2;
  uint8_t* d2b;               // nullptr: no byte copy
  int n_prim;
  const int* k01;             // device, n_prim x (k0, k1): the layers each primitive's slab projects
  uint16_t* slab;
  // self filter (smp_carve.h), nullptr: none.  Its launches run after the scatter of the keys and clear the carved
  // keys' bits, so every derived array sees the carved occupancy; hipEventRecord of ev[0] / ev[1] (when given) brackets
  // them on the stream.
  const CarveArgs* carve = nullptr;
  hipEvent_t carve_ev[2] = {nullptr, nullptr};
};

// Whether the passes can stage this grid's lines in LDS and index their launches (false: lines of more than 32768
// cells along y or z, or more than 2^19 along x).
bool scene_build_fits(int nx, int ny, int nz, int n_prim);
// 64-bit words each of the two bit scratch buffers needs.
size_t scene_words(int nx, int ny, int nz, int n_prim);
// Enqueues every pass on `st`; no synchronisation.
hipError_t launch_scene_build(hipStream_t st, const SceneBuildArgs& a);
// The byte copy min(d2, 255) of n cells of a finished box-gap field (both device arrays, as hipMalloc aligns them);
// enqueued on `st`, no synchronisation.
hipError_t launch_scene_bytes(hipStream_t st, const uint16_t* d2, long long n, uint8_t* d2b);
size_t scene_kernels_private_bytes();

}  // namespace smp
