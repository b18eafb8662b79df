// A grasped object as one more collision link of a robot model (smp_robot_attach), and sphere covers of a box or a
// cylinder for callers that hold a bounding volume (smp_cover_box / smp_cover_cylinder).  Host only, no HIP: the unit
// builds with smp_host.cpp alone (tests/cpp/attach_table.cpp).
#pragma once
#include "../../include/smp_gpu.h"
#include "smp_host.h"

namespace smp {

// base with the object of `a` appended: one link after all links (parent a->link, fixed, identity frame), its spheres
// after all spheres, one link bound and the self pairs (i, new) -- the RobotHost robot_from_model_value builds from
// base's model with these additions, byte for byte in RobotDev.  SMP_OK, SMP_ERR_ARG or SMP_ERR_CAPACITY; *out is
// written on SMP_OK only.
int robot_attach(const RobotHost& base, const smp_attach& a, RobotHost* out);

}  // namespace smp
