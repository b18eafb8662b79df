// Driver of the margin checks' host threshold (csrc/smp_paths.cpp: margin_threshold), built with ASAN / UBSAN by
// tests/test_margin_cpu.py.  stdin: lines "r m" (hex floats); stdout per line: S, then fl(fl(sqrt(S)) - r) and the same
// of the next double above S, all as hex floats, so the test sees the function's own arithmetic and checks it again.
#include <cmath>
#include <cstdio>

#include "../../squirrel_motion_planner_amd/csrc/smp_paths.h"

int main() {
  double r, m;
  while (std::scanf("%la %la", &r, &m) == 2) {
    const double S = smp::margin_threshold(r, m);
    const double up = std::nextafter(S, HUGE_VAL);
    const double t = std::sqrt(S), tu = std::sqrt(up);
    std::printf("%a %a %a\n", S, t - r, tu - r);
  }
  return 0;
}
