// Driver of the HIP-free attach unit (csrc/smp_attach.cpp with csrc/smp_host.cpp), built with ASAN / UBSAN by
// tests/test_attach_cpu.py.  argv[1]: the base model JSON.  stdin, one command per line, on a current robot that starts
// as the base model:
//   A link name n n_touch [touch ...] [3n centres] [n radii]   (hex floats)  attach to the current robot -> "status S"
//   R                                                           back to the base model
//   D                                                           "dev <hex of RobotDev>" and "links <names>"
//   F seed count                                                `count` seeded malformed attaches -> "fuzz ok arg cap"
//   B hx hy hz tol max | C radius half_length tol max           the covers -> "cover S n" then n lines "x y z r"
// "-" stands for a NULL link or name.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <limits>
#include <sstream>
#include <string>
#include <vector>

#include "../../squirrel_motion_planner_amd/csrc/smp_attach.h"

static double hexd(std::istream& in) {
  std::string t;
  in >> t;
  return std::strtod(t.c_str(), nullptr);
}

static uint64_t rng_state = 1;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream f(argv[1]);
  std::stringstream ss;
  ss << f.rdbuf();
  smp::RobotHost base;
  smp::robot_from_json(ss.str(), &base);
  smp::RobotHost cur = base;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    if (cmd == "R") {
      cur = base;
    } else if (cmd == "A") {
      std::string link, name;
      int n = 0, nt = 0;
      in >> link >> name >> n >> nt;
      std::vector<std::string> touch(nt > 0 ? nt : 0);
      for (auto& t : touch) in >> t;
      std::vector<const char*> tp;
      for (auto& t : touch) tp.push_back(t.c_str());
      std::vector<double> c(n > 0 ? 3 * n : 0), r(n > 0 ? n : 0);
      for (auto& x : c) x = hexd(in);
      for (auto& x : r) x = hexd(in);
      smp_attach a{};
      a.link = link == "-" ? nullptr : link.c_str();
      a.name = name == "-" ? nullptr : name.c_str();
      a.n_spheres = n;
      a.centres = c.data();
      a.radii = r.data();
      a.touch_links = tp.data();
      a.n_touch = nt;
      smp::RobotHost out;
      const int st = smp::robot_attach(cur, a, &out);
      if (st == SMP_OK) cur = out;
      std::printf("status %d\n", st);
    } else if (cmd == "D") {
      std::printf("dev ");
      const unsigned char* b = reinterpret_cast<const unsigned char*>(&cur.dev);
      for (size_t i = 0; i < sizeof(cur.dev); ++i) std::printf("%02x", b[i]);
      std::printf("\nlinks");
      for (const std::string& s : cur.link_names) std::printf(" %s", s.c_str());
      std::printf("\n");
    } else if (cmd == "F") {
      unsigned long long seed = 1;
      int count = 0;
      in >> seed >> count;
      rng_state = seed;
      int ok = 0, arg = 0, cap = 0;
      const double bad[] = {std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(), -1.0, 0.0,
                            0.46, 1e300, -0.0};
      for (int it = 0; it < count; ++it) {
        const int n = (int)(rnd() % 24) - 2;  // -2 .. 21: below 1 and beyond the capacity too
        std::vector<double> c(n > 0 ? 3 * n : 0), r(n > 0 ? n : 0);
        for (auto& x : c) x = (double)(rnd() % 2001) / 1000.0 - 1.0;
        for (auto& x : r) x = 0.01 + (double)(rnd() % 400) / 1000.0;
        const int what = (int)(rnd() % 8);
        if (what == 0 && n > 0) c[rnd() % c.size()] = bad[rnd() % 2];
        if (what == 1 && n > 0) r[rnd() % r.size()] = bad[rnd() % 7];
        const std::string& l0 = cur.link_names[rnd() % cur.link_names.size()];
        const std::string link = what == 2 ? "no_such_link" : l0;
        const std::string name = what == 3 ? cur.link_names[rnd() % cur.link_names.size()] : "fuzz_object";
        std::vector<std::string> touch;
        for (int t = (int)(rnd() % 4); t > 0; --t)
          touch.push_back(what == 4 && t == 1 ? "no_such_touch" : cur.link_names[rnd() % cur.link_names.size()]);
        std::vector<const char*> tp;
        for (auto& t : touch) tp.push_back(t.c_str());
        smp_attach a{};
        a.link = what == 5 ? nullptr : link.c_str();
        a.name = what == 6 ? nullptr : name.c_str();
        a.n_spheres = n;
        a.centres = what == 7 ? nullptr : c.data();
        a.radii = r.data();
        a.touch_links = tp.empty() ? nullptr : tp.data();
        a.n_touch = (int)tp.size();
        smp::RobotHost out;
        const int st = smp::robot_attach(cur, a, &out);
        if (st == SMP_OK) {
          if ((int)out.link_names.size() != (int)cur.link_names.size() + 1 || out.dev.n_sph != cur.dev.n_sph + n) return 3;
          ++ok;
        } else if (st == SMP_ERR_ARG) {
          ++arg;
        } else if (st == SMP_ERR_CAPACITY) {
          ++cap;
        } else {
          return 4;
        }
      }
      std::printf("fuzz %d %d %d\n", ok, arg, cap);
    } else if (cmd == "B" || cmd == "C") {
      double a0 = hexd(in), a1 = hexd(in), a2 = cmd == "B" ? hexd(in) : 0.0;
      const double tol = hexd(in);
      int mx = 0;
      in >> mx;
      std::vector<double> c(mx > 0 ? 3 * mx : 3), r(mx > 0 ? mx : 1);
      int n = 0;
      const double half[3] = {a0, a1, a2};
      const int st = cmd == "B" ? smp_cover_box(half, nullptr, tol, mx, c.data(), r.data(), &n)
                                : smp_cover_cylinder(a0, a1, nullptr, tol, mx, c.data(), r.data(), &n);
      std::printf("cover %d %d\n", st, st == SMP_OK ? n : 0);
      for (int k = 0; k < n && st == SMP_OK; ++k) std::printf("%a %a %a %a\n", c[3 * k], c[3 * k + 1], c[3 * k + 2], r[k]);
    }
  }
  return 0;
}
