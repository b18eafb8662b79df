// smp_robot_attach's model surgery and the sphere covers.  See smp_attach.h.
//
// The arithmetic that places the object's spheres in their body's frame is tools/gen_robot_model.py's to_body, term
// by term (fp64, no contraction), over the tree frames RobotHost keeps: the augmented model written as JSON and read
// by smp_robot_create_json gives the same doubles.
#include "smp_attach.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace smp {
namespace {

struct Frame {
  double R[9], p[3];
};

void rot_vec(const double* a, const double* v, double* o) {
  for (int r = 0; r < 3; ++r) o[r] = a[r * 3 + 0] * v[0] + a[r * 3 + 1] * v[1] + a[r * 3 + 2] * v[2];
}
Frame frame_mul(const Frame& f1, const Frame& f2) {
  Frame o;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c)
      o.R[r * 3 + c] = f1.R[r * 3 + 0] * f2.R[0 * 3 + c] + f1.R[r * 3 + 1] * f2.R[1 * 3 + c] + f1.R[r * 3 + 2] * f2.R[2 * 3 + c];
  double mp[3];
  rot_vec(f1.R, f2.p, mp);
  for (int i = 0; i < 3; ++i) o.p[i] = mp[i] + f1.p[i];
  return o;
}

// gen_robot_model.py offset(): F_{body+1} * ... * F_parent * F_new, left-associated; F_new is the identity frame.
Frame offset_of_new(const RobotHost& h, int body_link, int parent) {
  std::vector<int> path;
  for (int i = parent; i != body_link; i = h.link_parent[i]) path.push_back(i);
  Frame f{{1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 0, 0}};
  bool first = true;
  for (auto it = path.rbegin(); it != path.rend(); ++it) {
    Frame fk;
    std::memcpy(fk.R, &h.link_R[(size_t)*it * 9], sizeof(fk.R));
    std::memcpy(fk.p, &h.link_p[(size_t)*it * 3], sizeof(fk.p));
    f = first ? fk : frame_mul(f, fk);
    first = false;
  }
  const Frame ident{{1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 0, 0}};
  return first ? ident : frame_mul(f, ident);
}

void to_body(const Frame& f, const double* c, double* o) {
  double m[3];
  rot_vec(f.R, c, m);
  for (int d = 0; d < 3; ++d) o[d] = m[d] + f.p[d];
}

int find_link(const RobotHost& h, const char* name) {
  if (!name) return -1;
  for (size_t i = 0; i < h.link_names.size(); ++i)
    if (h.link_names[i] == name) return (int)i;
  return -1;
}

}  // namespace

int robot_attach(const RobotHost& base, const smp_attach& a, RobotHost* out) {
  if (!out || !a.link || !a.name || !a.name[0] || a.n_spheres < 1 || !a.centres || !a.radii || a.n_touch < 0 ||
      (a.n_touch > 0 && !a.touch_links))
    return SMP_ERR_ARG;
  const size_t nl = base.link_names.size();
  if (!base.has_tree || base.link_parent.size() != nl || base.clink_of_link.size() != nl) return SMP_ERR_ARG;
  const int parent = find_link(base, a.link);
  if (parent < 0 || find_link(base, a.name) >= 0) return SMP_ERR_ARG;
  for (int k = 0; k < a.n_spheres; ++k) {
    for (int d = 0; d < 3; ++d)
      if (!std::isfinite(a.centres[k * 3 + d])) return SMP_ERR_ARG;
    if (!std::isfinite(a.radii[k]) || !(a.radii[k] > 0.0) || a.radii[k] > GRID_REACH) return SMP_ERR_ARG;
  }
  const RobotDev& bd = base.dev;
  std::vector<char> touch(bd.n_clink, 0);
  for (int t = 0; t < a.n_touch; ++t) {
    const int l = find_link(base, a.touch_links[t]);
    if (l < 0 || base.clink_of_link[l] < 0) return SMP_ERR_ARG;
    touch[base.clink_of_link[l]] = 1;
  }
  // the parent's body: its nearest movable ancestor-or-self, which the body chain must place
  int body_link = parent;
  while (body_link >= 0 && base.link_joint[body_link] < 0) body_link = base.link_parent[body_link];
  if (body_link < 0) return SMP_ERR_ARG;
  const auto bit = std::find(base.bodies.begin(), base.bodies.end(), body_link);
  if (bit == base.bodies.end()) return SMP_ERR_ARG;
  const int body = (int)(bit - base.bodies.begin());

  // capacities, before anything is written
  const int n = a.n_spheres, nc = bd.n_clink;
  if (bd.n_sph + n > MAX_SPH || nc + 1 > MAX_CLINK) return SMP_ERR_CAPACITY;
  std::vector<int> partners;  // collision links that get a pair with the object
  long long spairs = bd.n_spairs, ppairs = bd.n_ppairs;
  for (int i = 0; i < nc; ++i) {
    if (bd.cl_body[i] == body || touch[i]) continue;
    partners.push_back(i);
    if (bd.cl_prim[i] >= 0) ppairs += n;
    else spairs += (long long)bd.cl_nsph[i] * n;
  }
  if (bd.n_pairs + (int)partners.size() > MAX_PAIRS || spairs > MAX_SPAIRS || ppairs > MAX_PPAIRS) return SMP_ERR_CAPACITY;

  RobotHost r = base;
  RobotDev& d = r.dev;
  const int new_link = (int)nl;
  r.link_names.push_back(a.name);
  r.clink_of_link.push_back(nc);
  r.link_parent.push_back(parent);
  r.link_joint.push_back(-1);
  const double I9[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  r.link_R.insert(r.link_R.end(), I9, I9 + 9);
  r.link_p.insert(r.link_p.end(), 3, 0.0);

  const Frame f = offset_of_new(base, body_link, parent);
  for (int k = 0; k < n; ++k) {
    const int s = bd.n_sph + k;
    d.sph_body[s] = body;
    d.sph_clink[s] = nc;
    to_body(f, &a.centres[k * 3], &d.sph_cb[s * 3]);
    d.sph_r[s] = a.radii[k];
  }
  d.n_sph = bd.n_sph + n;
  // the link bound (gen_robot_model.py: componentwise mean with sums in list order, max(dist + r) + 1e-6)
  double c[3] = {0.0, 0.0, 0.0}, rb = 0.0;
  for (int k = 0; k < n; ++k)
    for (int e = 0; e < 3; ++e) c[e] = c[e] + a.centres[k * 3 + e];
  for (int e = 0; e < 3; ++e) c[e] = c[e] / n;
  for (int k = 0; k < n; ++k) {
    const double dx = a.centres[k * 3] - c[0], dy = a.centres[k * 3 + 1] - c[1], dz = a.centres[k * 3 + 2] - c[2];
    rb = std::max(rb, std::sqrt(dx * dx + dy * dy + dz * dz) + a.radii[k]);
  }
  rb = rb + 1e-6;
  d.cl_sph0[nc] = bd.n_sph;
  d.cl_nsph[nc] = n;
  d.cl_body[nc] = body;
  d.cl_link[nc] = new_link;
  to_body(f, c, &d.cl_cb[nc * 3]);
  d.cl_r[nc] = rb;
  d.cl_prim[nc] = -1;
  d.n_clink = nc + 1;
  // self pairs in lexicographic (link a, link b) order
  std::vector<std::pair<int, int>> pairs;
  for (int p = 0; p < bd.n_pairs; ++p) pairs.push_back({bd.pair_a[p], bd.pair_b[p]});
  for (int i : partners) pairs.push_back({i, nc});
  std::stable_sort(pairs.begin(), pairs.end(), [&](const std::pair<int, int>& x, const std::pair<int, int>& y) {
    return std::make_pair(d.cl_link[x.first], d.cl_link[x.second]) < std::make_pair(d.cl_link[y.first], d.cl_link[y.second]);
  });
  d.n_pairs = (int)pairs.size();
  for (int p = 0; p < d.n_pairs; ++p) { d.pair_a[p] = pairs[p].first; d.pair_b[p] = pairs[p].second; }
  // the flat lists are rebuilt in full: clear what the base's longer or differently ordered lists left behind
  std::memset(d.sp_ab, 0, sizeof(d.sp_ab));
  std::memset(d.sp_rr2, 0, sizeof(d.sp_rr2));
  std::memset(d.pp_ps, 0, sizeof(d.pp_ps));
  try {
    finish_pairs(&d);
  } catch (const std::exception&) {
    return SMP_ERR_CAPACITY;
  }
  *out = std::move(r);
  return SMP_OK;
}

namespace {

// m spheres on the axis `ax` of a volume with half length ha along it and cross radius rho (smp_gpu.h "Attached
// objects"), mapped by the pose.
int cover_axis(double ha, double rho, int ax, const double* pose, double tol, int max_spheres, double* centres,
               double* radii, int* n) {
  if (!centres || !radii || !n || max_spheres < 1 || !std::isfinite(tol) || !(tol > 0.0) || !std::isfinite(ha) ||
      !std::isfinite(rho) || !(ha > 0.0) || rho < 0.0)
    return SMP_ERR_ARG;
  if (pose)
    for (int i = 0; i < 12; ++i)
      if (!std::isfinite(pose[i])) return SMP_ERR_ARG;
  const double t = rho + tol;
  const double reach = std::sqrt(t * t - rho * rho);
  const double want = std::ceil(ha / reach);
  if (!(want >= 1.0) && !(want < 1.0)) return SMP_ERR_ARG;  // NaN
  const int m = want >= (double)max_spheres ? max_spheres : std::max(1, (int)want);
  const double step = ha / m;
  const double rad = std::sqrt(step * step + rho * rho);
  if (!std::isfinite(rad)) return SMP_ERR_ARG;
  for (int k = 0; k < m; ++k) {
    double c[3] = {0.0, 0.0, 0.0};
    c[ax] = -ha + (double)(2 * k + 1) * step;
    if (pose) {
      double w[3];
      rot_vec(pose, c, w);
      for (int e = 0; e < 3; ++e) centres[k * 3 + e] = w[e] + pose[9 + e];
    } else {
      for (int e = 0; e < 3; ++e) centres[k * 3 + e] = c[e];
    }
    radii[k] = rad;
  }
  *n = m;
  return SMP_OK;
}

}  // namespace
}  // namespace smp

extern "C" {

int smp_cover_box(const double half[3], const double pose[12], double tol, int max_spheres, double* centres,
                  double* radii, int* n) {
  if (!half) return SMP_ERR_ARG;
  for (int i = 0; i < 3; ++i)
    if (!std::isfinite(half[i]) || !(half[i] > 0.0)) return SMP_ERR_ARG;
  int ax = 0;
  for (int i = 1; i < 3; ++i)
    if (half[i] > half[ax]) ax = i;
  const double u = half[ax == 0 ? 1 : 0], v = half[ax == 2 ? 1 : 2];
  return smp::cover_axis(half[ax], std::sqrt(u * u + v * v), ax, pose, tol, max_spheres, centres, radii, n);
}

int smp_cover_cylinder(double radius, double half_length, const double pose[12], double tol, int max_spheres,
                       double* centres, double* radii, int* n) {
  if (!std::isfinite(radius) || !(radius > 0.0)) return SMP_ERR_ARG;
  return smp::cover_axis(half_length, radius, 2, pose, tol, max_spheres, centres, radii, n);
}

}  // extern "C"
