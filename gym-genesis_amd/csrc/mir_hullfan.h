// mir_hullfan.h — the faces of a convex hull given by its vertices, as planes and as triangle fans (host only: no HIP in it).
// Used by mir_dist.hip, once per handle, for every MIR_GEOM_HULL geom: the signed distance of a point inside the hull is the largest
// plane value, of a point outside the smallest point-triangle distance over the fans.
//   planes:    brute force over vertex triples (<= 32 vertices): a triple is a face when every vertex lies on one side of its plane
//              (the rule of mir_ray.hip's table and of tests/ray_ref.py); triples of one face give one plane.
//   triangles: per face, the vertices in its plane ordered by angle about the face's centroid (counter-clockwise seen from outside),
//              then the fan (v_0, v_i, v_i+1).  A face of k vertices gives k - 2 triangles; a hull of V vertices at most 2 V - 4.
#pragma once
#include <algorithm>
#include <cmath>
#include <utility>
#include <vector>

struct HullFan {
  std::vector<float> planes;  // 4 per face: unit outward normal, offset (n . x <= d inside)
  std::vector<float> tris;    // 12 per triangle: a xyz, face index; b xyz, 0; c xyz, 0
};

// appends the faces of the hull of v[0 .. nv) to `out`; false: the hull has no volume (its vertices lie in one plane)
inline bool hull_fan_build(const double (*v)[3], int nv, HullFan& out) {
  double scale = 0.0;
  for (int i = 0; i < nv; i++)
    for (int k = 0; k < 3; k++) scale = std::fmax(scale, std::fabs(v[i][k]));
  const double tol = 1e-6 * scale;
  std::vector<double> pl;  // this hull's planes, double
  bool volume = false;
  for (int i = 0; i < nv; i++)
    for (int j = i + 1; j < nv; j++)
      for (int k = j + 1; k < nv; k++) {
        const double e1[3] = {v[j][0] - v[i][0], v[j][1] - v[i][1], v[j][2] - v[i][2]}, e2[3] = {v[k][0] - v[i][0], v[k][1] - v[i][1], v[k][2] - v[i][2]};
        double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        const double len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        if (!(len > 1e-9 * scale * scale)) continue;  // (collinear)
        for (int c = 0; c < 3; c++) n[c] /= len;
        double d = n[0] * v[i][0] + n[1] * v[i][1] + n[2] * v[i][2], smin = 0.0, smax = 0.0;
        for (int m = 0; m < nv; m++) {
          const double s = n[0] * v[m][0] + n[1] * v[m][1] + n[2] * v[m][2] - d;
          smin = std::fmin(smin, s);
          smax = std::fmax(smax, s);
        }
        if (smax > tol && smin < -tol) continue;    // vertices on both sides: no face
        if (smax <= tol && smin >= -tol) continue;  // every vertex in this plane: no volume from this triple
        volume = true;
        if (smax > tol) { for (int c = 0; c < 3; c++) n[c] = -n[c]; d = -d; }
        bool dup = false;  // (another triple of the same face)
        for (size_t p = 0; p < pl.size() && !dup; p += 4) dup = n[0] * pl[p] + n[1] * pl[p + 1] + n[2] * pl[p + 2] > 1.0 - 1e-9 && std::fabs(d - pl[p + 3]) <= tol;
        if (dup) continue;
        pl.insert(pl.end(), {n[0], n[1], n[2], d});
      }
  if (!volume || pl.size() < 16) return false;
  for (size_t p = 0; p < pl.size(); p += 4) {
    const double* n = &pl[p];
    const int face = (int)(p / 4);
    std::vector<int> on;
    double c[3] = {0, 0, 0};
    for (int m = 0; m < nv; m++)
      if (std::fabs(n[0] * v[m][0] + n[1] * v[m][1] + n[2] * v[m][2] - n[3]) <= tol) {
        on.push_back(m);
        for (int k = 0; k < 3; k++) c[k] += v[m][k];
      }
    for (int k = 0; k < 3; k++) c[k] /= (double)on.size();
    // an in-plane basis (u, w) with u x w = n: angles grow counter-clockwise seen from outside
    const int ax = std::fabs(n[0]) <= std::fabs(n[1]) && std::fabs(n[0]) <= std::fabs(n[2]) ? 0 : (std::fabs(n[1]) <= std::fabs(n[2]) ? 1 : 2);
    double e[3] = {0, 0, 0}, u[3], w[3];
    e[ax] = 1.0;
    u[0] = n[1] * e[2] - n[2] * e[1]; u[1] = n[2] * e[0] - n[0] * e[2]; u[2] = n[0] * e[1] - n[1] * e[0];
    const double ul = std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    for (int k = 0; k < 3; k++) u[k] /= ul;
    w[0] = n[1] * u[2] - n[2] * u[1]; w[1] = n[2] * u[0] - n[0] * u[2]; w[2] = n[0] * u[1] - n[1] * u[0];
    std::vector<std::pair<double, int>> ang;
    for (int m : on) {
      const double r[3] = {v[m][0] - c[0], v[m][1] - c[1], v[m][2] - c[2]};
      ang.push_back({std::atan2(r[0] * w[0] + r[1] * w[1] + r[2] * w[2], r[0] * u[0] + r[1] * u[1] + r[2] * u[2]), m});
    }
    std::sort(ang.begin(), ang.end());
    for (size_t i = 1; i + 1 < ang.size(); i++) {
      const int t[3] = {ang[0].second, ang[i].second, ang[i + 1].second};
      for (int q = 0; q < 3; q++) {
        for (int k = 0; k < 3; k++) out.tris.push_back((float)v[t[q]][k]);
        out.tris.push_back(q == 0 ? (float)face : 0.0f);
      }
    }
    for (int k = 0; k < 4; k++) out.planes.push_back((float)n[k]);
  }
  return true;
}
