// mir_dist_body.h — the two device pieces of the signed-distance query that mir_dist.hip (mir_signed_distance) and mir_plan.hip
// (mir_plan_path, mir_path_clearance) share, and the geometry table they read:
//   (a) dist_build_records(): lane = geom; the geoms whose skip bit is clear, compacted in geom order by a ballot into an LDS list of
//       24-float records (world frame of the geom, its sizes, where its hull planes and triangles lie in the table);
//   (b) dist_probe_min():     lane = probe; the minimum of (signed distance - radius) over the record list with the closest point and
//       the normal of the winner in its geom's frame.  The record address and the geom type are wave-uniform, every distance is a
//       closed form (see the header of mir_dist.hip).
// Both are called by whole waves (they hold a ballot each).  What surrounds them in those kernels -- the row's env, the body poses in
// LDS, the probe centres, the wave reductions, the pointers into the table (DistTabPtrs) -- is in mir_sphere_front.h, which includes
// this file.  Needs mir_dev.h and mir_query.h in front of it, inside no namespace.
#pragma once

namespace {

constexpr int DIST_MAX_PROBES = 1024;
constexpr int DIST_REC = 24;  // floats per LDS record

// per-handle geometry table (device): the geoms as the spec has them, and the face planes and triangle fans of every hull
struct DistGeom {
  int32_t type, body, p0, np, t0, nt, _pad[2];  // p0, np / t0, nt: the hull's planes / triangles behind the table
  float size[3], rad;                           // rad: radius of the bounding sphere about the geom frame's origin
  float pos[3], quat[4], _pad2;
};
struct DistTab {
  int32_t ngeom, nplane, ntri, _pad;
  DistGeom g[MIR_MAX_GEOM];
  // float4 planes[nplane], then float4 tris[3 * ntri] follow (geom frame)
};

// closest point of the triangle (a, b, c) to p: the regions of the Voronoi diagram of its features, highest priority last;
// `face`: the foot of p on the triangle's plane lies inside it and p is on the outer side (a, b, c counter-clockwise seen from outside)
__device__ __forceinline__ V3 closest_on_triangle(V3 p, V3 a, V3 b, V3 c, bool& face) {
  const V3 ab = b - a, ac = c - a, ap = p - a, bp = p - b, cp = p - c;
  const float d1 = dot(ab, ap), d2 = dot(ac, ap), d3 = dot(ab, bp), d4 = dot(ac, bp), d5 = dot(ab, cp), d6 = dot(ac, cp);
  const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  const float den = 1.0f / (va + vb + vc);
  float v = vb * den, w = vc * den;  // the face
  bool in = true;
  if (va <= 0.0f && d4 - d3 >= 0.0f && d5 - d6 >= 0.0f) { w = (d4 - d3) / ((d4 - d3) + (d5 - d6)); v = 1.0f - w; in = false; }  // edge bc
  if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) { w = d2 / (d2 - d6); v = 0.0f; in = false; }                                     // edge ac
  if (d6 >= 0.0f && d5 <= d6) { v = 0.0f; w = 1.0f; in = false; }                                                                // vertex c
  if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) { v = d1 / (d1 - d3); w = 0.0f; in = false; }                                     // edge ab
  if (d3 >= 0.0f && d4 <= d3) { v = 1.0f; w = 0.0f; in = false; }                                                                // vertex b
  if (d1 <= 0.0f && d2 <= 0.0f) { v = 0.0f; w = 0.0f; in = false; }                                                              // vertex a
  face = in && dot(ap, cross(ab, ac)) > 0.0f;
  return a + v * ab + w * ac;
}

// ---- (a) geom records, lane = geom: xp / xq are the body poses in LDS; returns how many records `rec` holds (the caller takes it
// through readfirstlane).  Ends with a WSYNC: the records may be read when it returns.
__device__ __forceinline__ int dist_build_records(const DistTab* __restrict__ t, unsigned long long skip, int lane, const float (*xp)[4],
                                                  const float (*xq)[4], float* rec) {
  const int ng = t->ngeom;
  const bool isg = lane < ng;
  const int g = isg ? lane : 0;
  const int b = t->g[g].body;
  const V3 bp = ld3(xp[b]);
  const Q4 bq = ld4(xq[b]);
  // geom frame in the world: c = xpos + R(xquat) g_pos, q = xquat (x) g_quat
  const V3 c = bp + qrot(bq, ld3(t->g[g].pos));
  const M3 Rg = q2m(qnormalize(qmul(bq, ld4(t->g[g].quat))));
  const bool keep = isg && !((skip >> g) & 1ull);
  const unsigned long long m = __ballot(keep);
  if (keep) {
    const int slot = __popcll(m & ((1ull << lane) - 1ull));
    float* r = rec + slot * DIST_REC;
    const int type = t->g[g].type;
    const float hl = type == MIR_GEOM_CAPSULE ? t->g[g].size[1] : 0.0f;
    r[0] = __int_as_float(type); r[1] = __int_as_float(g);
    r[2] = t->g[g].size[0]; r[3] = type == MIR_GEOM_BOX ? t->g[g].size[1] : hl; r[4] = t->g[g].size[2];
    r[5] = c.x; r[6] = c.y; r[7] = c.z;
    r[8] = Rg.r0.x; r[9] = Rg.r0.y; r[10] = Rg.r0.z;  // rows of R_g: its columns are the geom's axes in the world
    r[11] = Rg.r1.x; r[12] = Rg.r1.y; r[13] = Rg.r1.z;
    r[14] = Rg.r2.x; r[15] = Rg.r2.y; r[16] = Rg.r2.z;
    r[17] = __int_as_float(t->g[g].p0); r[18] = __int_as_float(t->g[g].np);
    r[19] = __int_as_float(t->g[g].t0); r[20] = __int_as_float(t->g[g].nt);
    r[21] = t->g[g].rad;
  }
  const int count = __popcll(m);
  WSYNC();
  return count;
}

// ---- (b) the minimum over the record list for the probe of this lane: centre pw (world) and radius
struct DistBest {
  float best;  // min over the records of (signed distance - radius); INFINITY when the list is empty
  int bestk;   // its record, -1: none
  V3 bc, bn;   // closest point and normal of the best geom, in its frame
};
__device__ __forceinline__ DistBest dist_probe_min(const float* rec, int count, const float* planes, const float* tris, V3 pw, float radius,
                                                   float max_distance) {
  float best = INFINITY;
  int bestk = -1;
  V3 bc = v3(0, 0, 0), bn = v3(0, 0, 0);
  for (int k = 0; k < count; k++) {
    const float* r = rec + k * DIST_REC;
    const int type = __builtin_amdgcn_readfirstlane(__float_as_int(r[0]));
    const V3 rel = pw - v3(r[5], r[6], r[7]);
    // p = R_g^T rel
    const V3 p = v3(r[8] * rel.x + r[11] * rel.y + r[14] * rel.z, r[9] * rel.x + r[12] * rel.y + r[15] * rel.z, r[10] * rel.x + r[13] * rel.y + r[16] * rel.z);
    float d;
    V3 cp, n;
    if (type == MIR_GEOM_PLANE) {
      d = p.z;
      cp = v3(p.x, p.y, 0.0f);
      n = v3(0, 0, 1);
    } else if (type == MIR_GEOM_BOX) {
      const float h[3] = {r[2], r[3], r[4]}, pp[3] = {p.x, p.y, p.z};
      float q[3], cl[3];
#pragma unroll
      for (int i = 0; i < 3; i++) {
        q[i] = fabsf(pp[i]) - h[i];
        cl[i] = fminf(fmaxf(pp[i], -h[i]), h[i]);
      }
      int im = 0;
      float qm = q[0];
      if (q[1] > qm) { qm = q[1]; im = 1; }
      if (q[2] > qm) { qm = q[2]; im = 2; }
      const V3 v = v3(pp[0] - cl[0], pp[1] - cl[1], pp[2] - cl[2]);
      const float dv = sqrtf(dot(v, v));
      if (qm > 0.0f && dv > 0.0f) {  // outside: the clamped point
        d = dv;
        n = (1.0f / dv) * v;
        cp = v3(cl[0], cl[1], cl[2]);
      } else {  // inside or on the surface: the nearest face, the lower axis on a tie
        d = qm;
        const float sg = pp[im] >= 0.0f ? 1.0f : -1.0f;
        n = v3(im == 0 ? sg : 0.0f, im == 1 ? sg : 0.0f, im == 2 ? sg : 0.0f);
        cp = v3(im == 0 ? sg * h[0] : pp[0], im == 1 ? sg * h[1] : pp[1], im == 2 ? sg * h[2] : pp[2]);
      }
    } else if (type == MIR_GEOM_HULL) {
      const int p0 = __builtin_amdgcn_readfirstlane(__float_as_int(r[17])), np = __builtin_amdgcn_readfirstlane(__float_as_int(r[18]));
      const int t0 = __builtin_amdgcn_readfirstlane(__float_as_int(r[19])), nt = __builtin_amdgcn_readfirstlane(__float_as_int(r[20]));
      float sm = -INFINITY;
      V3 nm = v3(0, 0, 1);
      for (int f = 0; f < np; f++) {
        const float* pl = planes + 4 * (p0 + f);
        const float px = pl[0], py = pl[1], pz = pl[2], pd = pl[3];
        const float s = px * p.x + py * p.y + pz * p.z - pd;
        if (s > sm) { sm = s; nm = v3(px, py, pz); }  // (strict: the lower face index on a tie)
      }
      d = sm;
      n = nm;
      cp = p - sm * nm;
      // outside: the triangles, unless no lane of the wave can improve on what it holds (|p| - rad bounds the distance from below)
      const bool need = sm > 0.0f && sqrtf(dot(p, p)) - r[21] - radius <= fminf(best, max_distance);
      if (__ballot(need) != 0ull) {
        // A triangle that holds the foot of p with p on its outer side holds the nearest point of the whole hull (the hull lies
        // behind that plane): it is taken outright.  Left to the comparison of squared distances, a point a little inside such a
        // triangle and the point of its edge that a neighbour offers differ by the SQUARE of their distance, and float32 picks either.
        float d2m = INFINITY;
        V3 cm = cp;
        bool done = false;
        for (int ti = 0; ti < nt; ti++) {
          const float* tr = tris + 12 * (t0 + ti);
          bool face;
          const V3 c = closest_on_triangle(p, v3(tr[0], tr[1], tr[2]), v3(tr[4], tr[5], tr[6]), v3(tr[8], tr[9], tr[10]), face);
          const V3 v = p - c;
          const float d2 = dot(v, v);
          if (!done && (face || d2 < d2m)) { d2m = d2; cm = c; }  // (strict: the lower face index on a tie)
          done = done || face;
        }
        if (sm > 0.0f) {
          const float dd = sqrtf(d2m);
          d = dd;
          cp = cm;
          if (dd > 0.0f) n = (1.0f / dd) * (p - cm);  // (dd == 0: on the surface to float32, the face's normal stays)
        }
      } else if (sm > 0.0f) {
        d = INFINITY;  // (cannot win, cannot be within max_distance)
      }
    } else {  // capsule about |z| <= hl (sphere: hl = 0)
      const float rad = r[2], hl = r[3];
      const float cz = fminf(fmaxf(p.z, -hl), hl);
      const V3 v = v3(p.x, p.y, p.z - cz);
      const float len = sqrtf(dot(v, v));
      d = len - rad;
      n = len > 0.0f ? (1.0f / len) * v : v3(0, 0, 1);  // (the centre, the axis: +z of the geom frame)
      cp = v3(rad * n.x, rad * n.y, cz + rad * n.z);
    }
    const float s = d - radius;
    if (s < best) { best = s; bestk = k; bc = cp; bn = n; }  // (strict: a tie stays with the lower geom index)
  }
  return {best, bestk, bc, bn};
}

}  // namespace

static_assert(sizeof(DistTab) % 16 == 0 && sizeof(DistGeom) % 16 == 0, "the planes and triangles behind the table are 16-byte rows");

// host: the geometry table of the handle, built by the first call that needs it (mir_dist.hip).  MIR_OK: h->dist_tab / h->dist_nplane
// are valid.  Errors are reported under the entry point `who`.
int mir_dist_table(MirScene* h, const char* who);
