// mir_blend_front.h — the host-side checks of mir_blend_path and the pure part of its rule (mir_blend.hip; include/mirigid.h, "corner
// blending"): plain C++, no HIP in it, so that tests/blend_host.cpp builds it with g++ (`make blend-host`) and tests/test_blend_cpu.py
// walks every refusal and compares the compaction, the half-lengths, the check counts and the point count with the NumPy rule without
// a device.  The kernel calls the same scalar functions (BLEND_HD makes them device functions under hipcc) with a dof per lane;
// blend_row() below is the same rule over arrays, for the host.
// A refusal is `refuse(code, text)`: the caller's, which names the entry point.  The order of the checks and their texts are part of
// the interface.
#pragma once
#include <math.h>
#include <stdint.h>

#include "mirigid.h"

#ifdef __HIPCC__
#define BLEND_HD __host__ __device__ __forceinline__
#else
#define BLEND_HD static inline
#endif

namespace {

// what the entry point was handed, as far as these checks read it (the clearance side is checked by the planner's front end)
struct BlendCall {
  bool handle;
  const MirBlendQuery* q;
  const void *pq, *probes, *dof_qadr, *poly, *points, *n_points, *status, *path;
};

template <class Refuse>
static int blend_check(const BlendCall& c, Refuse refuse) {
  const MirBlendQuery* const q = c.q;
  if (!c.handle || !q || !c.pq || !c.probes || !c.dof_qadr || !c.poly || !c.points || !c.n_points || !c.status)
    return refuse(MIR_E_INVALID, "null argument");
  if (q->struct_size != (int32_t)sizeof(MirBlendQuery)) return refuse(MIR_E_INVALID, "struct_size is not sizeof(MirBlendQuery)");
  if (q->num_nodes < 2) return refuse(MIR_E_INVALID, "num_nodes < 2");
  if (q->num_nodes > MIR_PLAN_MAX_POLY) return refuse(MIR_E_CAPACITY, "num_nodes > MIR_PLAN_MAX_POLY");
  if (q->blend_points < 2 || q->blend_points > MIR_BLEND_MAX_POINTS_PER_CORNER) return refuse(MIR_E_INVALID, "blend_points outside 2 .. 64");
  if (q->max_shrinks < 0) return refuse(MIR_E_INVALID, "max_shrinks < 0");
  if (q->max_points < 2) return refuse(MIR_E_INVALID, "max_points < 2");
  if (q->num_waypoints < 0 || q->num_waypoints == 1) return refuse(MIR_E_INVALID, "num_waypoints must be 0 or >= 2");
  if (q->num_waypoints >= 2 && !c.path) return refuse(MIR_E_INVALID, "num_waypoints >= 2 without path");
  if (q->num_waypoints == 0 && c.path) return refuse(MIR_E_INVALID, "path with num_waypoints == 0");
  if (q->flags) return refuse(MIR_E_INVALID, "unknown flag bit in MirBlendQuery");
  if (!(isfinite(q->max_deviation) && q->max_deviation > 0.0f)) return refuse(MIR_E_INVALID, "max_deviation must be finite and > 0");
  return MIR_OK;
}

// R x max(P, W) x D floats must be addressable by 31 bits (behind the planner's front end, which yields R and D)
template <class Refuse>
static int blend_check_size(const MirBlendQuery* q, long long R, int D, Refuse refuse) {
  const long long per_row = (long long)(q->max_points > q->num_waypoints ? q->max_points : q->num_waypoints) * D;
  if (R > 0 && per_row > 0x7fffffffLL / R) return refuse(MIR_E_CAPACITY, "rows x max_points x n_dofs beyond 2^31 - 1");
  return MIR_OK;
}

// ---- the rule.  x / y with one refinement of the quotient: the division of the planner's edge rule (div_refined)
BLEND_HD float blend_div(float x, float y) {
  const float r = 1.0f / y;
  const float t = x * r;
  return fmaf(fmaf(-t, y, x), r, t);
}

BLEND_HD bool blend_finite(float x) { return fabsf(x) <= 3.4028234664e38f; }  // (false for a NaN)

// the valid leading nodes of a row of K
BLEND_HD int blend_valid(int n_poly, int K) { return n_poly < 1 ? 1 : n_poly > K ? K : n_poly; }

// the dense points a row of M kept nodes can need: 2 + (M - 2)(m + 1)
BLEND_HD long long blend_worst_points(int M, int m) { return M < 2 ? 1 : 2 + (long long)(M - 2) * (m + 1); }

// a component of the unit direction: d / L, 0 when L underflowed to 0
BLEND_HD float blend_unit(float d, float L) { return L > 0.0f ? blend_div(d, L) : 0.0f; }

// the half-length of the blend between segments of length Lp and Ln whose unit directions differ by du (L2)
BLEND_HD float blend_half(float Lp, float Ln, float du, float delta) {
  float h = 0.5f * fminf(Lp, Ln);
  if (du > 0.0f) h = fminf(h, blend_div(4.0f * delta, du));
  return h;
}

// the samples of a check: max(1, ceil(2 reach / resolution)), at most MIR_BLEND_MAX_CHECK; reach = max_j max(|Q_j - A_j|, |C_j - Q_j|)
BLEND_HD int blend_count(float reach, float resolution) {
  const float c = blend_div(2.0f * reach, resolution);
  if (!blend_finite(c)) return MIR_BLEND_MAX_CHECK;
  if (c <= 1.0f) return 1;
  return c < (float)MIR_BLEND_MAX_CHECK ? (int)ceilf(c) : MIR_BLEND_MAX_CHECK;
}

// the parameter of sample k of n (0 and 1 exactly at the ends)
BLEND_HD float blend_param(int k, int n) { return k <= 0 ? 0.0f : k >= n ? 1.0f : blend_div((float)k, (float)n); }

// one dof of the blend: the ends of the curve and the curve itself by de Casteljau (the ends' own bits at t = 0 and t = 1)
BLEND_HD float blend_a(float q, float h, float up) { const float s = h * up; return q - s; }
BLEND_HD float blend_c(float q, float h, float un) { const float s = h * un; return q + s; }
BLEND_HD float blend_curve(float a, float q, float c, float t) {
  if (t <= 0.0f) return a;
  if (t >= 1.0f) return c;
  const float e0 = q - a, e1 = c - q;
  const float s0 = t * e0, s1 = t * e1;
  const float p = a + s0, r = q + s1;
  const float e2 = r - p;
  const float s2 = t * e2;
  return p + s2;
}

#ifndef __HIPCC__
// ---- the rule over arrays, for the host: steps 1, 3, 4 and the first check count of 6. of one row.  poly (K, D); kept (K): the input
// index of each kept node; h, n_c (K): per KEPT node, 0 at the ends.  Returns M; *not_finite, *worst (the point count of 1.).
static float blend_norm(const float* v, int D) {
  float acc = 0.0f;
  for (int j = 0; j < D; j++) {
    const float sq = v[j] * v[j];
    acc = acc + sq;
  }
  return sqrtf(acc);
}

static int blend_row(const float* poly, int K, int D, int n_poly, float delta, int m, float resolution, int32_t* kept, float* h, int32_t* n_c,
                     int* not_finite, long long* worst) {
  const int nv = blend_valid(n_poly, K);
  int M = 0;
  *not_finite = 0;
  for (int k = 0; k < nv; k++) {
    bool same = M > 0;
    for (int j = 0; j < D; j++) {
      const float v = poly[(size_t)k * D + j];
      if (!blend_finite(v)) *not_finite = 1;
      if (M > 0 && !(v == poly[(size_t)kept[M - 1] * D + j])) same = false;
    }
    if (!same) kept[M++] = k;
  }
  *worst = blend_worst_points(M, m);
  for (int i = 0; i < M; i++) { h[i] = 0.0f; n_c[i] = 0; }
  if (*not_finite) return M;
  float d[16], up[16], un[16], w[16];
  float Lp = 0.0f;
  for (int i = 0; i + 1 < M; i++) {
    const float* const a = poly + (size_t)kept[i] * D;
    const float* const b = poly + (size_t)kept[i + 1] * D;
    for (int j = 0; j < D; j++) d[j] = b[j] - a[j];
    const float Ln = blend_norm(d, D);
    for (int j = 0; j < D; j++) un[j] = blend_unit(d[j], Ln);
    if (i > 0) {
      for (int j = 0; j < D; j++) w[j] = un[j] - up[j];
      h[i] = blend_half(Lp, Ln, blend_norm(w, D), delta);
      float reach = 0.0f;
      for (int j = 0; j < D; j++) {
        const float A = blend_a(a[j], h[i], up[j]), C = blend_c(a[j], h[i], un[j]);
        reach = fmaxf(reach, fmaxf(fabsf(a[j] - A), fabsf(C - a[j])));
      }
      n_c[i] = h[i] > 0.0f ? blend_count(reach, resolution) : 0;
    }
    for (int j = 0; j < D; j++) up[j] = un[j];
    Lp = Ln;
  }
  return M;
}
#endif

}  // namespace
