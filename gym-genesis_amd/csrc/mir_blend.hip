// mir_blend.hip — batched collision-checked corner blending (mir_blend_path); include/mirigid.h and DESIGN.md, "Corner blending".
//
// What it serves: the step between plan_path / plan_cartesian_path and retime_path.  For a list of envs, one launch replaces each
// interior corner of each row's joint-space polyline by a quadratic Bezier blend within max_deviation of the corner, checks the blend
// with the planner's clear(q), halves a blocked blend, and writes the smoothed path as dense points (and, resampled at equal arc
// length, as waypoints).
//
// Mapping: one workgroup of one wave64 per row, as mir_plan.hip and mir_cart.hip, whose row machinery (mir_plan_row.h: PlanRow<SELF,
// CARRY>, plan_setup) is the collision half unchanged: clear(q) with lane = body in the forward kinematics and lane = probe in the
// distance tests.  Lane j < D holds dof j of everything else: the kept nodes (PlanLds::poly, column j written and read by lane j), the
// segment in front of the corner and the one behind it, A, Q_i and C.  A norm over the dofs is PlanRow::norm2 (j ascending through LDS).
//   The scalar part of the rule is mir_blend_front.h, which the CPU tests build with g++.
//   Points go straight to global memory, column j by lane j; the waypoints are resampled from the row's own points by the lanes that
//   wrote them, with the cumulative length streamed (two passes over the points) so that P is not bounded by LDS.
//   PlanLds::cum holds the accepted half-length per kept node; two 64-bit masks (wave-uniform) say which input nodes were kept.
// Bounds: K <= MIR_PLAN_MAX_POLY, m, max_shrinks + 1, the 4096 samples of a check, P, W.  The point count is bounded by 2 + (M - 2)(m +
//   1) <= P, which is decided before a point is written.
// Stores: plain dword stores by lanes 0 .. D-1 (points, path), by every lane (blend_len) or by lane 0.  No atomics, no scratch, no
//   cross-wave barrier.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <cstring>

#include "mir_model.h"
#include "mir_model64.h"
#include "mir_scene.h"

#define G 16
#include "mir_dev.h"

#include "mir_query.h"
#include "mir_sphere_front.h"  // (brings mir_dist_body.h)

#include "mir_self_body.h"

#include "mir_plan_row.h"

#include "mir_blend_front.h"

namespace {

struct BlendArgs {
  PlanArgs p;  // the clearance side, as mir_path_clearance fills it
  int K, P, W, m, shrinks;
  float delta;
  const float* poly;
  const int32_t* n_poly;
  float *points, *path, *blend_len;
  int32_t *n_points, *status, *stats;
};
static_assert(sizeof(BlendArgs) <= 4096, "kernel arguments");

extern __shared__ float blend_dyn[];

// the dense points of a row: column j by lane j, a point whose bits equal the point before is not emitted
struct BlendOut {
  float* out;
  int D, lane, np;
  float last;
  __device__ __forceinline__ void emit(float v) {
    const bool isd = lane < D;
    if (np > 0 && __ballot(isd && __float_as_uint(v) != __float_as_uint(last)) == 0ull) return;
    if (isd) out[(size_t)np * D + lane] = v;
    np++;
    last = v;
  }
};

template <bool SELF, bool CARRY>
__global__ __launch_bounds__(64) void mir_blend_kernel(BlendArgs a) {
  __shared__ PlanLds L;
  const int lane = threadIdx.x, row = blockIdx.x, D = a.p.D;
  PlanRow<SELF, CARRY> r{a.p, L, lane, 0, 0, false, blend_dyn, SELF_LIST};
  plan_setup(r, row, sphere_row_env(a.p.r, row));
  const bool isd = lane < D;

  // ---- 1. compaction: the kept nodes into LDS (lane j: column j), which input nodes they were, finiteness
  const float* const in = a.poly + (size_t)row * a.K * D;
  const int nv = blend_valid(a.n_poly ? a.n_poly[row] : a.K, a.K);
  const float first = isd ? in[lane] : 0.0f;
  unsigned long long kept[2] = {0ull, 0ull};
  int M = 0;
  bool notfinite = false;
  for (int k = 0; k < nv; k++) {
    const float v = isd ? in[(size_t)k * D + lane] : 0.0f;
    notfinite = notfinite || __ballot(isd && !blend_finite(v)) != 0ull;
    const bool differs = isd && (M == 0 || !(v == L.poly[M - 1][lane]));
    if (__ballot(differs) == 0ull) continue;
    if (isd) L.poly[M][lane] = v;
    kept[k >> 6] |= 1ull << (k & 63);
    M++;
  }
  for (int k = lane; k < MIR_PLAN_MAX_POLY; k += 64) L.cum[k] = 0.0f;  // the accepted half-length per kept node
  WSYNC();

  float* const out = a.points + (size_t)row * a.P * D;
  BlendOut o{out, D, lane, 0, first};
  int status = MIR_PLAN_OK, blended = 0, sharp = 0;
  if (notfinite) status = MIR_BLEND_NOT_FINITE;
  else if (M == 1) status = MIR_BLEND_NO_MOTION;
  else if (blend_worst_points(M, a.m) > (long long)a.P) status = MIR_BLEND_TOO_MANY_POINTS;
  else if (!a.p.ignore && !(r.clearance(first) >= a.p.margin)) status = MIR_PLAN_START_IN_COLLISION;
  else if (SELF && !a.p.ignore && !(r.self_clearance() >= a.p.self_margin)) status = MIR_PLAN_START_IN_SELF_COLLISION;
  o.emit(first);
  if (status == MIR_PLAN_OK) {
    // ---- 3. - 8. corner by corner; (Lp, up): the segment in front of the corner
    float qi = isd ? L.poly[1][lane] : 0.0f;
    float Lp, up;
    {
      const float d = qi - first;
      Lp = sqrtf(r.norm2(isd ? d : 0.0f));
      up = blend_unit(d, Lp);
    }
    for (int i = 1; i + 1 < M; i++) {
      const float qn = isd ? L.poly[i + 1][lane] : 0.0f;
      const float d = qn - qi;
      const float Ln = sqrtf(r.norm2(isd ? d : 0.0f));
      const float un = blend_unit(d, Ln);
      const float du = sqrtf(r.norm2(isd ? un - up : 0.0f));
      float h = blend_half(Lp, Ln, du, a.delta);
      float A = qi, C = qi;
      if (h > 0.0f) {
        for (int t = 0;; t++) {
          A = blend_a(qi, h, up);
          C = blend_c(qi, h, un);
          bool blocked = false;
          if (!a.p.ignore) {
            const float reach = wave_max(isd ? fmaxf(fabsf(qi - A), fabsf(C - qi)) : 0.0f);
            const int nc = __builtin_amdgcn_readfirstlane(blend_count(reach, a.p.resolution));
            for (int k = 0; k <= nc && !blocked; k++) blocked = !r.clear(blend_curve(A, qi, C, blend_param(k, nc)));
          }
          if (!blocked) break;
          if (t == a.shrinks) { h = 0.0f; break; }
          h = 0.5f * h;
          if (!(h > 0.0f)) break;  // (halved into nothing)
        }
      }
      if (h > 0.0f) {
        blended++;
        if (lane == 0) L.cum[i] = h;
        for (int k = 0; k <= a.m; k++) o.emit(blend_curve(A, qi, C, blend_param(k, a.m)));
      } else {
        sharp++;
        o.emit(qi);
      }
      qi = qn; Lp = Ln; up = un;
    }
    o.emit(qi);  // Q_{M-1}
  }
  const int np = o.np;
  const float last = o.last;
  WSYNC();

  // ---- the tail repeats the last point
  for (int k = np; k < a.P; k++)
    if (isd) out[(size_t)k * D + lane] = last;
  // ---- 9. waypoints: step 7 of mir_plan_path on the dense points (every lane reads the column it wrote), the cumulative length streamed
  if (a.path) {
    float* const wp = a.path + (size_t)row * a.W * D;
    const auto pt = [&](int k) { return isd ? out[(size_t)k * D + lane] : 0.0f; };
    const auto len = [&](int k) { return sqrtf(r.norm2(pt(k + 1) - pt(k))); };
    float total = 0.0f;
    if (np > 2)
      for (int k = 0; k + 1 < np; k++) total = total + len(k);
    int k = 0;
    float c0 = 0.0f, c1 = np > 2 ? 0.0f + len(0) : 0.0f;
    for (int w = 0; w < a.W; w++) {
      float v;
      if (np == 1 || w == 0) v = first;
      else if (w == a.W - 1) v = last;
      else {
        const float f = div_refined((float)w, (float)(a.W - 1));
        float t = f;  // (one segment: the fraction itself, no length enters)
        if (np > 2) {
          const float s = f * total;
          while (k < np - 2 && c1 <= s) {
            k++;
            c0 = c1;
            c1 = c0 + len(k);
          }
          const float ln = c1 - c0;
          t = ln > 0.0f ? fminf(div_refined(s - c0, ln), 1.0f) : 0.0f;
        }
        const float p0 = pt(k), p1 = pt(k + 1);
        const float e = p1 - p0;
        const float se = t * e;
        v = p0 + se;
      }
      if (isd) wp[(size_t)w * D + lane] = v;
    }
  }
  // ---- the accepted half-length at each INPUT node: the rank of a kept node among the kept ones indexes PlanLds::cum
  if (a.blend_len) {
    float* const bl = a.blend_len + (size_t)row * MIR_PLAN_MAX_POLY;
    for (int k = lane; k < MIR_PLAN_MAX_POLY; k += 64) {
      const int w = k >> 6, b = k & 63;
      const bool is_kept = (kept[w] >> b) & 1ull;
      const int rank = (w ? __popcll(kept[0]) : 0) + __popcll(kept[w] & ((1ull << b) - 1ull));
      bl[k] = is_kept && status == MIR_PLAN_OK ? L.cum[rank] : 0.0f;
    }
  }
  if (lane == 0) {
    a.status[row] = status;
    a.n_points[row] = np;
    if (a.stats) {
      int32_t* const st = a.stats + (size_t)row * 4;
      st[0] = M; st[1] = blended; st[2] = sharp; st[3] = r.checked;
    }
  }
}

}  // namespace

extern "C" int mir_blend_query_sizeof(void) { return (int)sizeof(MirBlendQuery); }

extern "C" int mir_blend_path(MirHandle h, const MirBlendQuery* q, const MirPlanQuery* pq, const MirSelfQuery* sq, const MirCarryQuery* cq,
                              const float* probes, const int32_t* probe_link, const int32_t* dof_qadr, const int64_t* env_idx, int32_t n_rows,
                              const float* qpos_start, const float* poly, const int32_t* n_poly, float* points, int32_t* n_points, int32_t* status,
                              float* path, float* blend_len, int32_t* stats, void* stream) {
  const char* const who = "mir_blend_path";
  const auto refuse = [&](int code, const char* what) { return query_error(code, who, what); };
  const BlendCall bc{h != nullptr, q, pq, probes, dof_qadr, poly, points, n_points, status, path};
  int rc;
  if ((rc = blend_check(bc, refuse)) != MIR_OK) return rc;
  const PlanCall c = plan_call(who, h, pq, sq, sq != nullptr, cq, cq != nullptr, probes, probe_link, dof_qadr, env_idx, n_rows, qpos_start, nullptr,
                               nullptr, stream);
  BlendArgs a;
  memset(&a, 0, sizeof a);
  long long R = 0;
  if ((rc = plan_front(c, false, a.p, R)) != MIR_OK) return rc;
  if ((rc = blend_check_size(q, R, pq->n_dofs, refuse)) != MIR_OK) return rc;
  if (R == 0) return MIR_OK;
  a.K = q->num_nodes; a.P = q->max_points; a.W = q->num_waypoints; a.m = q->blend_points; a.shrinks = q->max_shrinks;
  a.delta = q->max_deviation;
  a.poly = poly; a.n_poly = n_poly;
  a.points = points; a.path = path; a.blend_len = blend_len; a.n_points = n_points; a.status = status; a.stats = stats;
  const auto kernel = pick_self_carry(c.self, c.carry, [](auto S, auto C) { return mir_blend_kernel<decltype(S)::value, decltype(C)::value>; });
  return plan_launch(c, kernel, R, a, a.p, 0);
}
