// mir_opt_front.h — the host-side checks of mir_optimize_path and the scalar part of its rule (mir_opt.hip; include/mirigid.h,
// "trajectory optimisation"): plain C++, no HIP in it, so that tests/opt_host.cpp builds it with g++ (`make opt-host`) and
// tests/test_opt_cpu.py walks every refusal and compares the constants, c and c', the Thomas recurrence, the cost and gradient
// assembly and the decisions of the line search with the NumPy port bit for bit, without a device.  The kernel calls the same scalar
// functions (OPT_HD makes them device functions under hipcc) with a dof per lane; opt_solve_column() below is the recurrence over one
// column, for the host.
// One statement per rounding: under -ffp-contract=on nothing is fused that the port does not fuse (the two fmas of opt_div are its own).
// A refusal is `refuse(code, text)`: the caller's, which names the entry point.  The order of the checks and their texts are part of
// the interface.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "mirigid.h"

#ifdef __HIPCC__
#define OPT_HD __host__ __device__ __forceinline__
#else
#define OPT_HD static inline
#endif

namespace {

// what the entry point was handed, as far as these checks read it (the clearance side is checked by the planner's front end)
struct OptCall {
  bool handle;
  const MirOptQuery* q;
  const MirPlanQuery* pq;
  const void *probes, *dof_qadr, *paths, *path_out, *status;
  int32_t K;
};

static inline bool opt_host_finite(float x) { return fabsf(x) <= 3.4028234664e38f; }  // (false for a NaN)

template <class Refuse>
static int opt_check(const OptCall& c, Refuse refuse) {
  const MirOptQuery* const q = c.q;
  if (!c.handle || !q || !c.pq || !c.probes || !c.dof_qadr || !c.paths || !c.path_out || !c.status) return refuse(MIR_E_INVALID, "null argument");
  if (q->struct_size != (int32_t)sizeof(MirOptQuery)) return refuse(MIR_E_INVALID, "struct_size is not sizeof(MirOptQuery)");
  if (q->num_waypoints < 3 || q->num_waypoints > MIR_PLAN_MAX_POLY) return refuse(MIR_E_INVALID, "num_waypoints outside 3 .. MIR_PLAN_MAX_POLY");
  if (c.K != q->num_waypoints) return refuse(MIR_E_INVALID, "K is not num_waypoints");
  if (q->flags) return refuse(MIR_E_INVALID, "unknown flag bit in MirOptQuery");
  if (!opt_host_finite(q->smooth_weight) || !opt_host_finite(q->obstacle_weight) || !opt_host_finite(q->step) || !opt_host_finite(q->activation) ||
      !opt_host_finite(q->ftol))
    return refuse(MIR_E_INVALID, "a weight, step, activation or ftol is not finite");
  if (!(q->smooth_weight > 0.0f)) return refuse(MIR_E_INVALID, "smooth_weight must be > 0");
  if (!(q->obstacle_weight >= 0.0f)) return refuse(MIR_E_INVALID, "obstacle_weight must be >= 0");
  if (!(q->step > 0.0f)) return refuse(MIR_E_INVALID, "step must be > 0");
  if (!(q->activation > 0.0f)) return refuse(MIR_E_INVALID, "activation must be > 0");
  if (!(q->ftol >= 0.0f)) return refuse(MIR_E_INVALID, "ftol must be >= 0");
  if (q->max_iterations < 0 || q->max_halvings < 0) return refuse(MIR_E_INVALID, "negative max_iterations or max_halvings");
  return MIR_OK;
}

// behind the planner's front end (which has checked margin and max_distance on their own): the obstacle cost must see its whole band
template <class Refuse>
static int opt_check_band(const MirOptQuery* q, const MirPlanQuery* pq, Refuse refuse) {
  if ((double)pq->max_distance < (double)pq->margin + (double)q->activation) return refuse(MIR_E_INVALID, "max_distance < margin + activation");
  return MIR_OK;
}

// the LDS of a row: the fixed part (the planner's PlanLds and the axis and anchor of every planned dof: mir_opt.hip asserts the sum),
// three K x 16 buffers, the sphere list of the self test
constexpr size_t OPT_FIXED_LDS = 14368;
template <class Refuse>
static int opt_check_lds(int K, long long NS, bool self, Refuse refuse) {
  if (OPT_FIXED_LDS + (size_t)3 * (size_t)K * 64 + (self ? 16 * (size_t)NS : 0) > 65536)
    return refuse(MIR_E_CAPACITY, "the path and gradient buffers and the sphere list do not fit 64 KB of LDS (num_waypoints, n_probes + n_extra)");
  return MIR_OK;
}

// ---- the constants of a call, rounded once from double.  rpiv holds r_i = i / (i + 1) at index i - 1, i = 1 .. K - 2
struct OptConsts {
  float km1, hk, ik;
  float rpiv[MIR_PLAN_MAX_POLY];
};
static void opt_consts(int K, OptConsts& c) {
  c.km1 = (float)(double)(K - 1);
  c.hk = (float)(0.5 * (double)(K - 1));
  c.ik = (float)(1.0 / (double)(K - 1));
  for (int i = 1; i <= MIR_PLAN_MAX_POLY; i++) c.rpiv[i - 1] = i <= K - 2 ? (float)((double)i / (double)(i + 1)) : 0.0f;
}

// ---- the rule.  x / y with one refinement of the quotient: the division of the planner's edge rule (div_refined)
OPT_HD float opt_div(float x, float y) {
  const float r = 1.0f / y;
  const float t = x * r;
  return fmaf(fmaf(-t, y, x), r, t);
}

OPT_HD bool opt_finite(float x) { return fabsf(x) <= 3.4028234664e38f; }  // (false for a NaN)

// c(d) and c'(d) of a probe that counts
OPT_HD float opt_c(float d, float eps) {
  if (d < 0.0f) {
    const float h = 0.5f * eps;
    return h - d;
  }
  if (d <= eps) {
    const float t = d - eps;
    const float t2 = t * t;
    const float den = eps + eps;
    return opt_div(t2, den);
  }
  return 0.0f;
}
OPT_HD float opt_dc(float d, float eps) {
  if (d < 0.0f) return -1.0f;
  if (d <= eps) {
    const float t = d - eps;
    return opt_div(t, eps);
  }
  return 0.0f;
}

// one term of a dof's share of S
OPT_HD float opt_s_add(float acc, float q_next, float q) {
  const float e = q_next - q;
  const float e2 = e * e;
  return acc + e2;
}
// U = (w_s S) + (w_o O) with S = hk ss and O = ik oo
OPT_HD float opt_S(float hk, float ss) { return hk * ss; }
OPT_HD float opt_O(float ik, float oo) { return ik * oo; }
OPT_HD float opt_U(float ws, float S, float wo, float O) {
  const float a = ws * S;
  const float b = wo * O;
  return a + b;
}
// g_ij from the three waypoints and the probe sum of 3.
OPT_HD float opt_grad(float q_prev, float q, float q_next, float gsum_ij, float ws, float wo, float km1, float ik) {
  const float two = q + q;
  const float a = two - q_prev;
  const float b = a - q_next;
  const float sm = km1 * b;
  const float t1 = ws * sm;
  const float go = ik * gsum_ij;
  const float t2 = wo * go;
  return t1 + t2;
}
// the Thomas recurrence on tridiag(-1, 2, -1): forward y_i from g_i and y_{i-1}, backward x_i from y_i and x_{i+1}
OPT_HD float opt_forward(float g, float r_prev, float y_prev) {
  const float t = r_prev * y_prev;
  return g + t;
}
OPT_HD float opt_backward(float y, float x_next, float r) {
  const float s = y + x_next;
  return r * s;
}
// the candidate of one value: q - alpha (ik x)
OPT_HD float opt_candidate(float q, float x, float ik, float alpha) {
  const float delta = ik * x;
  const float s = alpha * delta;
  return q - s;
}
OPT_HD bool opt_outside(float q, float lo, float hi) { return !(q >= lo && q <= hi); }
// the line search's acceptance and the stop test of an accepted step
OPT_HD bool opt_accept(float U_new, float U) { return opt_finite(U_new) && U_new < U; }
OPT_HD bool opt_converged(float U, float U_new, float ftol) {
  const float dec = U - U_new;
  const float thr = ftol * U;
  return dec < thr;
}

#ifndef __HIPCC__
// ---- the candidate of one column (one dof) of n interior values, for the host: g (n), q (n) -> out (n)
static void opt_solve_column(const float* g, const float* q, int n, const OptConsts& c, float alpha, float* out) {
  float y = 0.0f;
  for (int i = 1; i <= n; i++) {
    y = i == 1 ? g[0] : opt_forward(g[i - 1], c.rpiv[i - 2], y);
    out[i - 1] = y;
  }
  float x = 0.0f;
  for (int i = n; i >= 1; i--) {
    x = opt_backward(out[i - 1], i == n ? 0.0f : x, c.rpiv[i - 1]);
    out[i - 1] = x;
  }
  for (int i = 0; i < n; i++) out[i] = opt_candidate(q[i], out[i], c.ik, alpha);
}
#endif

}  // namespace
