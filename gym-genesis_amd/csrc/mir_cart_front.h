// mir_cart_front.h — the host-side checks of mir_cartesian_path and the rule of its targets (mir_cart.hip; include/mirigid.h, "Cartesian
// paths"): plain C++, no HIP in it, so that tests/cart_host.cpp builds it with g++ (`make cart-host`) and tests/test_cart_cpu.py walks
// every refusal and compares the sample counts and the interpolation with the NumPy rule without a device.  The kernel calls the same
// functions (CART_HD makes them device functions under hipcc), so what the test sees is the text the kernel runs; the library's sqrtf,
// atan2f, sinf and cosf differ between host and device within their documented few ulp.
// A refusal is `refuse(code, text)`: the caller's, which names the entry point.  The order of the checks and their texts are part of
// the interface.
#pragma once
#include <math.h>
#include <stdint.h>

#include "mirigid.h"

#ifdef __HIPCC__
#define CART_HD __host__ __device__ __forceinline__
#else
#define CART_HD static inline
#endif

namespace {

constexpr int CART_MAX_COUNT = 1 << 30;  // the samples of one segment are capped here: far above every max_points that fits a call

// what the entry point was handed, as far as these checks read it (the clearance side is checked by the planner's front end)
struct CartCall {
  bool handle;
  const MirCartQuery* q;
  const void *pq, *probes, *dof_qadr, *target_pos, *points, *n_points, *fraction, *status, *path;
};

static bool cart_positive(float v) { return isfinite(v) && v > 0.0f; }

template <class Refuse>
static int cart_check(const CartCall& c, Refuse refuse) {
  const MirCartQuery* const q = c.q;
  if (!c.handle || !q || !c.pq || !c.probes || !c.dof_qadr || !c.target_pos || !c.points || !c.n_points || !c.fraction || !c.status)
    return refuse(MIR_E_INVALID, "null argument");
  if (q->struct_size != (int32_t)sizeof(MirCartQuery)) return refuse(MIR_E_INVALID, "struct_size is not sizeof(MirCartQuery)");
  if (q->num_targets < 1) return refuse(MIR_E_INVALID, "num_targets < 1");
  if (q->max_points < 2) return refuse(MIR_E_INVALID, "max_points < 2");
  if (q->num_waypoints < 0 || q->num_waypoints == 1) return refuse(MIR_E_INVALID, "num_waypoints must be 0 or >= 2");
  if (q->num_waypoints >= 2 && !c.path) return refuse(MIR_E_INVALID, "num_waypoints >= 2 without path");
  if (q->num_waypoints == 0 && c.path) return refuse(MIR_E_INVALID, "path with num_waypoints == 0");
  if (q->flags) return refuse(MIR_E_INVALID, "unknown flag bit in MirCartQuery");
  if (!cart_positive(q->max_pos_step)) return refuse(MIR_E_INVALID, "max_pos_step must be finite and > 0");
  if (!cart_positive(q->max_rot_step)) return refuse(MIR_E_INVALID, "max_rot_step must be finite and > 0");
  if (!cart_positive(q->jump_threshold)) return refuse(MIR_E_INVALID, "jump_threshold must be finite and > 0");
  return MIR_OK;
}

// R x max(P, W) x D floats must be addressable by 31 bits (behind the planner's front end, which yields R and D)
template <class Refuse>
static int cart_check_size(const MirCartQuery* q, long long R, int D, Refuse refuse) {
  const long long per_row = (long long)(q->max_points > q->num_waypoints ? q->max_points : q->num_waypoints) * D;
  if (R > 0 && per_row > 0x7fffffffLL / R) return refuse(MIR_E_CAPACITY, "rows x max_points x n_dofs beyond 2^31 - 1");
  return MIR_OK;
}

// ---- the rule of the targets.  x / y with one refinement of the quotient: the division of the planner's edge rule (div_refined)
CART_HD float cart_div(float x, float y) {
  const float r = 1.0f / y;
  const float t = x * r;
  return fmaf(fmaf(-t, y, x), r, t);
}

CART_HD bool cart_finite(float x) { return fabsf(x) <= 3.4028234664e38f; }  // (false for a NaN)

// d = conj(a) b along the shorter arc (negated when d.w < 0; d.w == 0, the antipodal case, is left as it is: the half turn about
// +d.xyz), sn = |d.xyz|, ang = 2 atan2(sn, d.w) in [0, pi].  Quaternions are wxyz.
CART_HD void cart_delta(const float* a, const float* b, float* d, float* sn, float* ang) {
  float w = a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
  float x = a[0] * b[1] - a[1] * b[0] - a[2] * b[3] + a[3] * b[2];
  float y = a[0] * b[2] + a[1] * b[3] - a[2] * b[0] - a[3] * b[1];
  float z = a[0] * b[3] - a[1] * b[2] + a[2] * b[1] - a[3] * b[0];
  if (w < 0.0f) { w = -w; x = -x; y = -y; z = -z; }
  d[0] = w; d[1] = x; d[2] = y; d[3] = z;
  *sn = sqrtf(x * x + y * y + z * z);
  *ang = 2.0f * atan2f(*sn, w);
}

// the samples of a segment of length dp (metres) and angle ang (radians): max(1, ceil(max(dp / max_pos_step, ang / max_rot_step))), at
// most CART_MAX_COUNT; a quotient that is not finite counts as CART_MAX_COUNT
CART_HD int cart_count(float dp, float ang, float max_pos_step, float max_rot_step) {
  const float cp = cart_div(dp, max_pos_step), cr = cart_div(ang, max_rot_step);
  if (!cart_finite(cp) || !cart_finite(cr)) return CART_MAX_COUNT;  // (asked first: fmaxf would drop a NaN)
  const float c = fmaxf(cp, cr);
  if (c <= 1.0f) return 1;
  return c < (float)CART_MAX_COUNT ? (int)ceilf(c) : CART_MAX_COUNT;
}

// the target of sample i = 1 .. n of the segment (pa, qa) -> (pb, qb) with (d, sn, ang) = cart_delta(qa, qb): the end's own bits at
// i == n; else t = i / n (refined), p = pa + t (pb - pa), q = qa (cos h, sin h d.xyz / sn) with h = t ang / 2 -- qa itself when
// sn <= 1e-9 (the zero-angle case).  userot false: q is not written.
CART_HD void cart_target(const float* pa, const float* pb, const float* qa, const float* qb, const float* d, float sn, float ang, int i, int n,
                         bool userot, float* p, float* q) {
  if (i == n) {
    for (int k = 0; k < 3; k++) p[k] = pb[k];
    if (userot) for (int k = 0; k < 4; k++) q[k] = qb[k];
    return;
  }
  const float t = cart_div((float)i, (float)n);
  for (int k = 0; k < 3; k++) p[k] = pa[k] + t * (pb[k] - pa[k]);
  if (!userot) return;
  if (!(sn > 1e-9f)) {
    for (int k = 0; k < 4; k++) q[k] = qa[k];
    return;
  }
  const float h = 0.5f * (t * ang), s = sinf(h) / sn, w = cosf(h);
  const float x = s * d[1], y = s * d[2], z = s * d[3];
  q[0] = qa[0] * w - qa[1] * x - qa[2] * y - qa[3] * z;
  q[1] = qa[0] * x + qa[1] * w + qa[2] * z - qa[3] * y;
  q[2] = qa[0] * y - qa[1] * z + qa[2] * w + qa[3] * x;
  q[3] = qa[0] * z + qa[1] * y - qa[2] * x + qa[3] * w;
}

// waypoint w of W over n_points >= 2 dense points, 0 < w < W - 1: the index i0 <= n_points - 2 of the left neighbour and the weight t
// of the right one, u = (w / (W - 1)) (n_points - 1), i0 = min(floor(u), n_points - 2), t = u - i0
CART_HD void cart_waypoint(int w, int W, int n_points, int* i0, float* t) {
  const float u = cart_div((float)w, (float)(W - 1)) * (float)(n_points - 1);
  int i = (int)u;
  if (i > n_points - 2) i = n_points - 2;
  *i0 = i;
  *t = u - (float)i;
}

}  // namespace
