// mir_retime.hip — batched time parameterisation of joint paths (mir_retime_path); include/mirigid.h and DESIGN.md, "Time
// parameterisation": TOPP-RA with the interpolation collocation scheme on the caller's waypoints, steps 1 - 9 of the header.
//
// Mapping: one workgroup of one wave64 per row.  WSYNC() only; nothing travels from lane to lane through global memory.
//   Compaction.  Lane = waypoint in chunks of 64: a waypoint is kept when a value differs from the waypoint in front of it (equality is
//   transitive on finite values, and a row with a value that is not finite ends before it matters); a ballot and a population count
//   place the kept ones.  The kept waypoints' indices (16 bits each), Kmax / x (one array: the forward pass overwrites Kmax_i by x_i
//   once it has read it) and t live in LDS: 20 KB.
//   An interval's LP.  Lane = one of its <= 64 rows: lanes 0 .. D+E-1 the rows of gridpoint i, lanes D+E .. 2(D+E)-1 those of gridpoint
//   i+1 at (x + 2u, u).  A lane takes its coefficients from the three neighbouring kept waypoints of its dof (global: they stream
//   through L2 twice, once per pass; the loads of the next interval are issued before the bisection of this one) or from its extra
//   row, and turns them into bounds on u that are linear in x: p - r x <= u <= q - r x.  "Is there a u at x" is a wave maximum, a wave
//   minimum and a ballot (the rows with alpha == 0, which bound x alone).  A bound that is not a number (a row whose alpha is so small that its
//   quotients overflow) is passed over by the minimum and the maximum.
//   The two sequential passes are the chain: M - 2 bisections of 32 halvings backward, M - 1 minima forward.
//   Sampling.  The lanes stride over the T samples, each with a binary search over t in LDS (<= 11 steps).
// The arithmetic is written one rounding per operation, in the order of tests/retime_ref.py (no a * b + c in one expression: the
// build contracts those), so that the float32 port of the reference differs from this kernel by the division and the square root only.
// Bounds: every loop is bounded by K, M * E, T, 32 or 12.  Stores: plain dword stores.  No atomics, no scratch, no cross-wave barrier.
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
#include "mir_retime_front.h"

namespace {

constexpr int RETIME_BISECT = 32;

struct RetimeArgs {
  const float* paths;                // (R, K, D)
  const float *ea, *eb, *elo, *ehi;  // (R, K, E)
  float *x, *t, *duration;
  int32_t *status, *n_samples;
  float *samples, *sample_vel;  // (R, T, D), nullable
  int K, D, E, T;
  float dt, vs2;  // vs2: max_path_speed^2
  float vmax[RETIME_MAX_DOF], amax[RETIME_MAX_DOF];
};

// ---- wave reductions, the same value in every lane: the 16-lane row by DPP, the four rows by v_readlane.  A NaN is passed over.
__device__ __forceinline__ float retime_lane(float v, int l) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l)); }
__device__ __forceinline__ float retime_wave_max(float v) {
  v = gmaxf(v);
  return fmaxf(fmaxf(retime_lane(v, 0), retime_lane(v, 16)), fmaxf(retime_lane(v, 32), retime_lane(v, 48)));
}
__device__ __forceinline__ float retime_wave_min(float v) {
  v = fminf(v, row_ror<1>(v));
  v = fminf(v, row_ror<2>(v));
  v = fminf(v, row_ror<4>(v));
  v = fminf(v, row_ror<8>(v));
  return fminf(fminf(retime_lane(v, 0), retime_lane(v, 16)), fminf(retime_lane(v, 32), retime_lane(v, 48)));
}

// a lane's row of an interval's LP as it is given (4. and 5.), with the lane's share of the speed cap (3.) ...
struct RetimeRow { float al, be, lo, hi, cap; };
// ... and as bounds on u that are linear in x (xo: alpha == 0, the row bounds x alone)
struct RetimeBounds { float p, q, r, be, lo, hi; bool xo; };

__device__ __forceinline__ RetimeBounds retime_bounds(const RetimeRow& w) {
  const bool nz = w.al != 0.0f, pos = w.al > 0.0f;
  RetimeBounds z;
  z.p = nz ? (pos ? w.lo : w.hi) / w.al : -INFINITY;
  z.q = nz ? (pos ? w.hi : w.lo) / w.al : INFINITY;
  z.r = nz ? w.be / w.al : 0.0f;
  z.be = w.be; z.lo = w.lo; z.hi = w.hi; z.xo = !nz;
  return z;
}

// is there a u at x under 5. (kn: Kmax of the next gridpoint)?  The same answer in every lane.
__device__ __forceinline__ bool retime_feasible(const RetimeBounds& z, float x, float kn) {
  const float rx = z.r * x;
  const float low = z.p - rx, up = z.q - rx;
  const float rest = kn - x;
  const float L = fmaxf(retime_wave_max(low), -0.5f * x), U = fminf(retime_wave_min(up), 0.5f * rest);
  const float bx = z.be * x;
  const bool out = z.xo && !(z.lo <= bx && bx <= z.hi);
  return L <= U && __ballot(out) == 0ull;
}

__global__ __launch_bounds__(64) void mir_retime_kernel(RetimeArgs a) {
  __shared__ float sx[MIR_RETIME_MAX_WAYPOINTS], st[MIR_RETIME_MAX_WAYPOINTS];
  __shared__ uint16_t skept[MIR_RETIME_MAX_WAYPOINTS];
  const int lane = threadIdx.x, row = blockIdx.x, K = a.K, D = a.D, E = a.E, n = D + E;
  const float* const P = a.paths + (size_t)row * K * D;

  // ---- 1. compaction; the values that are not finite
  int M = 0;
  bool nf = false;
  for (int base = 0; base < K; base += 64) {
    const int k = base + lane;
    const bool valid = k < K;
    bool keep = valid && k == 0, bad = false;
    if (valid)
      for (int j = 0; j < D; j++) {
        const float v = P[k * D + j];
        bad = bad || nonfinite(v);
        if (k > 0) keep = keep || v != P[(k - 1) * D + j];
      }
    const unsigned long long mask = __ballot(keep);
    nf = nf || __ballot(bad) != 0ull;
    if (keep) skept[M + __popcll(mask & ((1ull << lane) - 1ull))] = (uint16_t)k;
    M += __popcll(mask);
  }
  if (lane == 0) { sx[0] = 0.0f; st[0] = 0.0f; }
  WSYNC();
  bool esign = false;
  if (E > 0 && !nf) {
    bool ebad = false;
    for (int idx = lane; idx < M * E; idx += 64) {
      const int i = idx / E, e = idx - i * E;
      const size_t off = ((size_t)row * K + skept[i]) * E + e;
      const float va = a.ea[off], vb = a.eb[off], vl = a.elo[off], vh = a.ehi[off];
      ebad = ebad || nonfinite(va) || nonfinite(vb) || nonfinite(vl) || nonfinite(vh);
      esign = esign || !(vl < 0.0f && vh > 0.0f);
    }
    nf = __ballot(ebad) != 0ull;
    esign = __ballot(esign) != 0ull;
  }
  int status = MIR_RETIME_OK;
  if (nf) status = MIR_RETIME_NOT_FINITE;
  else if (M == 1) status = MIR_RETIME_NO_MOTION;
  else if (M == 2) status = MIR_RETIME_TOO_FEW_WAYPOINTS;
  else if (esign) status = MIR_RETIME_INFEASIBLE;

  float duration = 0.0f;
  if (status == MIR_RETIME_OK) {
    // ---- the row of interval i this lane holds: lanes 0 .. n-1 gridpoint i, lanes n .. 2n-1 gridpoint i + 1
    const int side = lane >= n ? 1 : 0, r = lane - side * n;
    const bool isrow = lane < 2 * n, isacc = isrow && r < D;
    const float amax = isacc ? a.amax[r] : 0.0f, vmax = isacc ? a.vmax[r] : 0.0f;
    auto load_row = [&](int i) {
      RetimeRow w{0.0f, 0.0f, -INFINITY, INFINITY, INFINITY};  // (a lane without a row: alpha = beta = 0 bounds nothing)
      if (isrow) {
        const int g = i + side, kg = skept[g];
        if (isacc) {
          const float qg = P[kg * D + r];
          const float dp = g > 0 ? qg - P[(int)skept[g - 1] * D + r] : 0.0f;
          const float dn = g < M - 1 ? P[(int)skept[g + 1] * D + r] - qg : 0.0f;
          const bool inner = g > 0 && g < M - 1;
          const float dsum = dn + dp;
          w.al = inner ? dsum * 0.5f : dsum;  // (an end: the other difference is 0)
          w.be = inner ? dn - dp : 0.0f;
          w.lo = -amax; w.hi = amax;
          if (dp != 0.0f) { const float rr = vmax / fabsf(dp); w.cap = rr * rr; }
          if (dn != 0.0f) { const float rr = vmax / fabsf(dn); w.cap = fminf(w.cap, rr * rr); }
        } else {
          const size_t off = ((size_t)row * K + kg) * E + (r - D);
          w.al = a.ea[off]; w.be = a.eb[off]; w.lo = a.elo[off]; w.hi = a.ehi[off];
        }
        if (side) {
          const float b2 = 2.0f * w.be;
          w.al = w.al + b2;
          w.cap = INFINITY;  // (the cap of gridpoint i is the left lanes')
        }
      }
      return w;
    };

    // ---- 6. backward: Kmax_i into sx[i]
    if (lane == 0) sx[M - 1] = 0.0f;
    float kn = 0.0f;
    RetimeRow nxt = load_row(M - 2);
    for (int i = M - 2; i >= 1; i--) {
      const RetimeRow w = nxt;
      if (i > 1) nxt = load_row(i - 1);
      const float cap = fminf(a.vs2, retime_wave_min(w.cap));
      const RetimeBounds z = retime_bounds(w);
      float k = cap;
      if (!retime_feasible(z, cap, kn)) {
        float lo = 0.0f, hi = cap;
        for (int it = 0; it < RETIME_BISECT; it++) {
          const float mid = 0.5f * (lo + hi);
          if (retime_feasible(z, mid, kn)) lo = mid;
          else hi = mid;
        }
        k = lo;
      }
      if (lane == 0) sx[i] = k;
      kn = k;
    }
    WSYNC();

    // ---- 7. forward: x_i into sx[i]; 8. t_i into st[i]
    float xi = 0.0f, ti = 0.0f;
    nxt = load_row(0);
    for (int i = 0; i < M - 1; i++) {
      const RetimeRow w = nxt;
      if (i + 1 < M - 1) nxt = load_row(i + 1);
      const RetimeBounds z = retime_bounds(w);
      const float kmax = sx[i + 1];
      const float rx = z.r * xi;
      const float up = z.q - rx;
      const float rest = kmax - xi;
      float u = fminf(retime_wave_min(up), 0.5f * rest);
      u = fmaxf(u, -0.5f * xi);
      const float u2 = 2.0f * u;
      float xn = fmaxf(xi + u2, 0.0f);
      if (i + 1 == M - 1) xn = 0.0f;
      const float den = sqrtf(xi) + sqrtf(xn);
      if (!(den > 0.0f)) { status = MIR_RETIME_INFEASIBLE; break; }
      const float step = 2.0f / den;
      ti = ti + step;
      WSYNC();  // (every lane has read Kmax_{i+1})
      if (lane == 0) { sx[i + 1] = xn; st[i + 1] = ti; }
      xi = xn;
    }
    WSYNC();
    if (status == MIR_RETIME_OK) duration = ti;
  }

  // ---- x and t in the caller's indexing; 9. the samples
  const bool timed = status == MIR_RETIME_OK;
  float* const xo = a.x + (size_t)row * K;
  float* const to = a.t + (size_t)row * K;
  if (timed) {
    for (int i = lane; i < M; i += 64) {
      const int k1 = i + 1 < M ? (int)skept[i + 1] : K;
      const float xv = sx[i], tv = st[i];
      for (int k = skept[i]; k < k1; k++) { xo[k] = xv; to[k] = tv; }
    }
  } else {
    for (int k = lane; k < K; k += 64) { xo[k] = 0.0f; to[k] = 0.0f; }
  }
  int ns = 1;
  if (timed) ns = (int)fminf(ceilf(duration / a.dt), 2.0e9f) + 1;
  const bool sampled = a.samples || a.sample_vel;
  if (timed && sampled && ns > a.T) status = MIR_RETIME_TRUNCATED;
  if (lane == 0) {
    a.duration[row] = duration;
    a.status[row] = status;
    a.n_samples[row] = ns;
  }
  if (!sampled) return;
  const bool still = !timed && status != MIR_RETIME_NO_MOTION;  // a failed row: P_0 everywhere
  for (int s = lane; s < a.T; s += 64) {
    const float tau = (float)s * a.dt;
    int k0 = 0, k1 = 0;  // the sample is Q0 + f (Q1 - Q0) of the caller's waypoints k0, k1; k1 == k0: the bits of k0
    float f = 0.0f, speed = 0.0f;
    if (!still && s > 0) {
      if (!(tau < duration)) k0 = k1 = K - 1;
      else {
        int lo = 0, hi = M - 1;  // st[lo] <= tau < st[hi]
        for (int it = 0; it < 12 && hi - lo > 1; it++) {
          const int mid = (lo + hi) >> 1;
          if (st[mid] <= tau) lo = mid;
          else hi = mid;
        }
        const float delta = tau - st[lo];
        const float x0 = sx[lo], x1 = sx[lo + 1];
        const float s0 = sqrtf(x0), u = (x1 - x0) * 0.5f;
        const float ud = u * delta;
        const float lin = s0 * delta, quad = (ud * delta) * 0.5f;
        f = fminf(fmaxf(lin + quad, 0.0f), 1.0f);
        speed = s0 + ud;
        k0 = skept[lo]; k1 = skept[lo + 1];
      }
    }
    const size_t o = ((size_t)row * a.T + s) * D;
    for (int j = 0; j < D; j++) {
      const float q0 = P[k0 * D + j];
      float q = q0, v = 0.0f;
      if (k1 != k0) {
        const float di = P[k1 * D + j] - q0;
        const float fd = f * di;
        q = q0 + fd;
        v = di * speed;
      }
      if (a.samples) a.samples[o + j] = q;
      if (a.sample_vel) a.sample_vel[o + j] = v;
    }
  }
}

}  // namespace

extern "C" int mir_retime_query_sizeof(void) { return (int)sizeof(MirRetimeQuery); }

extern "C" int mir_retime_path(MirHandle h, const MirRetimeQuery* q, int n_rows, const float* paths, const float* ea, const float* eb,
                               const float* elo, const float* ehi, float* x, float* t, float* duration, int32_t* status, int32_t* n_samples,
                               float* samples, float* sample_vel, void* stream) {
  const char* const who = "mir_retime_path";
  const RetimeCall c{h != nullptr, h && h->pending, q, n_rows, paths, ea, eb, elo, ehi, x, t, duration, status, n_samples, samples, sample_vel};
  const int rc = retime_check(c, [&](int code, const char* what) { return query_error(code, who, what); });
  if (rc != MIR_OK || n_rows == 0) return rc;
  RetimeArgs a;
  memset(&a, 0, sizeof a);
  a.paths = paths; a.x = x; a.t = t; a.duration = duration; a.status = status; a.n_samples = n_samples; a.samples = samples; a.sample_vel = sample_vel;
  a.K = q->num_waypoints; a.D = q->n_dofs; a.E = q->n_extra; a.T = q->num_samples;
  if (a.E > 0) { a.ea = ea; a.eb = eb; a.elo = elo; a.ehi = ehi; }
  a.dt = q->dt; a.vs2 = q->max_path_speed * q->max_path_speed;
  memcpy(a.vmax, q->vmax, sizeof a.vmax);
  memcpy(a.amax, q->amax, sizeof a.amax);
  return launch_rows<64>(h, mir_retime_kernel, n_rows, stream, a);
}
