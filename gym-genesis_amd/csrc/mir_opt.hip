// mir_opt.hip — batched trajectory optimisation of joint paths (mir_optimize_path); include/mirigid.h and DESIGN.md, "Trajectory
// optimisation".
//
// What it serves: the step behind plan_path / blend_path that makes a path better.  For a list of envs, one launch takes each row's
// joint path as a seed, moves its interior waypoints down the covariant gradient of smoothness plus an obstacle cost of the sphere
// model against the static scene (CHOMP's update, a backtracking line search), sweeps the result with the planner's edge rule and
// writes it -- or the input, where the sweep blocks.
//
// Mapping: one workgroup of one wave64 per row, as mir_plan.hip and mir_blend.hip, whose row machinery (mir_plan_row.h: PlanRow<SELF,
// CARRY>, plan_setup) does the set-up, the forward kinematics (lane = body) and the whole of the final sweep (clearance, self_clearance,
// n_sub, sample: the planner's edge rule on the same bits).  The descent's own pass over a path is here: per interior waypoint the
// forward kinematics, lane j < D turns the axis and anchor of planned dof j into the world (LDS), then lane = probe in chunks of 64
// through dist_probe_min, whose winner gives d, c(d), c'(d) and the normal; the cost is one butterfly sum per chunk, the gradient one
// butterfly sum per chunk and dof (skipped for a chunk without an active probe), kept by lane j.  Lane j < D holds column j of every
// path and gradient buffer (written and read by lane j alone), the Thomas recurrence (n serial steps forward, n back, the candidate
// written on the way back) and the limit test.
//   The scalar part of the rule is mir_opt_front.h, which the CPU tests build with g++.
// LDS: PlanLds (its poly member is one of the two path buffers), the other path buffer and two gradient buffers of K x 16 floats in
//   dynamic LDS, the sphere list of the self test behind them.  The buffers change roles by exchanging pointers.
// Bounds: the descent is ONE loop of at most 1 + max_iterations (max_halvings + 1) passes (every pass ends the loop, ends an iteration
//   or halves alpha); a pass is bounded by n, N, D, the geoms and the depth of the tree; the sweep by K and the 4096 samples of an edge.
// Stores: plain dword stores by lanes 0 .. D-1 or by lane 0.  No atomics, no scratch, no cross-wave barrier: the same bits run to run.
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

#include "mir_opt_front.h"

namespace {

constexpr int OPT_STRIDE = PLAN_MAX_DOF;  // floats per waypoint of a path or gradient buffer (PlanLds::poly's row)

struct OptArgs {
  PlanArgs p;  // the clearance side, as mir_path_clearance fills it
  int K, max_iter, max_halvings;
  float ws, wo, step, eps, ftol;
  OptConsts c;
  uint16_t chain[MIR_MAX_BODY];    // bit j: planned dof j lies on the chain from the world to the body
  uint8_t dof_body[PLAN_MAX_DOF];  // the body of planned dof j
  uint32_t prismatic;              // bit j: planned dof j is prismatic
  const float* paths;
  float *path_out, *cost, *min_d, *grad0;
  int32_t *status, *stats;
};
static_assert(sizeof(OptArgs) <= 4096, "kernel arguments");
static_assert(sizeof(PlanLds) + 2 * sizeof(float) * PLAN_MAX_DOF * 4 == OPT_FIXED_LDS, "the fixed LDS of a row");

extern __shared__ float opt_dyn[];

// the butterfly sum of a chunk: every lane takes part and holds the same bits
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off);
  return v;
}

struct OptValue { float S, O, U, mind; };

template <bool SELF, bool CARRY>
__global__ __launch_bounds__(64) void mir_opt_kernel(OptArgs a) {
  __shared__ PlanLds L;
  __shared__ float jax[PLAN_MAX_DOF][4], jan[PLAN_MAX_DOF][4];  // axis and anchor of planned dof j in the world
  const int lane = threadIdx.x, row = blockIdx.x, D = a.p.D, K = a.K, n = K - 2;
  PlanRow<SELF, CARRY> r{a.p, L, lane, 0, 0, false, opt_dyn + (size_t)3 * K * OPT_STRIDE, SELF_LIST};
  plan_setup(r, row, sphere_row_env(a.p.r, row));
  const bool isd = lane < D;
  const int dj = isd ? lane : 0;
  const float lo = a.p.lo[dj], hi = a.p.hi[dj];
  const float wo = a.p.ignore ? 0.0f : a.wo;
  float* X = &L.poly[0][0];  // the path the descent stands on, and its gradient
  float* Gx = opt_dyn + (size_t)K * OPT_STRIDE;
  float* Xc = opt_dyn;  // the candidate, and its gradient
  float* Gc = opt_dyn + (size_t)2 * K * OPT_STRIDE;

  // ---- 1. the input into both path buffers (lane j: column j), the checks
  const float* const in = a.paths + (size_t)row * K * D;
  const float first = isd ? in[lane] : 0.0f;
  bool notfinite = false, moves = false, outside = false;
  for (int k = 0; k < K; k++) {
    const float v = isd ? in[(size_t)k * D + lane] : 0.0f;
    notfinite = notfinite || (isd && !opt_finite(v));
    moves = moves || (isd && !(v == first));
    outside = outside || (isd && k > 0 && k < K - 1 && opt_outside(v, lo, hi));
    if (isd) {
      X[k * OPT_STRIDE + lane] = v;
      Xc[k * OPT_STRIDE + lane] = v;
    }
  }
  int status = MIR_PLAN_OK;
  if (__ballot(notfinite) != 0ull) status = MIR_OPT_NOT_FINITE;
  else if (__ballot(moves) == 0ull) status = MIR_OPT_NO_MOTION;
  else if (__ballot(outside) != 0ull) status = MIR_OPT_OUT_OF_LIMITS;

  int stop = MIR_OPT_STOP_NONE, iterations = 0, accepted = 0, halvings = 0, evaluated = 0;
  OptValue cur{0.0f, 0.0f, 0.0f, INFINITY}, v0 = cur;
  if (status == MIR_PLAN_OK) {
    // ---- 2. - 6. one loop of passes: the first evaluates the input, every later one a candidate of the line search
    bool seeded = false;
    int it = 0, h = 0;
    float alpha = a.step;
    stop = MIR_OPT_STOP_ITERATIONS;
    for (;;) {
      bool out = false;
      if (seeded) {  // 4. the Thomas recurrence on column j, the candidate written on the way back
        if (isd) {
          float y = 0.0f;
          for (int i = 1; i <= n; i++) {
            y = i == 1 ? Gx[OPT_STRIDE + lane] : opt_forward(Gx[i * OPT_STRIDE + lane], a.c.rpiv[i - 2], y);
            Xc[i * OPT_STRIDE + lane] = y;
          }
          float x = 0.0f;
          for (int i = n; i >= 1; i--) {
            x = opt_backward(Xc[i * OPT_STRIDE + lane], x, a.c.rpiv[i - 1]);  // (x_{n+1} = 0)
            const float cand = opt_candidate(X[i * OPT_STRIDE + lane], x, a.c.ik, alpha);
            Xc[i * OPT_STRIDE + lane] = cand;
            out = out || opt_outside(cand, lo, hi);
          }
        }
        out = __ballot(out) != 0ull;
      }
      OptValue e{0.0f, 0.0f, INFINITY, INFINITY};
      if (!out) {
        // ---- 2., 3. the pass: S, then per interior waypoint the probes' cost and gradient
        float sl = 0.0f;
        if (isd)
          for (int i = 0; i + 1 < K; i++) sl = opt_s_add(sl, Xc[(i + 1) * OPT_STRIDE + lane], Xc[i * OPT_STRIDE + lane]);
        if (isd) L.qs[lane] = sl;
        WSYNC();
        float ss = 0.0f;
        for (int j = 0; j < D; j++) ss = ss + L.qs[j];
        WSYNC();
        float oo = 0.0f, mind = INFINITY;
        unsigned long long nan = 0ull;
        for (int i = 1; i <= n; i++) {
          const float q = isd ? Xc[i * OPT_STRIDE + lane] : 0.0f;
          float Gs = 0.0f;
          if (!a.p.ignore) {
            if (isd) L.qrow[a.p.qadr[lane]] = q;
            WSYNC();
            r.fk(false);
            if (isd) {
              const int b = a.dof_body[lane];
              st3(jax[lane], qrot(ld4(L.xq[b]), ld3(a.p.r.m.b_axis + b * 3)));
              st3(jan[lane], ld3(L.xp[b]));
            }
            WSYNC();
            evaluated++;
            for (int base = 0; base < a.p.N; base += 64) {
              const bool valid = base + lane < a.p.N;
              const int probe = valid ? base + lane : a.p.N - 1;
              const ProbeWorld p = probe_world(a.p.r, probe, L.xp, L.xq);
              const DistBest w = dist_probe_min(L.rec, r.count, a.p.t.planes, a.p.t.tris, p.c, p.radius, a.p.max_distance);
              const bool hit = valid && w.bestk >= 0 && w.best <= a.p.max_distance;
              nan |= probe_nonfinite(valid, p.c);
              const float d = (hit ? w.best : a.p.max_distance) - a.p.margin;
              if (valid) mind = fminf(mind, d);
              const float cv = hit ? opt_c(d, a.eps) : 0.0f;
              const float dc = hit ? opt_dc(d, a.eps) : 0.0f;
              oo = oo + wave_sum(cv);
              if (__ballot(dc != 0.0f) != 0ull) {
                const float* const rc = L.rec + (w.bestk >= 0 ? w.bestk : 0) * DIST_REC;  // the winner's frame: rows of R_g
                const V3 nw = v3(rc[8] * w.bn.x + rc[9] * w.bn.y + rc[10] * w.bn.z, rc[11] * w.bn.x + rc[12] * w.bn.y + rc[13] * w.bn.z,
                                 rc[14] * w.bn.x + rc[15] * w.bn.y + rc[16] * w.bn.z);
                const uint32_t chain = a.chain[a.p.r.link[probe]];
                for (int j = 0; j < D; j++) {
                  const V3 aj = ld3(jax[j]);
                  const V3 J = ((a.prismatic >> j) & 1u) ? aj : cross(aj, p.c - ld3(jan[j]));
                  const float t = wave_sum(((chain >> j) & 1u) && dc != 0.0f ? dc * dot(nw, J) : 0.0f);
                  if (lane == j) Gs = Gs + t;
                }
              }
            }
          }
          if (isd) Gc[i * OPT_STRIDE + lane] = opt_grad(Xc[(i - 1) * OPT_STRIDE + lane], q, Xc[(i + 1) * OPT_STRIDE + lane], Gs, a.ws, wo, a.c.km1, a.c.ik);
        }
        e.S = opt_S(a.c.hk, ss);
        e.O = nan != 0ull || r.bad ? INFINITY : opt_O(a.c.ik, oo);
        e.U = opt_U(a.ws, e.S, wo, e.O);
        e.mind = wave_min(mind);
      }
      if (!seeded) {  // the input's pass: its cost and gradient are what the descent starts from
        seeded = true;
        { float* t = X; X = Xc; Xc = t; }
        { float* t = Gx; Gx = Gc; Gc = t; }
        cur = e;
        v0 = e;
        if (a.grad0) {
          float* const g0 = a.grad0 + (size_t)row * K * D;
          for (int k = 0; k < K; k++)
            if (isd) g0[(size_t)k * D + lane] = k > 0 && k < K - 1 ? Gx[k * OPT_STRIDE + lane] : 0.0f;
        }
        if (a.max_iter == 0) break;
        iterations = 1;
        continue;
      }
      if (!out && opt_accept(e.U, cur.U)) {  // 5., 6.
        const bool conv = opt_converged(cur.U, e.U, a.ftol);
        { float* t = X; X = Xc; Xc = t; }
        { float* t = Gx; Gx = Gc; Gc = t; }
        cur = e;
        accepted++;
        if (conv) { stop = MIR_OPT_STOP_CONVERGED; break; }
        it++;
        if (it == a.max_iter) break;
        iterations = it + 1;
        h = 0;
        alpha = a.step;
        continue;
      }
      if (h == a.max_halvings) { stop = MIR_OPT_STOP_STALLED; break; }
      h++;
      halvings++;
      alpha = 0.5f * alpha;
    }

    // ---- 7. the sweep of what the descent reached: q_0 (an edge of one sample), then every edge, the first failure ends it
    if (!a.p.ignore) {
      for (int k = -1; k + 1 < K && status == MIR_PLAN_OK; k++) {
        const float av = isd ? X[(k < 0 ? 0 : k) * OPT_STRIDE + lane] : 0.0f, bv = isd ? X[(k + 1) * OPT_STRIDE + lane] : 0.0f;
        const float diff = bv - av;
        const int ns = r.n_sub(diff);
        for (int i = 1; i <= ns && status == MIR_PLAN_OK; i++) {
          if (!(r.clearance(PlanRow<SELF, CARRY>::sample(av, bv, diff, i, ns)) >= a.p.margin)) status = MIR_OPT_BLOCKED;
          if constexpr (SELF)
            if (status == MIR_PLAN_OK && !(r.self_clearance() >= a.p.self_margin)) status = MIR_OPT_BLOCKED_SELF;
        }
      }
    }
  }

  // ---- outputs: the path reached where the sweep passed, else the input's bits
  float* const out = a.path_out + (size_t)row * K * D;
  if (status == MIR_PLAN_OK) {
    for (int k = 0; k < K; k++)
      if (isd) out[(size_t)k * D + lane] = X[k * OPT_STRIDE + lane];
  } else {
    for (int k = 0; k < K; k++)
      if (isd) out[(size_t)k * D + lane] = in[(size_t)k * D + lane];
  }
  if (status > MIR_OPT_BLOCKED_SELF && a.grad0) {  // (a failed check: no gradient)
    float* const g0 = a.grad0 + (size_t)row * K * D;
    for (int k = 0; k < K; k++)
      if (isd) g0[(size_t)k * D + lane] = 0.0f;
  }
  if (lane == 0) {
    a.status[row] = status;
    if (a.cost) {
      float* const c = a.cost + (size_t)row * 4;
      c[0] = v0.S; c[1] = v0.O; c[2] = cur.S; c[3] = cur.O;
    }
    if (a.stats) {
      int32_t* const st = a.stats + (size_t)row * 6;
      st[0] = iterations; st[1] = accepted; st[2] = halvings; st[3] = evaluated; st[4] = r.checked; st[5] = stop;
    }
    if (a.min_d) a.min_d[row] = status == MIR_PLAN_OK ? cur.mind : v0.mind;
  }
}

}  // namespace

extern "C" int mir_opt_query_sizeof(void) { return (int)sizeof(MirOptQuery); }

extern "C" int mir_optimize_path(MirHandle h, const MirOptQuery* q, const MirPlanQuery* pq, const MirSelfQuery* sq, const MirCarryQuery* cq,
                                 const float* probes, const int32_t* probe_link, const int32_t* dof_qadr, const int64_t* env_idx, int32_t n_rows,
                                 const float* qpos_start, const float* paths, int32_t K, float* path_out, int32_t* status, float* cost,
                                 int32_t* stats, float* min_d, float* grad0, void* stream) {
  const char* const who = "mir_optimize_path";
  const auto refuse = [&](int code, const char* what) { return query_error(code, who, what); };
  const OptCall oc{h != nullptr, q, pq, probes, dof_qadr, paths, path_out, status, K};
  int rc;
  if ((rc = opt_check(oc, refuse)) != MIR_OK) return rc;
  const PlanCall c = plan_call(who, h, pq, sq, sq != nullptr, cq, cq != nullptr, probes, probe_link, dof_qadr, env_idx, n_rows, qpos_start, nullptr,
                               nullptr, stream);
  OptArgs a;
  memset(&a, 0, sizeof a);
  long long R = 0;
  if ((rc = plan_front(c, false, a.p, R)) != MIR_OK) return rc;
  if ((rc = opt_check_band(q, pq, refuse)) != MIR_OK) return rc;
  if ((rc = opt_check_lds(K, a.p.NS, c.self, refuse)) != MIR_OK) return rc;
  if (R == 0) return MIR_OK;
  a.K = K; a.max_iter = q->max_iterations; a.max_halvings = q->max_halvings;
  a.ws = q->smooth_weight; a.wo = q->obstacle_weight; a.step = q->step; a.eps = q->activation; a.ftol = q->ftol;
  opt_consts(K, a.c);
  // the chain of every body over the planned dofs (a free body starts a chain of its own; the carried body takes its link's)
  const ModelView mv(h);
  const int D = pq->n_dofs;
  for (int j = 0; j < D; j++)
    for (int b = 1; b < h->nbody; b++) {
      const int jt = mv.jtype(b);
      if ((jt == MIR_JNT_REVOLUTE || jt == MIR_JNT_PRISMATIC) && mv.qadr(b) == dof_qadr[j]) {
        a.dof_body[j] = (uint8_t)b;
        if (jt == MIR_JNT_PRISMATIC) a.prismatic |= 1u << j;
      }
    }
  for (int b = 1; b < h->nbody; b++) {
    const int par = mv.parent(b);
    uint16_t m = par > 0 && mv.jtype(b) != MIR_JNT_FREE ? a.chain[par] : (uint16_t)0;
    for (int j = 0; j < D; j++)
      if (a.dof_body[j] == b) m |= (uint16_t)(1u << j);
    a.chain[b] = m;
  }
  if (c.carry) a.chain[cq->body] = a.chain[cq->link];
  a.paths = paths; a.path_out = path_out; a.status = status; a.cost = cost; a.stats = stats; a.min_d = min_d; a.grad0 = grad0;
  const auto kernel = pick_self_carry(c.self, c.carry, [](auto S, auto C) { return mir_opt_kernel<decltype(S)::value, decltype(C)::value>; });
  return plan_launch(c, kernel, R, a, a.p, (size_t)3 * K * OPT_STRIDE * sizeof(float));
}
