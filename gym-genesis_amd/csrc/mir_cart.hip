// mir_cart.hip — batched straight-line end-effector paths (mir_cartesian_path); include/mirigid.h and DESIGN.md, "Cartesian paths".
//
// What it serves: the approach, the lift and the place of a grasp.  For a list of envs, one launch takes each row's link along K
// straight segments: at every sample the inverse kinematics of mir_inverse_kinematics from the sample before, a joint-jump test, and
// the planner's edge check from the sample before.  The first failure ends the row, which keeps what it achieved.
//
// Mapping: one workgroup of one wave64 per row, as mir_plan.hip, whose row machinery (mir_plan_row.h: PlanRow<SELF, CARRY>, plan_setup)
// is the collision half unchanged: clear(q) with lane = body in the forward kinematics and lane = probe in the distance tests.
//   The IK half is written from the device helpers of mir_ik_front.h.  The 16-lane solver of mir_ik.hip runs REDUNDANTLY in all four
//   DPP rows of the wave: lane & 15 = element of the chain, every row holds the same bits (same operands, same row operations), so a
//   decision of the solver is wave-uniform without a broadcast and no lane idles behind a predicate that the DPP row operations would
//   not honour anyway.  A configuration changes layout between the halves through LDS (PlanLds::qs): the lanes 0 .. 15 write their
//   moving joint to its planned dof, lane j < D reads planned dof j.
//   Points go straight to global memory, column j by lane j; the waypoints are resampled from the row's own points by the lanes that
//   wrote them.  K is streamed twice: once for the sample count S, once for the samples.
// Bounds: K, S <= P, max_iters, the 4096 samples of an edge, P, W.  A NaN anywhere ends the row: in a target by NOT_FINITE, in a
//   configuration by IK_FAILED (a NaN compares false with the tolerances).
// Stores: plain dword stores by lanes 0 .. D-1 (or lane 0).  No atomics, no scratch, no cross-wave barrier.
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

#include "mir_ik_front.h"

#include "mir_cart_front.h"

namespace {

struct CartArgs {
  PlanArgs p;       // the clearance side, as mir_path_clearance fills it
  IkElems ch;       // the chain world -> link, root first
  int dof_of[G];    // the planned dof an element's joint is, -1: the joint does not move
  int el_qadr[G];   // the qpos address of a scalar element's joint in the row
  int K, P, W, userot;
  int max_iters, respect_limits;
  float damping2, pos_tol, rot_tol, inv_pos_tol, inv_rot_tol, max_step;
  float max_pos_step, max_rot_step, jump;
  const float *target_pos, *target_quat;
  float *points, *fraction, *path;
  int32_t *n_points, *status, *stats;
};
static_assert(sizeof(CartArgs) <= 4096, "kernel arguments");

extern __shared__ float cart_dyn[];

// target k of the row: its position, its quaternion normalised (userot), whether it counts as not finite
struct CartKnot { float p[3], q[4]; bool bad; };
__device__ __forceinline__ CartKnot cart_knot(const float* tp, const float* tq, int k) {
  CartKnot t;
  t.bad = false;
  for (int c = 0; c < 3; c++) {
    t.p[c] = tp[(size_t)k * 3 + c];
    t.bad = t.bad || !cart_finite(t.p[c]);
  }
  t.q[0] = 1.0f; t.q[1] = t.q[2] = t.q[3] = 0.0f;
  if (tq) {
    const Q4 raw = ld4(tq + (size_t)k * 4);
    const float n2 = raw.w * raw.w + raw.x * raw.x + raw.y * raw.y + raw.z * raw.z;
    t.bad = t.bad || !cart_finite(raw.w) || !cart_finite(raw.x) || !cart_finite(raw.y) || !cart_finite(raw.z) || !(n2 >= 1e-30f) || !cart_finite(n2);
    const Q4 nq = qnormalize(raw);
    t.q[0] = nq.w; t.q[1] = nq.x; t.q[2] = nq.y; t.q[3] = nq.z;
  }
  return t;
}

// the segment from (pa, qa) to knot b: its quaternion delta and its sample count
struct CartSeg { float d[4], sn, ang; int n; };
__device__ __forceinline__ CartSeg cart_segment(const CartArgs& a, const float* pa, const float* qa, const CartKnot& b) {
  CartSeg s;
  s.d[0] = 1.0f; s.d[1] = s.d[2] = s.d[3] = 0.0f;
  s.sn = 0.0f; s.ang = 0.0f;
  if (a.userot) cart_delta(qa, b.q, s.d, &s.sn, &s.ang);
  const float dx = b.p[0] - pa[0], dy = b.p[1] - pa[1], dz = b.p[2] - pa[2];
  s.n = cart_count(sqrtf(dx * dx + dy * dy + dz * dz), s.ang, a.max_pos_step, a.max_rot_step);
  return s;
}

template <bool SELF, bool CARRY>
__global__ __launch_bounds__(64) void mir_cart_kernel(CartArgs a) {
  __shared__ PlanLds L;
  const int lane = threadIdx.x, l16 = lane & 15, row = blockIdx.x, D = a.p.D;
  PlanRow<SELF, CARRY> r{a.p, L, lane, 0, 0, false, cart_dyn, SELF_LIST};
  plan_setup(r, row, sphere_row_env(a.p.r, row));
  const bool isd = lane < D;
  const int dj = isd ? lane : 0;
  const float sv = isd ? L.qrow[a.p.qadr[dj]] : 0.0f;  // a0: planned dof j in lane j
  // ---- my element of the chain (the same in each of the four DPP rows)
  const int n = a.ch.n;
  const int eef4 = ((lane & ~15) + n - 1) << 2;  // (lane_gather address of the chain's last element in this DPP row)
  const bool onchain = l16 < n;
  const int jt = onchain ? a.ch.jtype[l16] : MIR_JNT_FIXED;
  const bool scalar = onchain && a.ch.qcol[l16] >= 0 && (jt == MIR_JNT_REVOLUTE || jt == MIR_JNT_PRISMATIC);
  const int dof = scalar ? a.dof_of[l16] : -1;
  const bool moving = dof >= 0;
  const V3 bpos = ld3(a.ch.pos[l16]), baxis = ld3(a.ch.axis[l16]);
  const Q4 bquat = ld4(a.ch.quat[l16]);
  const float lo = a.ch.lo[l16], hi = a.ch.hi[l16];
  const bool lim = moving && a.ch.limited[l16] && a.respect_limits;
  const bool userot = a.userot != 0;
  float q = scalar ? L.qrow[a.el_qadr[l16]] : 0.0f;  // every scalar joint of the chain from the start row; the moving ones will move
  WSYNC();

  // ---- X_0: the link's pose at a0 by the chain's forward kinematics
  float pa[3], qa[4];
  {
    const Pose x = path_scan(ik_elem_local(onchain, jt, bpos, bquat, baxis, q), l16, n);
    const V3 pe = gather3(eef4, x.P);
    const Q4 qe = gather4(eef4, x.Qx);
    pa[0] = pe.x; pa[1] = pe.y; pa[2] = pe.z;
    qa[0] = qe.w; qa[1] = qe.x; qa[2] = qe.y; qa[3] = qe.z;
  }
  const float* const tp = a.target_pos + (size_t)row * a.K * 3;
  const float* const tq = userot ? a.target_quat + (size_t)row * a.K * 4 : nullptr;

  // ---- the sample count S and the targets' finiteness: K streamed once
  long long S = 0;
  bool notfinite = false;
  {
    float pk[3] = {pa[0], pa[1], pa[2]}, qk[4] = {qa[0], qa[1], qa[2], qa[3]};
    for (int k = 0; k < a.K; k++) {
      const CartKnot b = cart_knot(tp, tq, k);
      notfinite = notfinite || b.bad;
      S += cart_segment(a, pk, qk, b).n;
      for (int c = 0; c < 3; c++) pk[c] = b.p[c];
      for (int c = 0; c < 4; c++) qk[c] = b.q[c];
    }
  }

  float* const out = a.points + (size_t)row * a.P * D;
  if (isd) out[lane] = sv;
  int status = MIR_PLAN_OK, np = 1, failseg = -1, iters = 0;
  float prev = sv;  // the last accepted configuration, planned dof j in lane j
  if (notfinite) status = MIR_CART_NOT_FINITE;
  else if (S + 1 > (long long)a.P) status = MIR_CART_TOO_MANY_POINTS;
  else if (!(r.clearance(sv) >= a.p.margin)) status = MIR_PLAN_START_IN_COLLISION;
  else if (SELF && !(r.self_clearance() >= a.p.self_margin)) status = MIR_PLAN_START_IN_SELF_COLLISION;
  else {
    for (int k = 0; k < a.K && status == MIR_PLAN_OK; k++) {
      const CartKnot b = cart_knot(tp, tq, k);
      const CartSeg sg = cart_segment(a, pa, qa, b);
      for (int i = 1; i <= sg.n && status == MIR_PLAN_OK; i++) {
        float tpv[3], tqv[4] = {1.0f, 0.0f, 0.0f, 0.0f};
        cart_target(pa, b.p, qa, b.q, sg.d, sg.sn, sg.ang, i, sg.n, userot, tpv, tqv);
        const V3 tpos = v3(tpv[0], tpv[1], tpv[2]);
        const Q4 tquat = Q4{tqv[0], tqv[1], tqv[2], tqv[3]};
        // ---- the iteration of mir_ik.hip on my element, seeded with the last accepted configuration (q)
        bool done = false;
        int my_iters = 0;
        float q_acc = q, epn = 0.0f, ern = 0.0f;
        LmState lm = {a.damping2, 0, 0.0f};
        float J[6] = {0, 0, 0, 0, 0, 0}, e[6] = {0, 0, 0, 0, 0, 0};
        for (int it = 0; it <= a.max_iters; it++) {
          const Pose x = path_scan(ik_elem_local(onchain, jt, bpos, bquat, baxis, q), l16, n);
          const V3 P = x.P;
          const Q4 Qx = x.Qx;
          const V3 pe = gather3(eef4, P);
          const Q4 qe = gather4(eef4, Qx);
          const V3 ep = tpos - pe;
          V3 er = v3(0, 0, 0);
          if (userot) er = ik_rot_error(tquat, qe);
          const float epn_c = sqrtf(dot(ep, ep)), ern_c = sqrtf(dot(er, er));
          const float metric = epn_c * a.inv_pos_tol + ern_c * a.inv_rot_tol;
          if (!done) {
            if (lm_accepts(lm, metric, it == 0)) {
              lm = lm_accept(lm, metric, it == 0, a.damping2);
              epn = epn_c; ern = ern_c;
              e[0] = ep.x; e[1] = ep.y; e[2] = ep.z; e[3] = er.x; e[4] = er.y; e[5] = er.z;
              q_acc = q;
              const JacColumn c = ik_jac_column(moving, jt, Qx, P, baxis, pe);
              J[0] = c.jv.x; J[1] = c.jv.y; J[2] = c.jv.z; J[3] = userot ? c.jw.x : 0.0f; J[4] = userot ? c.jw.y : 0.0f; J[5] = userot ? c.jw.z : 0.0f;
            } else {
              lm = lm_reject(lm, a.damping2);
            }
            if ((epn < a.pos_tol && ern < a.rot_tol) || lm_stalled(lm)) done = true;
          }
          if (it == a.max_iters) break;
          if (!__any(!done)) break;
          // A = J J^T + lambda^2 I in every lane (J, e: the accepted iterate's)
          float A[6][6];
#pragma unroll
          for (int rr = 0; rr < 6; rr++)
#pragma unroll
            for (int c = 0; c <= rr; c++) {
              const float v = gsum(J[rr] * J[c]) + (rr == c ? lm.lam2 : 0.0f);
              A[rr][c] = v;
              A[c][rr] = v;
            }
          // y = A^-1 e (Cholesky, SPD by the damping)
          float Lc[6][6], y[6], il[6];
#pragma unroll
          for (int rr = 0; rr < 6; rr++)
#pragma unroll
            for (int c = 0; c <= rr; c++) {
              float sacc = A[rr][c];
#pragma unroll
              for (int kk = 0; kk < c; kk++) sacc -= Lc[rr][kk] * Lc[c][kk];
              if (rr == c) {
                const float dd = sqrtf(fmaxf(sacc, 1e-30f));
                float ir = __builtin_amdgcn_rcpf(dd);
                Lc[rr][c] = dd;
                il[rr] = ir;
              } else {
                Lc[rr][c] = sacc * il[c];
              }
            }
#pragma unroll
          for (int rr = 0; rr < 6; rr++) {
            float sacc = e[rr];
#pragma unroll
            for (int kk = 0; kk < rr; kk++) sacc -= Lc[rr][kk] * y[kk];
            y[rr] = sacc * il[rr];
          }
#pragma unroll
          for (int rr = 5; rr >= 0; rr--) {
            float sacc = y[rr];
#pragma unroll
            for (int kk = rr + 1; kk < 6; kk++) sacc -= Lc[kk][rr] * y[kk];
            y[rr] = sacc * il[rr];
          }
          float dq = 0.0f;
#pragma unroll
          for (int rr = 0; rr < 6; rr++) dq += J[rr] * y[rr];
          const float sc = ik_step_scale(dq, a.max_step);
          if (!done) my_iters = it + 1;
          q = q_acc;
          if (moving && !done) {
            q = q_acc + sc * dq;
            if (lim) q = fminf(fmaxf(q, lo), hi);
          }
        }
        iters += my_iters;
        if (!(epn < a.pos_tol && ern < a.rot_tol)) { status = MIR_CART_IK_FAILED; failseg = k; break; }
        // ---- the candidate in the planner's layout: the moving joints from q_acc, the other planned dofs from a0
        if (isd) L.qs[lane] = prev;
        WSYNC();
        if (lane < G && moving) L.qs[dof] = q_acc;
        WSYNC();
        const float cand = isd ? L.qs[lane] : 0.0f;
        WSYNC();
        const float diff = cand - prev;
        if (wave_max(isd ? fabsf(diff) : 0.0f) > a.jump) { status = MIR_CART_JOINT_JUMP; failseg = k; break; }
        // ---- edge(prev, cand): the planner's samples in order; the scene test is asked first
        if (!a.p.ignore) {
          const int ns = r.n_sub(diff);
          for (int s = 1; s <= ns; s++) {
            if (!(r.clearance(PlanRow<SELF, CARRY>::sample(prev, cand, diff, s, ns)) >= a.p.margin)) { status = MIR_CART_BLOCKED; break; }
            if constexpr (SELF)
              if (!(r.self_clearance() >= a.p.self_margin)) { status = MIR_CART_BLOCKED_SELF; break; }
          }
          if (status != MIR_PLAN_OK) { failseg = k; break; }
        }
        if (isd) out[(size_t)np * D + lane] = cand;
        np++;
        prev = cand;
        q = q_acc;
      }
      for (int c = 0; c < 3; c++) pa[c] = b.p[c];
      for (int c = 0; c < 4; c++) qa[c] = b.q[c];
    }
  }

  // ---- the tail repeats the last accepted point
  for (int k = np; k < a.P; k++)
    if (isd) out[(size_t)k * D + lane] = prev;
  // ---- waypoints: the dense polyline at equal steps of its index (every lane reads the column it wrote)
  if (a.path) {
    float* const wp = a.path + (size_t)row * a.W * D;
    for (int w = 0; w < a.W; w++) {
      float v = sv;
      if (np > 1) {
        if (w == 0) v = sv;
        else if (w == a.W - 1) v = prev;
        else {
          int i0;
          float t;
          cart_waypoint(w, a.W, np, &i0, &t);
          const float p0 = isd ? out[(size_t)i0 * D + lane] : 0.0f, p1 = isd ? out[(size_t)(i0 + 1) * D + lane] : 0.0f;
          v = p0 + t * (p1 - p0);
        }
      }
      if (isd) wp[(size_t)w * D + lane] = v;
    }
  }
  if (lane == 0) {
    a.status[row] = status;
    a.n_points[row] = np;
    a.fraction[row] = np > 1 ? cart_div((float)(np - 1), (float)S) : 0.0f;
    if (a.stats) {
      int32_t* const st = a.stats + (size_t)row * 4;
      st[0] = iters; st[1] = r.checked; st[2] = (int32_t)(S > 0x7fffffffLL ? 0x7fffffffLL : S); st[3] = failseg;
    }
  }
}

}  // namespace

extern "C" int mir_cart_query_sizeof(void) { return (int)sizeof(MirCartQuery); }

extern "C" int mir_cartesian_path(MirHandle h, const MirCartQuery* q, const MirPlanQuery* pq, const MirSelfQuery* sq, const MirCarryQuery* cq,
                                  const float* probes, const int32_t* probe_link, const int32_t* dof_qadr, const int64_t* env_idx, int32_t n_rows,
                                  const float* qpos_start, const float* target_pos, const float* target_quat, const MirIkOptions* opt, float* points,
                                  int32_t* n_points, float* fraction, int32_t* status, float* path, int32_t* stats, void* stream) {
  const char* const who = "mir_cartesian_path";
  const auto refuse = [&](int code, const char* what) { return query_error(code, who, what); };
  const CartCall cc{h != nullptr, q, pq, probes, dof_qadr, target_pos, points, n_points, fraction, status, path};
  int rc;
  if ((rc = cart_check(cc, refuse)) != MIR_OK) return rc;
  const PlanCall c = plan_call(who, h, pq, sq, sq != nullptr, cq, cq != nullptr, probes, probe_link, dof_qadr, env_idx, n_rows, qpos_start, nullptr,
                               nullptr, stream);
  CartArgs a;
  memset(&a, 0, sizeof a);
  long long R = 0;
  if ((rc = plan_front(c, false, a.p, R)) != MIR_OK) return rc;
  const int D = pq->n_dofs;
  if ((rc = cart_check_size(q, R, D, refuse)) != MIR_OK) return rc;
  MirIkOptions o;
  if ((rc = ik_options(opt, true, who, o)) != MIR_OK) return rc;
  // the chain world -> link; its moving joints are those that are planned dofs (the mask over the columns needs the columns: twice)
  const ModelView mv(h);
  IkTree t;
  const char* what = "";
  const int32_t link = q->link_body;
  if ((rc = build_ik_tree(mv, h->nbody, &link, 1, nullptr, "chain longer than 16 elements", t, &what)) != MIR_OK) return query_error(rc, who, what);
  uint8_t mask[MIR_MAX_DOF] = {0};
  for (int k = 0; k < t.n_arm; k++)
    for (int j = 0; j < D; j++)
      if (t.arm_qadr[k] == dof_qadr[j]) mask[k] = 1;
  if ((rc = build_ik_tree(mv, h->nbody, &link, 1, mask, "chain longer than 16 elements", t, &what)) != MIR_OK) return query_error(rc, who, what);
  if (!t.moving_cols) return refuse(MIR_E_INVALID, "no moving joint: no planned dof lies on the chain world -> link");
  if (R == 0) return MIR_OK;
  a.ch = t.el;
  for (int i = 0; i < G; i++) {
    const int col = t.el.qcol[i];
    a.dof_of[i] = -1;
    a.el_qadr[i] = col >= 0 ? t.arm_qadr[col] : 0;
    if (i < t.el.n && t.moving[i])
      for (int j = 0; j < D; j++)
        if (dof_qadr[j] == t.arm_qadr[col]) a.dof_of[i] = j;
  }
  a.K = q->num_targets; a.P = q->max_points; a.W = q->num_waypoints; a.userot = target_quat ? 1 : 0;
  a.max_iters = o.max_iters; a.respect_limits = o.respect_joint_limit;
  a.damping2 = (float)(o.damping * o.damping); a.pos_tol = (float)o.pos_tol; a.rot_tol = (float)o.rot_tol;
  a.inv_pos_tol = (float)(1.0 / o.pos_tol); a.inv_rot_tol = (float)(1.0 / o.rot_tol); a.max_step = (float)o.max_step;
  a.max_pos_step = q->max_pos_step; a.max_rot_step = q->max_rot_step; a.jump = q->jump_threshold;
  a.target_pos = target_pos; a.target_quat = target_quat;
  a.points = points; a.fraction = fraction; a.path = path; a.n_points = n_points; a.status = status; a.stats = stats;
  const auto kernel = pick_self_carry(c.self, c.carry, [](auto S, auto C) { return mir_cart_kernel<decltype(S)::value, decltype(C)::value>; });
  return plan_launch(c, kernel, R, a, a.p, 0);
}
