// mir_goal.hip — batched collision-checked motion planning to a SET of goal configurations (mir_plan_path_goals) and to a POSE of a link
// (mir_plan_path_pose: the same kernel with POSE set, which makes its goal set itself); include/mirigid.h and DESIGN.md, "Goal sets and
// pose goals".
//
// What it serves: two grasp approaches, the four symmetric grasps of a cube, several inverse-kinematics branches of one pose.  For a list
// of envs, one launch judges up to MIR_PLAN_MAX_GOALS goal configurations per row, tries the direct edge to the valid ones nearest
// first, and otherwise grows RRT-Connect with the goal tree started as a forest of the valid goals: the plan ends at whichever goal
// the trees meet through.  No host decision in between.
//
// Mapping: one workgroup of one wave64 per row, as mir_plan.hip, with its row machinery (mir_plan_row.h: PlanRow<SELF, CARRY>, plan_setup)
// and its tree loop (mir_plan_tree.h: PlanTrees, plan_grow_and_store) unchanged.  WSYNC() only.
//   Goals.  Goal g of the row is read by lanes 0 .. D-1 (lane j: planned dof j), checked against the limits and by clear(); a valid
//   goal goes straight into Tb's next node in dynamic LDS with PLAN_NO_PARENT, so the roots are the valid goals in ascending g and no
//   further LDS is needed.  Which g a root is travels in one register, four bits a root.
//   Direct edges.  Lane k < (valid goals) holds the squared L2 distance of root k from the start (the sum of `nearest`); a wave argmin
//   over the roots not yet tried gives the order, the lower root on a tie.
//   POSE.  The goal set is not read but made before the planner starts: for up to max_samples seeds the 16-lane LM-damped IK iteration of
//   mir_cart.hip (the helpers of mir_ik_front.h) runs redundantly in the four DPP rows of the wave, so every decision is wave-uniform;
//   the candidate changes layout through PlanLds::qs as in mir_cart.hip, is judged (converged, limits, clear(), not a duplicate) and goes
//   straight into Tb's next node.  Bounded by max_samples, max_iters and max_goals.
// Bounds: max_goals <= 8 for the two goal loops; everything else is the tree loop's (max_iterations, max_nodes, the 4096 samples of
//   an edge, MIR_PLAN_MAX_POLY, smooth_passes, num_waypoints).  A goal with a NaN or an infinity in it is outside the limits.
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

#include "mir_plan_tree.h"

#include "mir_ik_front.h"

#include "mir_cart_front.h"  // (cart_finite)

namespace {

struct GoalArgs {
  PlanArgs p;              // as mir_plan_path fills it; p.goal: the goal sets (R, NG, D)
  int NG;                  // max_goals
  const int32_t* n_goals;  // (R), nullable: NG for every row
  int32_t *goal_index, *goal_status;  // (R), (R, NG); both nullable
  // POSE (mir_plan_path_pose): the goal set is made by the row's wave, p.goal is not read
  IkElems ch;       // the chain world -> link, root first
  int dof_of[G];    // the planned dof an element's joint is, -1: the joint does not move
  int el_qadr[G];   // the qpos address of a scalar element's joint in the row
  int userot, max_iters, respect_limits, max_samples;
  float damping2, pos_tol, rot_tol, inv_pos_tol, inv_rot_tol, max_step, dedup;
  const float *target_pos, *target_quat;  // (R, 3), (R, 4) nullable
  float* goals_out;                        // (R, NG, D) nullable
  int32_t *n_goals_out, *goal_stats;       // (R), (R, 4); nullable
};
static_assert(sizeof(GoalArgs) <= 4096, "kernel arguments");

extern __shared__ float goal_dyn[];

template <bool SELF, bool CARRY, bool POSE>
__global__ __launch_bounds__(64) void mir_goal_kernel(GoalArgs ga) {
  __shared__ PlanLds L;
  const PlanArgs& a = ga.p;
  const int lane = threadIdx.x, row = blockIdx.x, D = a.D, MN = a.max_nodes, NG = ga.NG;
  const int env = sphere_row_env(a.r, row);
  PlanTrees T(L, goal_dyn, lane, D, MN);
  PlanRow<SELF, CARRY> r{a, L, lane, 0, 0, false, goal_dyn + PlanTrees::floats(D, MN), SELF_LIST};
  plan_setup(r, row, env);
  const bool isd = lane < D;
  const int dj = isd ? lane : 0;
  const float lo = a.lo[dj], hi = a.hi[dj];
  const float sv = isd ? L.qrow[a.qadr[dj]] : 0.0f;
  const int ng = POSE ? 0 : ga.n_goals ? min(max(__builtin_amdgcn_readfirstlane(ga.n_goals[row]), 0), NG) : NG;
  // POSE: my element of the chain (the same in each of the four DPP rows), its joint value in the start row
  const int l16 = lane & 15, nel = ga.ch.n;
  const int eef4 = ((lane & ~15) + nel - 1) << 2;  // (lane_gather address of the chain's last element in this DPP row)
  const bool onchain = POSE && l16 < nel;
  const int jt = onchain ? ga.ch.jtype[l16] : MIR_JNT_FIXED;
  const bool scalar = onchain && ga.ch.qcol[l16] >= 0 && (jt == MIR_JNT_REVOLUTE || jt == MIR_JNT_PRISMATIC);
  const int dof = scalar ? ga.dof_of[l16] : -1;
  const bool moving = dof >= 0;
  const float q0 = scalar ? L.qrow[ga.el_qadr[l16]] : 0.0f;
  int32_t* const gs = ga.goal_status ? ga.goal_status + (size_t)row * NG : nullptr;
  WSYNC();

  int status = MIR_PLAN_OK, npoly = 1, nvalid = 0, gi = -1;
  uint32_t root_goal = 0;  // four bits a root: the g it is
  V3 tpos = v3(0, 0, 0);
  Q4 tquat = Q4{1.0f, 0.0f, 0.0f, 0.0f};
  if constexpr (POSE) {  // the target: a value that is not finite or a zero quaternion ends the row before anything is evaluated
    const float* const tp = ga.target_pos + (size_t)row * 3;
    tpos = ld3(tp);
    bool badt = !cart_finite(tpos.x) || !cart_finite(tpos.y) || !cart_finite(tpos.z);
    if (ga.userot) {
      const Q4 raw = ld4(ga.target_quat + (size_t)row * 4);
      const float n2 = raw.w * raw.w + raw.x * raw.x + raw.y * raw.y + raw.z * raw.z;
      badt = badt || !cart_finite(raw.w) || !cart_finite(raw.x) || !cart_finite(raw.y) || !cart_finite(raw.z) || !(n2 >= 1e-30f) || !cart_finite(n2);
      tquat = qnormalize(raw);
    }
    if (badt) status = MIR_CART_NOT_FINITE;
  }
  if (status != MIR_PLAN_OK) {}
  else if (!(r.clearance(sv) >= a.margin)) status = MIR_PLAN_START_IN_COLLISION;
  else if (SELF && !(r.self_clearance() >= a.self_margin)) status = MIR_PLAN_START_IN_SELF_COLLISION;
  // ---- POSE: the goal set is made here.  Sample s: the seed (the start for s = 0, else every moving limited joint of the chain drawn
  // from its range by u(env, 0x40000000 | s, dof)), the iteration of mir_cart.hip on my element, redundantly in the four DPP rows, and
  // the candidate in the planner's layout; it is kept when it converged, lies inside the limits, is clear and is not a goal already kept
  if constexpr (POSE) {
    int tried = 0, conv = 0, rej = 0, iters = 0;
    const V3 bpos = ld3(ga.ch.pos[l16]), baxis = ld3(ga.ch.axis[l16]);
    const Q4 bquat = ld4(ga.ch.quat[l16]);
    const float clo = ga.ch.lo[l16], chi = ga.ch.hi[l16];
    const bool limited = moving && ga.ch.limited[l16];
    const bool lim = limited && ga.respect_limits;
    const bool userot = ga.userot != 0;
    for (int s = 0; s < ga.max_samples && nvalid < NG && status == MIR_PLAN_OK; s++) {
      tried++;
      float q = q0;
      if (s > 0 && limited) q = clo + plan_u(a.seed, (uint32_t)env, 0x40000000u | (uint32_t)s, (uint32_t)dof) * (chi - clo);
      bool done = false;
      int my_iters = 0;
      float q_acc = q, epn = 0.0f, ern = 0.0f;
      LmState lm = {ga.damping2, 0, 0.0f};
      float J[6] = {0, 0, 0, 0, 0, 0}, e[6] = {0, 0, 0, 0, 0, 0};
      for (int it = 0; it <= ga.max_iters; it++) {
        const Pose x = path_scan(ik_elem_local(onchain, jt, bpos, bquat, baxis, q), l16, nel);
        const V3 P = x.P;
        const Q4 Qx = x.Qx;
        const V3 pe = gather3(eef4, P);
        const Q4 qe = gather4(eef4, Qx);
        const V3 ep = tpos - pe;
        V3 er = v3(0, 0, 0);
        if (userot) er = ik_rot_error(tquat, qe);
        const float epn_c = sqrtf(dot(ep, ep)), ern_c = sqrtf(dot(er, er));
        const float metric = epn_c * ga.inv_pos_tol + ern_c * ga.inv_rot_tol;
        if (!done) {
          if (lm_accepts(lm, metric, it == 0)) {
            lm = lm_accept(lm, metric, it == 0, ga.damping2);
            epn = epn_c; ern = ern_c;
            e[0] = ep.x; e[1] = ep.y; e[2] = ep.z; e[3] = er.x; e[4] = er.y; e[5] = er.z;
            q_acc = q;
            const JacColumn c = ik_jac_column(moving, jt, Qx, P, baxis, pe);
            J[0] = c.jv.x; J[1] = c.jv.y; J[2] = c.jv.z; J[3] = userot ? c.jw.x : 0.0f; J[4] = userot ? c.jw.y : 0.0f; J[5] = userot ? c.jw.z : 0.0f;
          } else {
            lm = lm_reject(lm, ga.damping2);
          }
          if ((epn < ga.pos_tol && ern < ga.rot_tol) || lm_stalled(lm)) done = true;
        }
        if (it == ga.max_iters) break;
        if (!__any(!done)) break;
        float A[6][6];
#pragma unroll
        for (int rr = 0; rr < 6; rr++)
#pragma unroll
          for (int c = 0; c <= rr; c++) {
            const float v = gsum(J[rr] * J[c]) + (rr == c ? lm.lam2 : 0.0f);
            A[rr][c] = v;
            A[c][rr] = v;
          }
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
              Lc[rr][c] = dd;
              il[rr] = __builtin_amdgcn_rcpf(dd);
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
        const float sc = ik_step_scale(dq, ga.max_step);
        if (!done) my_iters = it + 1;
        q = q_acc;
        if (moving && !done) {
          q = q_acc + sc * dq;
          if (lim) q = fminf(fmaxf(q, clo), chi);
        }
      }
      iters += my_iters;
      if (!(epn < ga.pos_tol && ern < ga.rot_tol)) continue;  // (a) (a NaN compares false)
      conv++;
      // the candidate in the planner's layout: the moving joints from q_acc, the other planned dofs (the fingers) from the start
      if (isd) L.qs[lane] = sv;
      WSYNC();
      if (lane < G && moving) L.qs[dof] = q_acc;
      WSYNC();
      const float cand = isd ? L.qs[lane] : 0.0f;
      WSYNC();
      if (__ballot(isd && !(cand >= lo && cand <= hi)) != 0ull) { rej++; continue; }  // (b)
      if (!r.clear(cand)) { rej++; continue; }                                          // (c)
      bool dup = false;                                                                  // (d)
      for (int k = 0; k < nvalid && !dup; k++) dup = !(wave_max(isd ? fabsf(cand - T.node(1, k)) : 0.0f) >= ga.dedup);
      if (dup) continue;
      T.add(1, nvalid, cand, PLAN_NO_PARENT);
      root_goal |= (uint32_t)nvalid << (4 * nvalid);
      nvalid++;
    }
    if (ga.goals_out) {
      float* const out = ga.goals_out + (size_t)row * NG * D;
      for (int g = 0; g < NG; g++)
        if (isd) out[(size_t)g * D + lane] = g < nvalid ? T.node(1, g) : 0.0f;
    }
    if (lane == 0) {
      if (ga.n_goals_out) ga.n_goals_out[row] = nvalid;
      if (ga.goal_stats) {
        int32_t* const st = ga.goal_stats + (size_t)row * 4;
        st[0] = tried; st[1] = conv; st[2] = rej; st[3] = iters;
      }
      if (gs)
        for (int g = 0; g < NG; g++) gs[g] = g < nvalid ? MIR_PLAN_OK : -1;
    }
  }
  // ---- the goals: limits, then clear(); the valid ones become Tb's roots in ascending g (NG < max_nodes: they fit)
  for (int g = 0; g < (POSE ? 0 : NG); g++) {
    int s = -1;  // behind the row's count, or never judged (the start failed)
    if (status == MIR_PLAN_OK && g < ng) {
      const float gv = isd ? a.goal[((size_t)row * NG + g) * D + dj] : 0.0f;
      const bool outside = isd && !(gv >= lo && gv <= hi);  // (a NaN or an infinity compares false: outside)
      if (__ballot(outside) != 0ull) s = MIR_PLAN_GOAL_OUT_OF_LIMITS;
      else if (!(r.clearance(gv) >= a.margin)) s = MIR_PLAN_GOAL_IN_COLLISION;
      else if (SELF && !(r.self_clearance() >= a.self_margin)) s = MIR_PLAN_GOAL_IN_SELF_COLLISION;
      else {
        s = MIR_PLAN_OK;
        T.add(1, nvalid, gv, PLAN_NO_PARENT);
        root_goal |= (uint32_t)g << (4 * nvalid);
        nvalid++;
      }
    }
    if (gs && lane == 0) gs[g] = s;
  }
  if (status == MIR_PLAN_OK && nvalid == 0) status = MIR_PLAN_NO_VALID_GOAL;
  // ---- the direct edge to the valid goals, nearest first
  if (status == MIR_PLAN_OK) {
    uint32_t tried = 0;
    for (int p = 0; p < nvalid; p++) {
      if (isd) L.qs[lane] = sv;
      WSYNC();
      float bd = INFINITY;
      int bi = 0x7fffffff;
      if (lane < nvalid && !((tried >> lane) & 1u)) {
        float acc = 0.0f;
        for (int j = 0; j < D; j++) {
          const float e = T.tree[((size_t)D + j) * MN + lane] - L.qs[j];
          acc = acc + e * e;
        }
        bd = acc;
        bi = lane;
      }
      const ArgMin m = wave_argmin(bd, bi);
      WSYNC();
      const int k = __builtin_amdgcn_readfirstlane(m.i);
      if (k < 0 || k >= nvalid) break;  // (every distance a NaN: no direct edge, the trees decide)
      tried |= 1u << k;
      const float gv = T.node(1, k);
      if (r.edge(sv, gv)) {
        if (isd) { L.poly[0][lane] = sv; L.poly[1][lane] = gv; }
        npoly = 2;
        gi = (int)((root_goal >> (4 * k)) & 15u);
        break;
      }
    }
  }
  // ---- the trees where they are needed (Tb starts as the forest of the valid goals), the polyline, the waypoints and the stores
  const int reached = plan_grow_and_store(r, T, row, env, sv, lo, hi, status, npoly, nvalid);
  if (reached >= 0) gi = (int)((root_goal >> (4 * reached)) & 15u);
  if (ga.goal_index && lane == 0) ga.goal_index[row] = gi;
}

}  // namespace

extern "C" int mir_goal_query_sizeof(void) { return (int)sizeof(MirGoalQuery); }

// what the two entry points share behind their own checks: the planner's fields, the outputs, the launch
static int goal_launch(const PlanCall& c, GoalArgs& a, long long R, const MirPlanQuery* q, int NG, bool pose, float* path, int32_t* status, float* poly,
                       int32_t* n_poly, int32_t* stats, int32_t* goal_index, int32_t* goal_status) {
  PlanArgs& p = a.p;
  p.W = q->num_waypoints; p.max_nodes = q->max_nodes; p.max_iter = q->max_iterations; p.smooth = q->smooth_passes; p.seed = q->seed;
  p.step = q->step; p.path = path; p.status = status; p.poly = poly; p.n_poly = n_poly; p.stats = stats;
  a.NG = NG; a.goal_index = goal_index; a.goal_status = goal_status;
  const size_t trees = (size_t)2 * (size_t)p.max_nodes * (4 * (size_t)p.D + 2);
  const auto kernel = pose ? pick_self_carry(c.self, c.carry, [](auto S, auto C) { return mir_goal_kernel<decltype(S)::value, decltype(C)::value, true>; })
                           : pick_self_carry(c.self, c.carry, [](auto S, auto C) { return mir_goal_kernel<decltype(S)::value, decltype(C)::value, false>; });
  return plan_launch(c, kernel, R, a, a.p, trees);
}

extern "C" int mir_plan_path_goals(MirHandle h, const MirPlanQuery* q, const MirSelfQuery* sq, const MirCarryQuery* cq, const MirGoalQuery* gq,
                                   const float* probes, const int32_t* probe_link, const int32_t* dof_qadr, const int64_t* env_idx, int32_t n_rows,
                                   const float* qpos_start, const float* grasp, const float* qpos_goals, const int32_t* n_goals, float* path,
                                   int32_t* status, float* poly, int32_t* n_poly, int32_t* stats, float* grasp_used, int32_t* goal_index,
                                   int32_t* goal_status, void* stream) {
  const char* const who = "mir_plan_path_goals";
  if (!gq || !qpos_goals || !path || !status) return query_error(MIR_E_INVALID, who, "null argument");
  if (gq->struct_size != (int32_t)sizeof(MirGoalQuery)) return query_error(MIR_E_INVALID, who, "struct_size is not sizeof(MirGoalQuery)");
  if (gq->flags) return query_error(MIR_E_INVALID, who, "unknown flag bit in MirGoalQuery");
  if (gq->max_goals < 1 || gq->max_goals > MIR_PLAN_MAX_GOALS) return query_error(MIR_E_INVALID, who, "max_goals outside 1 .. 8");
  if (!cq && grasp) return query_error(MIR_E_INVALID, who, "grasp without a MirCarryQuery");
  if (!cq && grasp_used) return query_error(MIR_E_INVALID, who, "grasp_used without a MirCarryQuery");
  const PlanCall c = plan_call(who, h, q, sq, sq != nullptr, cq, cq != nullptr, probes, probe_link, dof_qadr, env_idx, n_rows, qpos_start, grasp,
                               grasp_used, stream);
  GoalArgs a;
  memset(&a, 0, sizeof a);
  long long R = 0;
  const int rc = plan_front(c, true, a.p, R);
  if (rc != MIR_OK) return rc;
  if (q->max_nodes <= gq->max_goals) return query_error(MIR_E_INVALID, who, "max_nodes <= max_goals (the goals are the first nodes of their tree)");
  if (R * (long long)gq->max_goals * q->n_dofs > 0x7fffffffLL) return query_error(MIR_E_CAPACITY, who, "R x max_goals x n_dofs beyond 2^31 - 1");
  if (R == 0) return MIR_OK;
  a.p.goal = qpos_goals; a.n_goals = n_goals;
  return goal_launch(c, a, R, q, gq->max_goals, false, path, status, poly, n_poly, stats, goal_index, goal_status);
}

extern "C" int mir_pose_goal_query_sizeof(void) { return (int)sizeof(MirPoseGoalQuery); }

extern "C" int mir_plan_path_pose(MirHandle h, const MirPlanQuery* q, const MirSelfQuery* sq, const MirCarryQuery* cq, const MirPoseGoalQuery* gq,
                                  const float* probes, const int32_t* probe_link, const int32_t* dof_qadr, const int64_t* env_idx, int32_t n_rows,
                                  const float* qpos_start, const float* grasp, const float* target_pos, const float* target_quat,
                                  const MirIkOptions* opt, float* path, int32_t* status, float* poly, int32_t* n_poly, int32_t* stats,
                                  float* grasp_used, int32_t* goal_index, int32_t* goal_status, float* goals, int32_t* n_goals, int32_t* goal_stats,
                                  void* stream) {
  const char* const who = "mir_plan_path_pose";
  if (!gq || !target_pos || !path || !status) return query_error(MIR_E_INVALID, who, "null argument");
  if (gq->struct_size != (int32_t)sizeof(MirPoseGoalQuery)) return query_error(MIR_E_INVALID, who, "struct_size is not sizeof(MirPoseGoalQuery)");
  if (gq->flags) return query_error(MIR_E_INVALID, who, "unknown flag bit in MirPoseGoalQuery");
  if (gq->max_goals < 1 || gq->max_goals > MIR_PLAN_MAX_GOALS) return query_error(MIR_E_INVALID, who, "max_goals outside 1 .. 8");
  if (gq->max_samples < 1 || gq->max_samples >= 0x40000000) return query_error(MIR_E_INVALID, who, "max_samples outside 1 .. 2^30 - 1");
  if (!std::isfinite(gq->dedup) || gq->dedup < 0.0f) return query_error(MIR_E_INVALID, who, "dedup must be finite and >= 0 (0: resolution)");
  if (!cq && grasp) return query_error(MIR_E_INVALID, who, "grasp without a MirCarryQuery");
  if (!cq && grasp_used) return query_error(MIR_E_INVALID, who, "grasp_used without a MirCarryQuery");
  const PlanCall c = plan_call(who, h, q, sq, sq != nullptr, cq, cq != nullptr, probes, probe_link, dof_qadr, env_idx, n_rows, qpos_start, grasp,
                               grasp_used, stream);
  GoalArgs a;
  memset(&a, 0, sizeof a);
  long long R = 0;
  int rc = plan_front(c, true, a.p, R);
  if (rc != MIR_OK) return rc;
  if (q->max_nodes <= gq->max_goals) return query_error(MIR_E_INVALID, who, "max_nodes <= max_goals (the goals are the first nodes of their tree)");
  if (q->max_iterations >= 0x40000000) return query_error(MIR_E_INVALID, who, "max_iterations must stay below 2^30 (the counters above are the samples')");
  if (R * (long long)gq->max_goals * q->n_dofs > 0x7fffffffLL) return query_error(MIR_E_CAPACITY, who, "R x max_goals x n_dofs beyond 2^31 - 1");
  MirIkOptions o;
  if ((rc = ik_options(opt, true, who, o)) != MIR_OK) return rc;
  // the chain world -> link; its moving joints are those that are planned dofs (as mir_cartesian_path builds it)
  const int D = q->n_dofs;
  const ModelView mv(h);
  IkTree t;
  const char* what = "";
  const int32_t link = gq->link;
  if ((rc = build_ik_tree(mv, h->nbody, &link, 1, nullptr, "chain longer than 16 elements", t, &what)) != MIR_OK) return query_error(rc, who, what);
  uint8_t mask[MIR_MAX_DOF] = {0};
  for (int k = 0; k < t.n_arm; k++)
    for (int j = 0; j < D; j++)
      if (t.arm_qadr[k] == dof_qadr[j]) mask[k] = 1;
  if ((rc = build_ik_tree(mv, h->nbody, &link, 1, mask, "chain longer than 16 elements", t, &what)) != MIR_OK) return query_error(rc, who, what);
  if (!t.moving_cols) return query_error(MIR_E_INVALID, who, "no moving joint: no planned dof lies on the chain world -> link");
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
  a.userot = target_quat ? 1 : 0; a.max_iters = o.max_iters; a.respect_limits = o.respect_joint_limit; a.max_samples = gq->max_samples;
  a.damping2 = (float)(o.damping * o.damping); a.pos_tol = (float)o.pos_tol; a.rot_tol = (float)o.rot_tol;
  a.inv_pos_tol = (float)(1.0 / o.pos_tol); a.inv_rot_tol = (float)(1.0 / o.rot_tol); a.max_step = (float)o.max_step;
  a.dedup = gq->dedup > 0.0f ? gq->dedup : q->resolution;
  a.target_pos = target_pos; a.target_quat = target_quat; a.goals_out = goals; a.n_goals_out = n_goals; a.goal_stats = goal_stats;
  return goal_launch(c, a, R, q, gq->max_goals, true, path, status, poly, n_poly, stats, goal_index, goal_status);
}
