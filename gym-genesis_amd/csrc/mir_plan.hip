// mir_plan.hip — batched collision-checked motion planning (mir_plan_path) and the swept clearance of a given trajectory
// (mir_path_clearance); include/mirigid.h, DESIGN.md "Motion planning".
//
// What it serves: for a list of envs, one launch takes each row's arm from a start configuration to a goal configuration through
// configurations whose sphere model (probe spheres that ride on links, as in mir_signed_distance) keeps `margin` from every geom that is
// not skipped: RRT-Connect in the space of the D planned dofs, shortcut smoothing, resampling to W waypoints.  The second entry point
// streams a caller's trajectory through the same configuration check and reports the lowest clearance per segment.
//
// Mapping: one workgroup of one wave64 per row, as mir_dist.hip.  WSYNC() only; nothing travels from lane to lane through global memory.
//   The row's env, the forward kinematics, the probe centres, the sphere-list entries, the wave reductions and the host's row checks and
//   argument filling are the front end shared with mir_dist.hip and mir_self.hip: mir_sphere_front.h.
//   Row set-up.  The row's full start configuration (nq floats) goes to LDS; forward kinematics with lane = body (sphere_poses_fk); the
//   geom records are built ONCE (dist_build_records): the host guarantees that every geom that is tested rides on a body without a
//   planned dof above it.
//   clear(q).  Lane j < D writes planned dof j into the LDS row; the bodies below a planned dof (bit 15 of their word) are recomputed,
//   every other body keeps its pose; the probes in chunks of 64 through dist_probe_min; the wave minimum of (distance - radius).
//   A configuration is a float per lane: lane j holds dof j, lanes >= D hold 0.
//   Trees.  Two trees in dynamic LDS: coordinates [tree][dof][node] (lanes stride over nodes: conflict free) and a 16-bit parent.
// Bounds: every loop is bounded by max_iterations, max_nodes, the 4096 samples of an edge (PLAN_MAX_SUB: n_sub is clamped), the
//   MIR_PLAN_MAX_POLY nodes of a polyline, smooth_passes, num_waypoints or (mir_path_clearance) the K points of the caller's path.  No
//   input can keep a wave running: a configuration or a geom pose that is not finite counts as blocked, a nearest-node index is
//   clamped to the tree.
// Stores: plain dword stores by lanes 0 .. D-1 (or lane 0).  No atomics, no scratch, no cross-wave barrier.
//
// Self-collision (mir_plan_path_self, mir_path_clearance_self): both kernels are templates on SELF; the instantiation without it is the
//   code of mir_plan_path / mir_path_clearance.  With it, clearance_at_poses() also stores every probe's world centre and radius to a
//   sphere list in dynamic LDS (behind the trees), the E extra probes behind the first N included; self_clearance() walks it: lane =
//   probe i in chunks of 64, a loop over j through the list (self_probe_min of mir_self_body.h: a chunk of the list per lane, sphere j
//   to all lanes by v_readlane), the pair filter as one bit of link_mask[link_i], one wave reduction.  s(i, j) is symmetric, so chunk
//   c of the i's meets the j's from chunk c on.  Bounded by N + E; the mask travels in the kernel arguments.
//
// Carried object (mir_plan_path_carry, mir_path_clearance_carry): a further template parameter, CARRY; the four instantiations without
//   it are the code of the four entry points above.  With it, plan_setup() takes the row's grasp transform (the carried body's pose in
//   the attach link's frame: from the start row's forward kinematics, or the caller's row) into seven registers (the same value in every lane), and the
//   partial fk() ends with one more step: lane 0 overwrites the carried body's pose in LDS by link o grasp.  The probes that ride on
//   the carried body then follow the hand through clearance_at_poses() and self_clearance() unchanged.  A grasp that is not finite or
//   has a zero quaternion sets `bad` (and blocks the self test): every clearance of the row is -INFINITY.
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

#include "mir_plan_row.h"  // (PlanArgs, PlanLds, div_refined, PlanRow, plan_setup, PlanCall, plan_front and the launch: shared with mir_cart.hip)

namespace {

// (the random numbers u(env, c, j): plan_u of mir_plan_row.h)
extern __shared__ float plan_dyn[];

template <bool SELF, bool CARRY>
__global__ __launch_bounds__(64) void mir_plan_kernel(PlanArgs a) {
  __shared__ PlanLds L;
  const int lane = threadIdx.x, row = blockIdx.x, D = a.D, MN = a.max_nodes;
  const int env = sphere_row_env(a.r, row);
  float* const tree = plan_dyn;                                                        // [2][D][MN]
  uint16_t* const parent = reinterpret_cast<uint16_t*>(plan_dyn + (size_t)2 * D * MN);  // [2][MN]
  PlanRow<SELF, CARRY> r{a, L, lane, 0, 0, false, plan_dyn + (size_t)(2 * D + 1) * MN, SELF_LIST};  // (2 MN 16-bit parents are MN floats)
  plan_setup(r, row, env);
  const bool isd = lane < D;
  const int dj = isd ? lane : 0;
  const float lo = a.lo[dj], hi = a.hi[dj];
  const float sv = isd ? L.qrow[a.qadr[dj]] : 0.0f;
  const float gv = isd ? a.goal[(size_t)row * D + dj] : 0.0f;
  WSYNC();

  auto node = [&](int t, int n) { return isd ? tree[((size_t)t * D + dj) * MN + n] : 0.0f; };
  auto add = [&](int t, int n, float v, int par) {
    if (isd) tree[((size_t)t * D + dj) * MN + n] = v;
    if (lane == 0) parent[t * MN + n] = (uint16_t)par;
    WSYNC();
  };
  // nearest node of tree t (cnt nodes) to q: squared L2 distance over the planned dofs, j ascending; the lower index wins a tie
  auto nearest = [&](int t, int cnt, float q, float& d2) {
    if (isd) L.qs[lane] = q;
    WSYNC();
    float bd = INFINITY;
    int bi = 0x7fffffff;
    for (int n = lane; n < cnt; n += 64) {
      float acc = 0.0f;
      for (int j = 0; j < D; j++) {
        const float e = tree[((size_t)t * D + j) * MN + n] - L.qs[j];
        acc = acc + e * e;
      }
      if (acc < bd) { bd = acc; bi = n; }  // (nodes ascend: the lower index keeps a tie)
    }
    const ArgMin m = wave_argmin(bd, bi);
    WSYNC();
    d2 = m.v;
    bi = __builtin_amdgcn_readfirstlane(m.i);
    return bi < cnt ? bi : 0;
  };

  int status = MIR_PLAN_OK, iterations = 0, na = 1, nb = 1, npoly = 1;
  const bool outside = isd && !(gv >= lo && gv <= hi);
  if (__ballot(outside) != 0ull) status = MIR_PLAN_GOAL_OUT_OF_LIMITS;
  else if (!(r.clearance(sv) >= a.margin)) status = MIR_PLAN_START_IN_COLLISION;
  else if (SELF && !(r.self_clearance() >= a.self_margin)) status = MIR_PLAN_START_IN_SELF_COLLISION;
  else if (!(r.clearance(gv) >= a.margin)) status = MIR_PLAN_GOAL_IN_COLLISION;
  else if (SELF && !(r.self_clearance() >= a.self_margin)) status = MIR_PLAN_GOAL_IN_SELF_COLLISION;
  else if (r.edge(sv, gv)) {
    if (isd) { L.poly[0][lane] = sv; L.poly[1][lane] = gv; }
    npoly = 2;
  } else {
    add(0, 0, sv, PLAN_NO_PARENT);
    add(1, 0, gv, PLAN_NO_PARENT);
    status = MIR_PLAN_ITERATION_LIMIT;
    for (int it = 0; it < a.max_iter; it++) {
      iterations = it + 1;
      const int t = it & 1, o = t ^ 1;
      int ct = t ? nb : na, co = t ? na : nb;
      const float qr = isd ? lo + plan_u(a.seed, (uint32_t)env, (uint32_t)it, (uint32_t)dj) * (hi - lo) : 0.0f;
      float d2;
      const int near = nearest(t, ct, qr, d2);
      const float nv = node(t, near);
      const float qn = nv + fminf(1.0f, a.step / sqrtf(d2)) * (qr - nv);
      if (!r.edge(nv, qn)) continue;
      if (ct >= MN) { status = MIR_PLAN_NODE_LIMIT; break; }
      add(t, ct, qn, near);
      const int inew = ct++;
      // connect: from the other tree's nearest node towards q_new, at most `step` at a time
      int ci = nearest(o, co, qn, d2);
      float cv = node(o, ci);
      bool met = false, full = false;
      for (int k = 0; k < MN; k++) {  // (every pass adds a node or leaves)
        const float diff = qn - cv;
        const float d = sqrtf(r.norm2(diff));
        const bool last = d <= a.step;
        const float tv = last ? qn : cv + (a.step / d) * diff;
        if (!r.edge(cv, tv)) break;
        if (co >= MN) { full = true; break; }
        add(o, co, tv, ci);
        ci = co++;
        cv = tv;
        if (last) { met = true; break; }
      }
      na = t ? co : ct;
      nb = t ? ct : co;
      if (full) { status = MIR_PLAN_NODE_LIMIT; break; }
      if (!met) continue;
      // extract: the parents of both trees into one polyline, start first
      const int ia = t ? ci : inew, ib = t ? inew : ci;
      int la = 0, lb = 0;
      for (int n = ia; n != PLAN_NO_PARENT && la <= MN; n = __builtin_amdgcn_readfirstlane((int)parent[n])) la++;
      for (int n = ib; n != PLAN_NO_PARENT && lb <= MN; n = __builtin_amdgcn_readfirstlane((int)parent[MN + n])) lb++;
      if (la + lb - 1 > MIR_PLAN_MAX_POLY) { status = MIR_PLAN_PATH_TOO_LONG; break; }
      int n = ia;
      for (int p = la - 1; p >= 0; p--) {
        if (isd) L.poly[p][lane] = node(0, n);
        n = __builtin_amdgcn_readfirstlane((int)parent[n]);
      }
      n = __builtin_amdgcn_readfirstlane((int)parent[MN + ib]);  // (the meeting node is in both trees: once)
      for (int p = la; p < la + lb - 1; p++) {
        if (isd) L.poly[p][lane] = node(1, n);
        n = __builtin_amdgcn_readfirstlane((int)parent[MN + n]);
      }
      npoly = la + lb - 1;
      status = MIR_PLAN_OK;
      break;
    }
  }
  if (status != MIR_PLAN_OK) {  // the arm stays put: the start W times, a polyline of one node
    if (isd) L.poly[0][lane] = sv;
    npoly = 1;
  }
  WSYNC();

  // ---- smooth: shortcuts between two nodes of the polyline
  for (int s = 0; s < a.smooth && npoly >= 3; s++) {
    const float u0 = plan_u(a.seed, (uint32_t)env, 0x80000000u | (uint32_t)s, 0u), u1 = plan_u(a.seed, (uint32_t)env, 0x80000000u | (uint32_t)s, 1u);
    const int i = min((int)(u0 * (float)(npoly - 2)), npoly - 3);
    const int j = i + 2 + min((int)(u1 * (float)(npoly - 2 - i)), npoly - 3 - i);
    if (!r.edge(isd ? L.poly[i][lane] : 0.0f, isd ? L.poly[j][lane] : 0.0f)) continue;
    for (int k = j; k < npoly; k++)  // (every lane moves its own column)
      if (isd) L.poly[i + 1 + k - j][lane] = L.poly[k][lane];
    npoly -= j - i - 1;
  }
  WSYNC();

  // ---- resample: W configurations at equal steps of the cumulative L2 length
  float total = 0.0f;
  for (int k = 0; k + 1 < npoly; k++) {
    const float d = sqrtf(r.norm2(isd ? L.poly[k + 1][lane] - L.poly[k][lane] : 0.0f));
    if (lane == 0) L.cum[k] = total;
    total = total + d;
    if (lane == 0) L.cum[k + 1] = total;
  }
  WSYNC();
  {
    float* const out = a.path + (size_t)row * a.W * D;
    int k = 0;
    for (int w = 0; w < a.W; w++) {
      float q;
      if (npoly == 1 || w == 0) q = isd ? L.poly[0][lane] : 0.0f;
      else if (w == a.W - 1) q = isd ? L.poly[npoly - 1][lane] : 0.0f;
      else {
        const float f = div_refined((float)w, (float)(a.W - 1));
        float t = f;  // (a polyline of one segment: the fraction itself, no length enters)
        if (npoly > 2) {
          const float s = f * total;
          while (k < npoly - 2 && L.cum[k + 1] <= s) k++;
          const float c0 = L.cum[k], len = L.cum[k + 1] - c0;
          t = len > 0.0f ? fminf(div_refined(s - c0, len), 1.0f) : 0.0f;
        }
        const float p0 = isd ? L.poly[k][lane] : 0.0f, p1 = isd ? L.poly[k + 1][lane] : 0.0f;
        q = p0 + t * (p1 - p0);
      }
      if (isd) out[(size_t)w * D + lane] = q;
    }
  }
  if (a.poly) {
    float* const out = a.poly + (size_t)row * MIR_PLAN_MAX_POLY * D;
    for (int k = 0; k < MIR_PLAN_MAX_POLY; k++)
      if (isd) out[(size_t)k * D + lane] = k < npoly ? L.poly[k][lane] : 0.0f;
  }
  if (lane == 0) {
    a.status[row] = status;
    if (a.n_poly) a.n_poly[row] = npoly;
    if (a.stats) {
      int32_t* const st = a.stats + (size_t)row * 4;
      st[0] = iterations; st[1] = na; st[2] = nb; st[3] = r.checked;
    }
  }
}

// the swept check on its own: every sample of the edge rule on every segment of the caller's path, no early exit
template <bool SELF, bool CARRY>
__global__ __launch_bounds__(64) void mir_path_clear_kernel(PlanArgs a) {
  __shared__ PlanLds L;
  const int lane = threadIdx.x, row = blockIdx.x, D = a.D;
  PlanRow<SELF, CARRY> r{a, L, lane, 0, 0, false, plan_dyn, SELF_LIST};
  plan_setup(r, row, sphere_row_env(a.r, row));
  const bool isd = lane < D;
  const float* const p = a.goal + (size_t)row * a.K * D;
  float rmin = INFINITY, rself = INFINITY;
  int first = -1;
  float av = isd ? p[lane] : 0.0f;
  for (int k = 0; k + 1 < a.K; k++) {
    const float bv = isd ? p[(size_t)(k + 1) * D + lane] : 0.0f;
    float smin = k == 0 ? r.clearance(av) : INFINITY;  // (a segment's first point counts only for segment 0)
    float sself = INFINITY;
    if constexpr (SELF)
      if (k == 0) sself = r.self_clearance();
    const float diff = bv - av;
    const int n = r.n_sub(diff);
    for (int i = 1; i <= n; i++) {
      smin = fminf(smin, r.clearance(PlanRow<SELF, CARRY>::sample(av, bv, diff, i, n)));
      if constexpr (SELF) sself = fminf(sself, r.self_clearance());
    }
    if (a.seg_min && lane == 0) a.seg_min[(size_t)row * (a.K - 1) + k] = smin;
    rmin = fminf(rmin, smin);
    bool blocked = smin < a.margin;
    if constexpr (SELF) {
      if (a.seg_self_min && lane == 0) a.seg_self_min[(size_t)row * (a.K - 1) + k] = sself;
      rself = fminf(rself, sself);
      blocked = blocked || sself < a.self_margin;
    }
    if (first < 0 && blocked) first = k;
    av = bv;
  }
  if (lane == 0) {
    if (a.row_min) a.row_min[row] = rmin;
    if constexpr (SELF)
      if (a.row_self_min) a.row_self_min[row] = rself;
    if (a.first_blocked) a.first_blocked[row] = first;
  }
}

// ---- host (the call description PlanCall with plan_call, plan_front, pick_self_carry and plan_launch, which every entry point
// shares: mir_plan_row.h)
int plan_entry(const PlanCall& c, const float* qpos_goal, float* path, int32_t* status, float* poly, int32_t* n_poly, int32_t* stats) {
  if (!qpos_goal || !path || !status) return query_error(MIR_E_INVALID, c.who, "null argument");
  PlanArgs a;
  long long R = 0;
  const int rc = plan_front(c, true, a, R);
  if (rc != MIR_OK || R == 0) return rc;
  a.W = c.q->num_waypoints; a.max_nodes = c.q->max_nodes; a.max_iter = c.q->max_iterations; a.smooth = c.q->smooth_passes; a.seed = c.q->seed;
  a.step = c.q->step; a.goal = qpos_goal; a.path = path; a.status = status; a.poly = poly; a.n_poly = n_poly; a.stats = stats;
  const size_t trees = (size_t)2 * (size_t)a.max_nodes * (4 * (size_t)a.D + 2);
  const auto kernel = pick_self_carry(c.self, c.carry, [](auto S, auto C) { return mir_plan_kernel<decltype(S)::value, decltype(C)::value>; });
  return plan_launch(c, kernel, R, a, a, trees);
}

int path_clear_entry(const PlanCall& c, const float* paths, int32_t K, float* seg_min, float* seg_self_min, float* row_min, float* row_self_min,
                     int32_t* row_first_blocked) {
  if (!paths) return query_error(MIR_E_INVALID, c.who, "null argument");
  if (K < 2) return query_error(MIR_E_INVALID, c.who, "K < 2");
  if (!c.self && (seg_self_min || row_self_min)) return query_error(MIR_E_INVALID, c.who, "seg_self_min / row_self_min without a MirSelfQuery");
  PlanArgs a;
  long long R = 0;
  const int rc = plan_front(c, false, a, R);
  if (rc != MIR_OK || R == 0 || (!seg_min && !seg_self_min && !row_min && !row_self_min && !row_first_blocked && !c.grasp_used)) return rc;
  a.K = K; a.goal = paths; a.seg_min = seg_min; a.row_min = row_min; a.first_blocked = row_first_blocked;
  a.seg_self_min = seg_self_min; a.row_self_min = row_self_min;
  const auto kernel = pick_self_carry(c.self, c.carry, [](auto S, auto C) { return mir_path_clear_kernel<decltype(S)::value, decltype(C)::value>; });
  return plan_launch(c, kernel, R, a, a, 0);
}

}  // namespace

extern "C" int mir_plan_query_sizeof(void) { return (int)sizeof(MirPlanQuery); }
extern "C" int mir_self_query_sizeof(void) { return (int)sizeof(MirSelfQuery); }
extern "C" int mir_carry_query_sizeof(void) { return (int)sizeof(MirCarryQuery); }

// (the _self forms: self with a possibly null sq, their refusal; the _carry forms: a null sq is "no self test")
extern "C" int mir_plan_path(MirHandle h, const MirPlanQuery* q, const float* probes, const int32_t* probe_link, const int32_t* dof_qadr,
                             const int64_t* env_idx, int32_t n_rows, const float* qpos_start, const float* qpos_goal, float* path,
                             int32_t* status, float* poly, int32_t* n_poly, int32_t* stats, void* stream) {
  const PlanCall c = plan_call("mir_plan_path", h, q, nullptr, false, nullptr, false, probes, probe_link, dof_qadr, env_idx, n_rows, qpos_start,
                               nullptr, nullptr, stream);
  return plan_entry(c, qpos_goal, path, status, poly, n_poly, stats);
}

extern "C" int mir_plan_path_self(MirHandle h, const MirPlanQuery* q, const MirSelfQuery* sq, const float* probes, const int32_t* probe_link,
                                  const int32_t* dof_qadr, const int64_t* env_idx, int32_t n_rows, const float* qpos_start, const float* qpos_goal,
                                  float* path, int32_t* status, float* poly, int32_t* n_poly, int32_t* stats, void* stream) {
  const PlanCall c = plan_call("mir_plan_path_self", h, q, sq, true, nullptr, false, probes, probe_link, dof_qadr, env_idx, n_rows, qpos_start,
                               nullptr, nullptr, stream);
  return plan_entry(c, qpos_goal, path, status, poly, n_poly, stats);
}

extern "C" int mir_path_clearance(MirHandle h, const MirPlanQuery* q, const float* probes, const int32_t* probe_link, const int32_t* dof_qadr,
                                  const int64_t* env_idx, int32_t n_rows, const float* qpos_start, const float* paths, int32_t K,
                                  float* seg_min, float* row_min, int32_t* row_first_blocked, void* stream) {
  const PlanCall c = plan_call("mir_path_clearance", h, q, nullptr, false, nullptr, false, probes, probe_link, dof_qadr, env_idx, n_rows,
                               qpos_start, nullptr, nullptr, stream);
  return path_clear_entry(c, paths, K, seg_min, /*seg_self_min*/ nullptr, row_min, /*row_self_min*/ nullptr, row_first_blocked);
}

extern "C" int mir_path_clearance_self(MirHandle h, const MirPlanQuery* q, const MirSelfQuery* sq, const float* probes, const int32_t* probe_link,
                                       const int32_t* dof_qadr, const int64_t* env_idx, int32_t n_rows, const float* qpos_start,
                                       const float* paths, int32_t K, float* seg_min, float* seg_self_min, float* row_min, float* row_self_min,
                                       int32_t* row_first_blocked, void* stream) {
  const PlanCall c = plan_call("mir_path_clearance_self", h, q, sq, true, nullptr, false, probes, probe_link, dof_qadr, env_idx, n_rows,
                               qpos_start, nullptr, nullptr, stream);
  return path_clear_entry(c, paths, K, seg_min, seg_self_min, row_min, row_self_min, row_first_blocked);
}

extern "C" int mir_plan_path_carry(MirHandle h, const MirPlanQuery* q, const MirSelfQuery* sq, const MirCarryQuery* cq, const float* probes,
                                   const int32_t* probe_link, const int32_t* dof_qadr, const int64_t* env_idx, int32_t n_rows, const float* qpos_start,
                                   const float* grasp, const float* qpos_goal, float* path, int32_t* status, float* poly, int32_t* n_poly,
                                   int32_t* stats, float* grasp_used, void* stream) {
  const PlanCall c = plan_call("mir_plan_path_carry", h, q, sq, sq != nullptr, cq, true, probes, probe_link, dof_qadr, env_idx, n_rows, qpos_start,
                               grasp, grasp_used, stream);
  return plan_entry(c, qpos_goal, path, status, poly, n_poly, stats);
}

extern "C" int mir_path_clearance_carry(MirHandle h, const MirPlanQuery* q, const MirSelfQuery* sq, const MirCarryQuery* cq, const float* probes,
                                        const int32_t* probe_link, const int32_t* dof_qadr, const int64_t* env_idx, int32_t n_rows,
                                        const float* qpos_start, const float* grasp, const float* paths, int32_t K, float* seg_min, float* seg_self_min,
                                        float* row_min, float* row_self_min, int32_t* row_first_blocked, float* grasp_used, void* stream) {
  const PlanCall c = plan_call("mir_path_clearance_carry", h, q, sq, sq != nullptr, cq, true, probes, probe_link, dof_qadr, env_idx, n_rows,
                               qpos_start, grasp, grasp_used, stream);
  return path_clear_entry(c, paths, K, seg_min, seg_self_min, row_min, row_self_min, row_first_blocked);
}
