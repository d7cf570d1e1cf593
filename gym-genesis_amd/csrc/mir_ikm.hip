// mir_ikm.hip — batched multi-link damped-least-squares inverse kinematics: axis masks, dof subsets, restarts.
//
// What it is for: robot.inverse_kinematics(link, pos, quat, pos_mask=..., rot_mask=..., dofs_idx_local=..., max_samples=...) and
// robot.inverse_kinematics_multilink(links=[left_finger, right_finger], poss=..., quats=...) of Genesis.  The iteration is defined in
// include/mirigid.h (mir_inverse_kinematics_multilink) and restated by tests/ikm_ref.py.  A kernel of its own beside mir_ik.hip's; what
// the two have in common is in mir_ik_front.h, once: on the host the tree builder (a chain is the tree of one link) and the rows /
// options part of the arguments, on the device the row decode, the seed, an element's local transform, the log-map rotation error, the
// Jacobian column, the accept / reject / stall rule with its damping schedule and the step scaling.  Of its own here: the pointer-doubling
// pose scan over a tree, the one-axis orientation error, the limit rule, the row-per-lane solve and the samples.
//
// Mapping: as in mir_ik.hip, 16 lanes per output row (one DPP row), four rows per wave64.  Lane j owns element j of the UNION of the
// chains world -> link_l, a tree of <= 16 elements once the fixed elements that are no target are folded into their children (host
// side): its local joint transform, its world pose, its Jacobian column for all <= 24 task rows (registers).
//   poses      pointer doubling over the tree: every lane holds its pose relative to an ancestor and composes it with that
//              ancestor's, <= 4 steps of 7 lane gathers for a depth of <= 16 (the log-step scan of mir_ik.hip, on a tree; the
//              ancestor of every step is a table the host builds);
//   task error the poses of the <= 4 links come over the crossbar into every lane (7 gathers per link), every lane computes the same
//              error, metric and decisions from the same bits;
//   step       (J^T J + lambda^2 I) dq = J^T e, the form with one ROW PER LANE: lane i builds row i of the 16 x 16 matrix from row
//              broadcasts of the columns (v_fmac_f32_dpp), a register-row Gauss-Jordan elimination (16 pivots, one reciprocal with a
//              Newton step each) leaves dq_i in lane i.  No LDS, no scratch, no atomics: the J J^T form would keep a 24 x 24
//              factorisation (300 entries) in every lane.
// Every loop whose trip count depends on the row (iterations, samples) runs to a wave-uniform bound with predication; links, tree
// depth and masks are kernel arguments and so uniform anyway.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>

#include "mir_model.h"
#include "mir_scene.h"

#define G 16
#include "mir_dev.h"

#include "mir_query.h"

#include "mir_ik_front.h"

namespace {

constexpr int IKM_L = IK_LINKS;  // links per call

struct IkmArgs {
  IkElems el;                  // the union tree of the chains, parents before children
  int nsteps;                  // pointer-doubling steps
  int moving[G];               // the joint may move (on a chain and in the dof mask)
  signed char anc[4][G];       // the element whose pose is composed in front of mine in step s, -1: none (my pose is complete)
  int L, link_lane[IKM_L];     // links; the lane of each link's element
  unsigned anc_mask[IKM_L];    // bit j: element j lies on the chain of link l
  int pm[3], rot_mode, rot_axis;  // position mask; 0: no orientation rows, 1: one axis (rot_axis), 3: all three
  int max_samples;
  unsigned seed;
  unsigned long long moving_cols;  // bit k: column k is written by its moving joint's lane (the others are copies of the seed)
  IkRowArgs r;               // (r.target_quat is unused when rot_mode == 0)
  float* qpos_out;           // (rows, n_arm)
  float* err_out;            // (rows, L, 2) or null
  int32_t* iters_out;        // (rows) or null
  int32_t* sample_out;       // (rows) or null
};

// row i of J^T J: h[k] += J_i[r] J_k[r], the other lane's entry by row broadcast inside the fma
template <int K>
struct HAcc {
  static __device__ __forceinline__ void run(float (&h)[G], float jr) {
    h[K] = fmaf(jr, row_bcast<K>(jr), h[K]);
    HAcc<K + 1>::run(h, jr);
  }
};
template <>
struct HAcc<G> {
  static __device__ __forceinline__ void run(float (&)[G], float) {}
};

// Gauss-Jordan on register rows, all 16 pivots (mir_dev.h's GJ stops at 15, the step kernels' dof limit): lane i holds row i of the
// SPD matrix and b_i; on return b = x_i.  The pivot's reciprocal takes one more Newton step (the library is built with the
// approximate v_rcp_f32; the matrix can have a condition number of 1e6).
template <int K>
struct GJ16 {
  static __device__ __forceinline__ void run(float (&a)[G], float& b, int lane) {
    const float pk = row_bcast<K>(a[K]);
    float inv = __builtin_amdgcn_rcpf(pk);
    inv = fmaf(fmaf(-pk, inv, 1.0f), inv, inv);
    const float f = lane == K ? 1.0f - inv : a[K] * inv;
#pragma unroll
    for (int j = K + 1; j < G; j++) a[j] = fmaf(-f, row_bcast<K>(a[j]), a[j]);
    b = fmaf(-f, row_bcast<K>(b), b);
    if constexpr (K + 1 < G) GJ16<K + 1>::run(a, b, lane);
  }
};

__device__ __forceinline__ float ikm_uniform(unsigned seed, unsigned env, unsigned s, unsigned k) {
  unsigned x = seed * 0x9E3779B1u + env * 0x85EBCA77u + s * 0xC2B2AE3Du + k * 0x27D4EB2Fu + 0x165667B1u;
  x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
  return (float)(x >> 8) * 5.9604644775390625e-08f;  // 2^-24: exact
}

__global__ __launch_bounds__(64) void mir_ikm_kernel(IkmArgs a) {
  const int tid = threadIdx.x, lane = tid & 15;
  const IkRow t = ik_row_decode(a.r);
  const int row = t.row, env = t.env;
  const bool valid = t.valid;
  const int n = a.el.n, L = a.L;
  const int rowbase = tid & ~15;
  const bool onchain = lane < n;
  const int jt = onchain ? a.el.jtype[lane] : MIR_JNT_FIXED, qc = onchain ? a.el.qcol[lane] : -1;
  const V3 bpos = ld3(a.el.pos[lane]), baxis = ld3(a.el.axis[lane]);
  const Q4 bquat = ld4(a.el.quat[lane]);
  const bool scalar = onchain && qc >= 0 && (jt == MIR_JNT_REVOLUTE || jt == MIR_JNT_PRISMATIC);
  const bool moving = scalar && a.moving[lane];
  const float lo = a.el.lo[lane], hi = a.el.hi[lane];
  const bool limited = moving && a.el.limited[lane];
  const bool lim = limited && a.r.respect_limits;
  int src4[4];  // (lane_gather address of the element composed in front of mine in step s; -1: none)
#pragma unroll
  for (int s = 0; s < 4; s++) {
    const int an = a.anc[s][lane];
    src4[s] = an >= 0 ? (rowbase + an) << 2 : -1;
  }
  // every column that no lane moves is the seed, bit for bit; a moving joint's column is written once, at the end, by its lane
  for (int k = lane; k < a.r.n_arm; k += G)
    if (valid && !((a.moving_cols >> k) & 1ull)) a.qpos_out[(size_t)row * a.r.n_arm + k] = ik_seed(a.r, env, t.irow, k);
  const float q_seed = scalar ? ik_seed(a.r, env, t.irow, qc) : 0.0f;
  const bool userot = a.rot_mode != 0;
  const V3 ek = v3(a.rot_axis == 0 ? 1.0f : 0.0f, a.rot_axis == 1 ? 1.0f : 0.0f, a.rot_axis == 2 ? 1.0f : 0.0f);
  V3 tp[IKM_L], ta[IKM_L];
  Q4 tq[IKM_L];
#pragma unroll
  for (int l = 0; l < IKM_L; l++) {
    tp[l] = v3(0, 0, 0); ta[l] = v3(0, 0, 0); tq[l] = Q4{1, 0, 0, 0};
    if (l < L) {
      tp[l] = ld3(a.r.target_pos + ((size_t)t.prow * L + l) * 3);
      if (userot) {
        tq[l] = qnormalize(ld4(a.r.target_quat + ((size_t)t.qrow * L + l) * 4));
        ta[l] = qrot(tq[l], ek);
      }
    }
  }
  // the result so far (the first converged sample, else the smallest final metric) and the row's state over the samples
  float res_q = q_seed, res_m = 0.0f, res_ep[IKM_L] = {0, 0, 0, 0}, res_er[IKM_L] = {0, 0, 0, 0};
  int res_s = 0, total_iters = 0;
  bool finished = false;
  for (int s = 0; s < a.max_samples; s++) {
    if (s > 0 && !__any(!finished)) break;
    float q = q_seed;
    if (s > 0 && limited) q = lo + (hi - lo) * ikm_uniform(a.seed, (unsigned)env, (unsigned)s, (unsigned)qc);
    bool done = finished, conv = false;
    int my_iters = 0;
    float q_acc = q, g_acc = 0.0f;
    LmState lm = {a.r.damping2, 0, 0.0f};
    float epn[IKM_L] = {0, 0, 0, 0}, ern[IKM_L] = {0, 0, 0, 0};
    float J[6 * IKM_L], e[6 * IKM_L];
#pragma unroll
    for (int r = 0; r < 6 * IKM_L; r++) J[r] = e[r] = 0.0f;
    for (int it = 0; it <= a.r.max_iters; it++) {
      // ---- local transform of my element (identity off the tree) at the CANDIDATE q ...
      const Pose x0 = ik_elem_local(onchain, jt, bpos, bquat, baxis, q);
      V3 P = x0.P;
      Q4 Qx = x0.Qx;
      // ... then my world pose by pointer doubling: (P, Q) is my pose relative to an ancestor; composing it with that ancestor's
      // pose relative to ITS ancestor doubles the distance covered (every lane gathers before any lane updates)
#pragma unroll
      for (int st = 0; st < 4; st++) {
        if (st < a.nsteps) {
          const int sa = src4[st], ad = sa >= 0 ? sa : (tid << 2);
          const V3 pp = gather3(ad, P);
          const Q4 pq = gather4(ad, Qx);
          if (sa >= 0) {
            P = pp + qrot(pq, P);
            Qx = qmul(pq, Qx);
          }
        }
      }
      // ---- task-space error of the candidate, every lane redundantly from the links' gathered poses
      V3 pe[IKM_L], ep[IKM_L], er[IKM_L], aw[IKM_L];
      float epn_c[IKM_L], ern_c[IKM_L], metric = 0.0f;
#pragma unroll
      for (int l = 0; l < IKM_L; l++) {
        pe[l] = ep[l] = er[l] = aw[l] = v3(0, 0, 0);
        epn_c[l] = ern_c[l] = 0.0f;
        if (l < L) {
          const int ad = (rowbase + a.link_lane[l]) << 2;
          pe[l] = gather3(ad, P);
          const V3 dp = tp[l] - pe[l];
          ep[l] = v3(a.pm[0] ? dp.x : 0.0f, a.pm[1] ? dp.y : 0.0f, a.pm[2] ? dp.z : 0.0f);
          if (userot) {
            const Q4 qe = gather4(ad, Qx);
            if (a.rot_mode == 3) {
              er[l] = ik_rot_error(tq[l], qe);
            } else {
              // one axis: turn the link's axis k onto the target's about their common normal; rotation about the axis is free
              aw[l] = qrot(qe, ek);
              const V3 c = cross(aw[l], ta[l]);
              const float sn = sqrtf(dot(c, c));
              const float k = sn < 1e-9f ? 0.0f : atan2f(sn, dot(aw[l], ta[l])) / sn;
              er[l] = v3(k * c.x, k * c.y, k * c.z);
            }
          }
          epn_c[l] = sqrtf(dot(ep[l], ep[l]));
          ern_c[l] = sqrtf(dot(er[l], er[l]));
          metric += epn_c[l] * a.r.inv_pos_tol + ern_c[l] * a.r.inv_rot_tol;
        }
      }
      if (!done) {
        if (lm_accepts(lm, metric, it == 0)) {
          lm = lm_accept(lm, metric, it == 0, a.r.damping2);
          q_acc = q;
          float g = 0.0f;
          conv = true;
#pragma unroll
          for (int l = 0; l < IKM_L; l++) {
            if (l < L) {
              epn[l] = epn_c[l]; ern[l] = ern_c[l];
              conv = conv && epn[l] < a.r.pos_tol && ern[l] < a.r.rot_tol;
              e[6 * l + 0] = ep[l].x; e[6 * l + 1] = ep[l].y; e[6 * l + 2] = ep[l].z;
              e[6 * l + 3] = er[l].x; e[6 * l + 4] = er[l].y; e[6 * l + 5] = er[l].z;
              // my Jacobian column for link l at the accepted iterate
              const JacColumn c = ik_jac_column(moving && ((a.anc_mask[l] >> lane) & 1u), jt, Qx, P, baxis, pe[l]);
              const V3 jv = c.jv;
              V3 jw = c.jw;
              if (a.rot_mode == 1) jw = jw - dot(aw[l], jw) * aw[l];
              if (!userot) jw = v3(0, 0, 0);
              J[6 * l + 0] = a.pm[0] ? jv.x : 0.0f; J[6 * l + 1] = a.pm[1] ? jv.y : 0.0f; J[6 * l + 2] = a.pm[2] ? jv.z : 0.0f;
              J[6 * l + 3] = jw.x; J[6 * l + 4] = jw.y; J[6 * l + 5] = jw.z;
#pragma unroll
              for (int r = 0; r < 6; r++) g = fmaf(J[6 * l + r], e[6 * l + r], g);
            }
          }
          // the limit rule: a joint that sits on a limit (the clamp produced the value: the comparison is exact) and whose gradient
          // component pushes it further out is taken out of the step until the next accepted iterate
          if (lim && ((q == lo && g < 0.0f) || (q == hi && g > 0.0f))) {
            g = 0.0f;
#pragma unroll
            for (int r = 0; r < 6 * IKM_L; r++) J[r] = 0.0f;
          }
          g_acc = g;
        } else {
          lm = lm_reject(lm, a.r.damping2);
        }
        if (conv || lm_stalled(lm)) done = true;
      }
      if (it == a.r.max_iters) break;
      if (!__any(!done)) break;
      // ---- row `lane` of J^T J + lambda^2 I (J, e: the accepted iterate's), then dq by elimination
      float H[G];
#pragma unroll
      for (int k = 0; k < G; k++) H[k] = k == lane ? lm.lam2 : 0.0f;
#pragma unroll
      for (int l = 0; l < IKM_L; l++) {
        if (l < L) {
#pragma unroll
          for (int r = 0; r < 6; r++)
            if (r < 3 ? a.pm[r] != 0 : userot) HAcc<0>::run(H, J[6 * l + r]);
        }
      }
      float dq = g_acc;
      GJ16<0>::run(H, dq, lane);
      const float sc = ik_step_scale(dq, a.r.max_step);
      if (!done) my_iters = it + 1;
      q = q_acc;
      if (moving && !done) {
        q = q_acc + sc * dq;
        if (lim) q = fminf(fmaxf(q, lo), hi);
      }
    }
    if (!finished) {
      total_iters += my_iters;
      if (conv || s == 0 || lm.m_acc < res_m) {
        res_q = q_acc; res_m = lm.m_acc; res_s = s;
#pragma unroll
        for (int l = 0; l < IKM_L; l++) { res_ep[l] = epn[l]; res_er[l] = ern[l]; }
      }
      finished = conv;
    }
  }
  if (valid && moving) a.qpos_out[(size_t)row * a.r.n_arm + qc] = res_q;
  if (valid && lane == 0) {
    if (a.iters_out) a.iters_out[row] = total_iters;
    if (a.sample_out) a.sample_out[row] = res_s;
    if (a.err_out) {
#pragma unroll
      for (int l = 0; l < IKM_L; l++)
        if (l < L) {
          a.err_out[((size_t)row * L + l) * 2] = res_ep[l];
          a.err_out[((size_t)row * L + l) * 2 + 1] = res_er[l];
        }
    }
  }
}

}  // namespace

extern "C" int mir_ik_multi_sizeof(void) { return (int)sizeof(MirIkMulti); }

extern "C" int mir_inverse_kinematics_multilink(MirHandle h, const MirIkMulti* mq, const float* target_pos, const float* target_quat,
                                                const float* init_qpos, const MirIkOptions* opt, float* qpos_out, float* err_out,
                                                int32_t* iters_out, int32_t* sample_out, void* stream) {
  const char* who = "mir_inverse_kinematics_multilink";
  if (!h || !mq || !target_pos || !qpos_out) return query_error(MIR_E_INVALID, who, "null argument");
  if (mq->struct_size != (int32_t)sizeof(MirIkMulti)) return query_error(MIR_E_INVALID, who, "struct_size");
  if (int rc = ik_check_rows(&mq->rows, who)) return rc;
  if (mq->n_links < 1 || mq->n_links > IKM_L) return query_error(MIR_E_INVALID, who, "n_links outside 1 .. 4");
  if (mq->max_samples < 1) return query_error(MIR_E_INVALID, who, "max_samples < 1");
  const int nrot = (mq->rot_mask[0] ? 1 : 0) + (mq->rot_mask[1] ? 1 : 0) + (mq->rot_mask[2] ? 1 : 0);
  const int npos = (mq->pos_mask[0] ? 1 : 0) + (mq->pos_mask[1] ? 1 : 0) + (mq->pos_mask[2] ? 1 : 0);
  if (nrot == 2) return query_error(MIR_E_INVALID, who, "rot_mask aligns 0, 1 or all 3 axes");
  const int rot_mode = target_quat ? nrot : 0;
  if (npos == 0 && rot_mode == 0) return query_error(MIR_E_INVALID, who, "the masks select no task row");
  MirIkOptions o;
  if (int rc = ik_options(opt, true, who, o)) return rc;
  // the union of the chains world -> link_l
  IkTree t;
  const char* what;
  if (int rc = build_ik_tree(ModelView(h), h->nbody, mq->link_body, mq->n_links, mq->dof_mask, "the union of the chains has more than 16 elements", t, &what))
    return query_error(rc, who, what);
  IkmArgs a;
  memset(&a, 0, sizeof a);
  if (int rc = fill_ik_rows(h, &mq->rows, o, t, true, who, target_pos, target_quat, init_qpos, a.r)) return rc;
  if (a.r.n_rows == 0) return MIR_OK;
  a.el = t.el; a.nsteps = t.nsteps; a.moving_cols = t.moving_cols;
  memcpy(a.moving, t.moving, sizeof a.moving);
  memcpy(a.anc, t.anc, sizeof a.anc);
  a.L = mq->n_links;
  for (int l = 0; l < mq->n_links; l++) { a.link_lane[l] = t.link_lane[l]; a.anc_mask[l] = t.anc_mask[l]; }
  for (int k = 0; k < 3; k++) a.pm[k] = mq->pos_mask[k] ? 1 : 0;
  a.rot_mode = rot_mode;
  a.rot_axis = mq->rot_mask[0] ? 0 : (mq->rot_mask[1] ? 1 : 2);
  a.max_samples = mq->max_samples; a.seed = mq->seed;
  a.qpos_out = qpos_out; a.err_out = err_out; a.iters_out = iters_out; a.sample_out = sample_out;
  return launch_rows(h, mir_ikm_kernel, (a.r.n_rows + 3) / 4, stream, a);
}
