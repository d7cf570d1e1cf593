// mir_ikm.hip — batched multi-link damped-least-squares inverse kinematics: axis masks, dof subsets, restarts.
//
// What it is for: robot.inverse_kinematics(link, pos, quat, pos_mask=..., rot_mask=..., dofs_idx_local=..., max_samples=...) and
// robot.inverse_kinematics_multilink(links=[left_finger, right_finger], poss=..., quats=...) of Genesis.  The iteration is defined in
// include/mirigid.h (mir_inverse_kinematics_multilink) and restated by tests/ikm_ref.py.  A kernel of its own: mir_ik.hip is not
// touched and shares no code with this file (its phases are copied here, not factored out: DESIGN.md, operational-space section).
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

namespace {

constexpr int IKM_L = 4;  // links per call

struct IkmTree {
  int n, nsteps;               // elements of the union tree (parents before children); pointer-doubling steps
  int jtype[G], qcol[G];       // joint type; column of the joint in the (rows, n_arm) arrays, -1 for fixed links
  float pos[G][3], quat[G][4], axis[G][3], lo[G], hi[G];
  int limited[G], moving[G];   // the joint has a range; the joint may move (on a chain and in the dof mask)
  signed char anc[4][G];       // the element whose pose is composed in front of mine in step s, -1: none (my pose is complete)
};

struct IkmArgs {
  IkmTree tr;
  int L, link_lane[IKM_L];     // links; the lane of each link's element
  unsigned anc_mask[IKM_L];    // bit j: element j lies on the chain of link l
  int pm[3], rot_mode, rot_axis;  // position mask; 0: no orientation rows, 1: one axis (rot_axis), 3: all three
  int max_samples;
  unsigned seed;
  unsigned long long moving_cols;  // bit k: column k is written by its moving joint's lane (the others are copies of the seed)
  const float* target_pos;   // (rows or B, L, 3)
  const float* target_quat;  // (rows or B or 1, L, 4); unused when rot_mode == 0
  const float* init_qpos;
  const float* scene_qpos;
  int qst, n_arm;
  int arm_qadr[MIR_MAX_DOF];
  float* qpos_out;           // (rows, n_arm)
  float* err_out;            // (rows, L, 2) or null
  int32_t* iters_out;        // (rows) or null
  int32_t* sample_out;       // (rows) or null
  const long long* env_idx;
  int n_rows, pos_by_env, quat_by_env, quat_one, init_by_env, init_col0, init_ncols;
  int B, max_iters, respect_limits;
  float inv_pos_tol, inv_rot_tol;
  float damping2, pos_tol, rot_tol, max_step;
};

__device__ __forceinline__ Q4 qconj(Q4 q) { return {q.w, -q.x, -q.y, -q.z}; }

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
  const int tid = threadIdx.x, lane = tid & 15, grp = tid >> 4;
  const int row_raw = blockIdx.x * 4 + grp;
  const bool valid = row_raw < a.n_rows;
  const int row = valid ? row_raw : a.n_rows - 1;
  int env = a.env_idx ? (int)a.env_idx[row] : row;
  env = env < 0 ? 0 : (env >= a.B ? a.B - 1 : env);  // (an index outside the batch is clamped, as in mir_inverse_kinematics_rows)
  const int prow = a.pos_by_env ? env : row, qrow = a.quat_one ? 0 : (a.quat_by_env ? env : row), irow = a.init_by_env ? env : row;
  const int n = a.tr.n, L = a.L;
  const int rowbase = tid & ~15;
  const bool onchain = lane < n;
  const int jt = onchain ? a.tr.jtype[lane] : MIR_JNT_FIXED, qc = onchain ? a.tr.qcol[lane] : -1;
  const V3 bpos = ld3(a.tr.pos[lane]), baxis = ld3(a.tr.axis[lane]);
  const Q4 bquat = ld4(a.tr.quat[lane]);
  const bool scalar = onchain && qc >= 0 && (jt == MIR_JNT_REVOLUTE || jt == MIR_JNT_PRISMATIC);
  const bool moving = scalar && a.tr.moving[lane];
  const float lo = a.tr.lo[lane], hi = a.tr.hi[lane];
  const bool limited = moving && a.tr.limited[lane];
  const bool lim = limited && a.respect_limits;
  int src4[4];  // (lane_gather address of the element composed in front of mine in step s; -1: none)
#pragma unroll
  for (int s = 0; s < 4; s++) {
    const int an = a.tr.anc[s][lane];
    src4[s] = an >= 0 ? (rowbase + an) << 2 : -1;
  }
  auto seed = [&](int k) -> float {
    const bool from_init = a.init_qpos && k >= a.init_col0 && k < a.init_col0 + a.init_ncols;
    return from_init ? a.init_qpos[(size_t)irow * a.init_ncols + (k - a.init_col0)] : a.scene_qpos[(size_t)env * a.qst + a.arm_qadr[k]];
  };
  // every column that no lane moves is the seed, bit for bit; a moving joint's column is written once, at the end, by its lane
  for (int k = lane; k < a.n_arm; k += G)
    if (valid && !((a.moving_cols >> k) & 1ull)) a.qpos_out[(size_t)row * a.n_arm + k] = seed(k);
  const float q_seed = scalar ? seed(qc) : 0.0f;
  const bool userot = a.rot_mode != 0;
  const V3 ek = v3(a.rot_axis == 0 ? 1.0f : 0.0f, a.rot_axis == 1 ? 1.0f : 0.0f, a.rot_axis == 2 ? 1.0f : 0.0f);
  V3 tp[IKM_L], ta[IKM_L];
  Q4 tq[IKM_L];
#pragma unroll
  for (int l = 0; l < IKM_L; l++) {
    tp[l] = v3(0, 0, 0); ta[l] = v3(0, 0, 0); tq[l] = Q4{1, 0, 0, 0};
    if (l < L) {
      tp[l] = ld3(a.target_pos + ((size_t)prow * L + l) * 3);
      if (userot) {
        tq[l] = qnormalize(ld4(a.target_quat + ((size_t)qrow * L + l) * 4));
        ta[l] = qrot(tq[l], ek);
      }
    }
  }
  const float lam2_min = a.damping2 * (1.0f / 256.0f), lam2_max = a.damping2 * 64.0f;
  // the result so far (the first converged sample, else the smallest final metric) and the row's state over the samples
  float res_q = q_seed, res_m = 0.0f, res_ep[IKM_L] = {0, 0, 0, 0}, res_er[IKM_L] = {0, 0, 0, 0};
  int res_s = 0, total_iters = 0;
  bool finished = false;
  for (int s = 0; s < a.max_samples; s++) {
    if (s > 0 && !__any(!finished)) break;
    float q = q_seed;
    if (s > 0 && limited) q = lo + (hi - lo) * ikm_uniform(a.seed, (unsigned)env, (unsigned)s, (unsigned)qc);
    bool done = finished, conv = false;
    int stall = 0, my_iters = 0;
    float q_acc = q, lam2 = a.damping2, m_acc = 0.0f, g_acc = 0.0f;
    float epn[IKM_L] = {0, 0, 0, 0}, ern[IKM_L] = {0, 0, 0, 0};
    float J[6 * IKM_L], e[6 * IKM_L];
#pragma unroll
    for (int r = 0; r < 6 * IKM_L; r++) J[r] = e[r] = 0.0f;
    for (int it = 0; it <= a.max_iters; it++) {
      // ---- local transform of my element (identity off the tree) at the CANDIDATE q ...
      V3 P = v3(0, 0, 0);
      Q4 Qx = Q4{1, 0, 0, 0};
      if (onchain) {
        Qx = bquat;
        P = bpos;
        if (jt == MIR_JNT_REVOLUTE) {
          float sn, cs;
          sincos_pi2(0.5f * q, &sn, &cs);
          Qx = qmul(bquat, Q4{cs, baxis.x * sn, baxis.y * sn, baxis.z * sn});
        } else if (jt == MIR_JNT_PRISMATIC) {
          P = bpos + qrot(bquat, q * baxis);
        }
      }
      // ... then my world pose by pointer doubling: (P, Q) is my pose relative to an ancestor; composing it with that ancestor's
      // pose relative to ITS ancestor doubles the distance covered (every lane gathers before any lane updates)
#pragma unroll
      for (int st = 0; st < 4; st++) {
        if (st < a.tr.nsteps) {
          const int sa = src4[st], ad = sa >= 0 ? sa : (tid << 2);
          const V3 pp = v3(lane_gather(ad, P.x), lane_gather(ad, P.y), lane_gather(ad, P.z));
          const Q4 pq = Q4{lane_gather(ad, Qx.w), lane_gather(ad, Qx.x), lane_gather(ad, Qx.y), lane_gather(ad, Qx.z)};
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
          pe[l] = v3(lane_gather(ad, P.x), lane_gather(ad, P.y), lane_gather(ad, P.z));
          const V3 dp = tp[l] - pe[l];
          ep[l] = v3(a.pm[0] ? dp.x : 0.0f, a.pm[1] ? dp.y : 0.0f, a.pm[2] ? dp.z : 0.0f);
          if (userot) {
            const Q4 qe = Q4{lane_gather(ad, Qx.w), lane_gather(ad, Qx.x), lane_gather(ad, Qx.y), lane_gather(ad, Qx.z)};
            if (a.rot_mode == 3) {
              Q4 d = qmul(tq[l], qconj(qe));  // rotation taking the current frame to the target, world axes
              if (d.w < 0.0f) d = Q4{-d.w, -d.x, -d.y, -d.z};
              const float sn = sqrtf(d.x * d.x + d.y * d.y + d.z * d.z);
              const float ang = 2.0f * atan2f(sn, d.w);
              const float k = sn > 1e-9f ? ang / sn : 2.0f;
              er[l] = v3(k * d.x, k * d.y, k * d.z);
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
          metric += epn_c[l] * a.inv_pos_tol + ern_c[l] * a.inv_rot_tol;
        }
      }
      if (!done) {
        if (it == 0 || metric < m_acc) {
          // accepted: the damping relaxes; stagnation = an accepted step that gained less than 1 %
          if (it > 0) {
            stall = metric > 0.99f * m_acc ? stall + 1 : 0;
            lam2 = fmaxf(lam2 * 0.25f, lam2_min);
          }
          m_acc = metric;
          q_acc = q;
          float g = 0.0f;
          conv = true;
#pragma unroll
          for (int l = 0; l < IKM_L; l++) {
            if (l < L) {
              epn[l] = epn_c[l]; ern[l] = ern_c[l];
              conv = conv && epn[l] < a.pos_tol && ern[l] < a.rot_tol;
              e[6 * l + 0] = ep[l].x; e[6 * l + 1] = ep[l].y; e[6 * l + 2] = ep[l].z;
              e[6 * l + 3] = er[l].x; e[6 * l + 4] = er[l].y; e[6 * l + 5] = er[l].z;
              // my Jacobian column for link l at the accepted iterate (joint frame = my world pose)
              V3 jv = v3(0, 0, 0), jw = v3(0, 0, 0);
              if (moving && ((a.anc_mask[l] >> lane) & 1u)) {
                const V3 axw = qrot(Qx, baxis);
                if (jt == MIR_JNT_REVOLUTE) { jw = axw; jv = cross(axw, pe[l] - P); }
                else jv = axw;
              }
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
          // rejected (the scaled error did not fall): back to the accepted iterate with eight times the damping; a stalled iteration
          stall++;
          lam2 = fminf(lam2 * 8.0f, lam2_max);
        }
        if (conv || stall >= 3) done = true;
      }
      if (it == a.max_iters) break;
      if (!__any(!done)) break;
      // ---- row `lane` of J^T J + lambda^2 I (J, e: the accepted iterate's), then dq by elimination
      float H[G];
#pragma unroll
      for (int k = 0; k < G; k++) H[k] = k == lane ? lam2 : 0.0f;
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
      const float big = gmaxf(fabsf(dq));
      const float sc = big > a.max_step ? a.max_step / big : 1.0f;
      if (!done) my_iters = it + 1;
      q = q_acc;
      if (moving && !done) {
        q = q_acc + sc * dq;
        if (lim) q = fminf(fmaxf(q, lo), hi);
      }
    }
    if (!finished) {
      total_iters += my_iters;
      if (conv || s == 0 || m_acc < res_m) {
        res_q = q_acc; res_m = m_acc; res_s = s;
#pragma unroll
        for (int l = 0; l < IKM_L; l++) { res_ep[l] = epn[l]; res_er[l] = ern[l]; }
      }
      finished = conv;
    }
  }
  if (valid && moving) a.qpos_out[(size_t)row * a.n_arm + qc] = res_q;
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

void qmul_h(const double* p, const double* q, double* r) {
  r[0] = p[0] * q[0] - p[1] * q[1] - p[2] * q[2] - p[3] * q[3]; r[1] = p[0] * q[1] + p[1] * q[0] + p[2] * q[3] - p[3] * q[2];
  r[2] = p[0] * q[2] - p[1] * q[3] + p[2] * q[0] + p[3] * q[1]; r[3] = p[0] * q[3] + p[1] * q[2] - p[2] * q[1] + p[3] * q[0];
}

}  // namespace

extern "C" int mir_ik_multi_sizeof(void) { return (int)sizeof(MirIkMulti); }

extern "C" int mir_inverse_kinematics_multilink(MirHandle h, const MirIkMulti* mq, const float* target_pos, const float* target_quat,
                                                const float* init_qpos, const MirIkOptions* opt, float* qpos_out, float* err_out,
                                                int32_t* iters_out, int32_t* sample_out, void* stream) {
  if (!h || !mq || !target_pos || !qpos_out) return mir_set_error(MIR_E_INVALID, "mir_inverse_kinematics_multilink: null argument");
  if (mq->struct_size != (int32_t)sizeof(MirIkMulti)) return mir_set_error(MIR_E_INVALID, "mir_inverse_kinematics_multilink: struct_size");
  const MirIkRows* rows = &mq->rows;
  if (rows->n_rows < 0 || (rows->flags & ~(uint32_t)(MIR_IK_POS_BY_ENV | MIR_IK_QUAT_BY_ENV | MIR_IK_QUAT_ONE | MIR_IK_INIT_BY_ENV)))
    return mir_set_error(MIR_E_INVALID, "mir_inverse_kinematics_multilink: bad row description");
  if (mq->n_links < 1 || mq->n_links > IKM_L) return mir_set_error(MIR_E_INVALID, "mir_inverse_kinematics_multilink: n_links outside 1 .. 4");
  if (mq->max_samples < 1) return mir_set_error(MIR_E_INVALID, "mir_inverse_kinematics_multilink: max_samples < 1");
  const int nrot = (mq->rot_mask[0] ? 1 : 0) + (mq->rot_mask[1] ? 1 : 0) + (mq->rot_mask[2] ? 1 : 0);
  const int npos = (mq->pos_mask[0] ? 1 : 0) + (mq->pos_mask[1] ? 1 : 0) + (mq->pos_mask[2] ? 1 : 0);
  if (nrot == 2) return mir_set_error(MIR_E_INVALID, "mir_inverse_kinematics_multilink: rot_mask aligns 0, 1 or all 3 axes");
  const int rot_mode = target_quat ? nrot : 0;
  if (npos == 0 && rot_mode == 0) return mir_set_error(MIR_E_INVALID, "mir_inverse_kinematics_multilink: the masks select no task row");
  MirIkOptions o = {20, 1, 0.05, 5e-4, 5e-3, 0.5};
  if (opt) {
    o = *opt;
    if (o.max_iters <= 0 || !(o.damping > 0.0) || !(o.max_step > 0.0) || !(o.pos_tol > 0.0) || !(o.rot_tol > 0.0))
      return mir_set_error(MIR_E_INVALID, "mir_inverse_kinematics_multilink: bad options");
  }
  const int nbody = h->nbody;
  const ModelView mv(h);
  // the union of the chains world -> link_l, with each body's depth
  int depth[MIR_MAX_BODY];
  bool inu[MIR_MAX_BODY], target[MIR_MAX_BODY];
  for (int b = 0; b < MIR_MAX_BODY; b++) { depth[b] = 0; inu[b] = target[b] = false; }
  for (int l = 0; l < mq->n_links; l++) {
    const int lb = mq->link_body[l];
    if (lb <= 0 || lb >= nbody) return mir_set_error(MIR_E_INVALID, "mir_inverse_kinematics_multilink: link out of range");
    target[lb] = true;
    int steps = 0;
    for (int b = lb; b > 0; b = mv.parent(b)) {
      if (mv.jtype(b) == MIR_JNT_FREE) return mir_set_error(MIR_E_INVALID, "mir_inverse_kinematics_multilink: the link hangs off a free body");
      if (++steps > MIR_MAX_BODY) return mir_set_error(MIR_E_INVALID, "mir_inverse_kinematics_multilink: parent cycle");
      inu[b] = true;
    }
  }
  for (int b = 1; b < nbody; b++)
    if (inu[b]) { int d = 0; for (int c = b; c > 0; c = mv.parent(c)) d++; depth[b] = d; }
  // columns of the scalar joints in the (rows, n_arm) arrays = their rank in body order
  IkmArgs a;
  memset(&a, 0, sizeof a);
  int col_of_body[MIR_MAX_BODY], narm = 0;
  for (int b = 1; b < nbody; b++) {
    const int jt = mv.jtype(b);
    col_of_body[b] = (jt == MIR_JNT_REVOLUTE || jt == MIR_JNT_PRISMATIC) ? narm++ : -1;
    if (col_of_body[b] >= 0) a.arm_qadr[col_of_body[b]] = mv.qadr(b);
  }
  if (rows->init_ncols > 0 && (rows->init_col0 < 0 || rows->init_col0 + rows->init_ncols > narm))
    return mir_set_error(MIR_E_INVALID, "mir_inverse_kinematics_multilink: init columns outside the joint row");
  if (rows->init_ncols < 0)
    return mir_set_error(MIR_E_INVALID, "mir_inverse_kinematics_multilink: init columns outside the joint row");
  // elements in order of depth (parents first).  A FIXED body that is no target is a constant: folded into the base transform of
  // each of its children (pos' = p_f + R_f pos, quat' = q_f quat), as mir_ik.hip folds the fixed elements of its chain
  int el_of[MIR_MAX_BODY], fold_par[MIR_MAX_BODY], par_el[G], nel = 0;
  bool folded[MIR_MAX_BODY];
  double fp[MIR_MAX_BODY][3], fq[MIR_MAX_BODY][4];
  for (int b = 0; b < MIR_MAX_BODY; b++) { el_of[b] = -1; fold_par[b] = -1; folded[b] = false; }
  for (int d = 1; d <= MIR_MAX_BODY; d++)
    for (int b = 1; b < nbody; b++) {
      if (!inu[b] || depth[b] != d) continue;
      double p[3], q[4], ax[3], lo = 0, hi = 0;
      int limited = 0;
      for (int k = 0; k < 3; k++) { p[k] = mv.body_pos(b)[k]; ax[k] = mv.body_axis(b)[k]; }
      for (int k = 0; k < 4; k++) q[k] = mv.body_quat(b)[k];
      if (col_of_body[b] >= 0) mv.limits(b, lo, hi, limited);
      const int pb = mv.parent(b);
      int pe = -1;
      if (pb > 0 && folded[pb]) {  // my base transform behind the folded parent's
        const double v[4] = {0, p[0], p[1], p[2]}, *cq = fq[pb];
        double t[4], cqc[4] = {cq[0], -cq[1], -cq[2], -cq[3]}, rv[4], nq[4];
        qmul_h(cq, v, t); qmul_h(t, cqc, rv);
        for (int k = 0; k < 3; k++) p[k] = fp[pb][k] + rv[1 + k];
        qmul_h(cq, q, nq);
        for (int k = 0; k < 4; k++) q[k] = nq[k];
        pe = fold_par[pb];
      } else if (pb > 0) {
        pe = el_of[pb];
      }
      if (mv.jtype(b) == MIR_JNT_FIXED && !target[b]) {
        folded[b] = true; fold_par[b] = pe;
        for (int k = 0; k < 3; k++) fp[b][k] = p[k];
        for (int k = 0; k < 4; k++) fq[b][k] = q[k];
        continue;
      }
      if (nel >= G) return mir_set_error(MIR_E_CAPACITY, "mir_inverse_kinematics_multilink: the union of the chains has more than 16 elements");
      const int i = nel++;
      el_of[b] = i; par_el[i] = pe;
      a.tr.jtype[i] = mv.jtype(b); a.tr.qcol[i] = col_of_body[b];
      for (int k = 0; k < 3; k++) { a.tr.pos[i][k] = (float)p[k]; a.tr.axis[i][k] = (float)ax[k]; }
      for (int k = 0; k < 4; k++) a.tr.quat[i][k] = (float)q[k];
      a.tr.lo[i] = (float)lo; a.tr.hi[i] = (float)hi; a.tr.limited[i] = limited;
      const int c = col_of_body[b];
      a.tr.moving[i] = c >= 0 && (!mq->dof_mask || mq->dof_mask[c]) ? 1 : 0;
      if (a.tr.moving[i]) a.moving_cols |= 1ull << c;
    }
  a.tr.n = nel;
  for (int i = nel; i < G; i++) { a.tr.jtype[i] = MIR_JNT_FIXED; a.tr.qcol[i] = -1; a.tr.quat[i][0] = 1.0f; }
  // pointer doubling: anc[0] = the parent element, anc[s + 1] = anc[s] of anc[s]; as many steps as leave an ancestor to compose
  {
    int cur[G];
    for (int i = 0; i < G; i++) cur[i] = i < nel ? par_el[i] : -1;
    int s = 0;
    for (; s < 4; s++) {
      bool any = false;
      for (int i = 0; i < G; i++) { a.tr.anc[s][i] = (signed char)cur[i]; any = any || cur[i] >= 0; }
      if (!any) break;
      int nxt[G];
      for (int i = 0; i < G; i++) nxt[i] = cur[i] >= 0 ? cur[cur[i]] : -1;
      for (int i = 0; i < G; i++) cur[i] = nxt[i];
    }
    a.tr.nsteps = s;
    for (int t = s; t < 4; t++) for (int i = 0; i < G; i++) a.tr.anc[t][i] = -1;
  }
  a.L = mq->n_links;
  for (int l = 0; l < mq->n_links; l++) {
    a.link_lane[l] = el_of[mq->link_body[l]];
    for (int i = a.link_lane[l]; i >= 0; i = par_el[i]) a.anc_mask[l] |= 1u << i;
  }
  for (int k = 0; k < 3; k++) a.pm[k] = mq->pos_mask[k] ? 1 : 0;
  a.rot_mode = rot_mode;
  a.rot_axis = mq->rot_mask[0] ? 0 : (mq->rot_mask[1] ? 1 : 2);
  a.max_samples = mq->max_samples; a.seed = mq->seed;
  a.target_pos = target_pos; a.target_quat = target_quat; a.init_qpos = init_qpos; a.scene_qpos = h->qpos;
  a.qst = h->pt.qst; a.n_arm = narm; a.qpos_out = qpos_out; a.err_out = err_out; a.iters_out = iters_out; a.sample_out = sample_out; a.B = h->B;
  a.env_idx = reinterpret_cast<const long long*>(rows->env_idx);
  a.n_rows = rows->env_idx ? rows->n_rows : h->B;
  if (a.n_rows == 0) return MIR_OK;
  a.pos_by_env = (rows->flags & MIR_IK_POS_BY_ENV) ? 1 : 0; a.quat_by_env = (rows->flags & MIR_IK_QUAT_BY_ENV) ? 1 : 0;
  a.quat_one = (rows->flags & MIR_IK_QUAT_ONE) ? 1 : 0; a.init_by_env = (rows->flags & MIR_IK_INIT_BY_ENV) ? 1 : 0;
  a.init_col0 = 0; a.init_ncols = narm;
  if (rows->init_ncols > 0) { a.init_col0 = rows->init_col0; a.init_ncols = rows->init_ncols; }
  a.max_iters = o.max_iters; a.respect_limits = o.respect_joint_limit;
  a.damping2 = (float)(o.damping * o.damping); a.pos_tol = (float)o.pos_tol; a.rot_tol = (float)o.rot_tol;
  a.inv_pos_tol = (float)(1.0 / o.pos_tol); a.inv_rot_tol = (float)(1.0 / o.rot_tol); a.max_step = (float)o.max_step;
  return launch_rows(h, mir_ikm_kernel, (a.n_rows + 3) / 4, stream, a);
}
