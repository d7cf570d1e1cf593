// mir_ik_front.h — the front end the two inverse-kinematics kernels share (mir_ik.hip: one link, a chain; mir_ikm.hip: up to four
// links, the union tree of their chains).
//   host:   the element table of the tree with its fixed elements folded, the pointer-doubling table and the link masks
//           (build_ik_tree: a chain is the tree of one link); the rows / options part of the kernel arguments with its validation;
//   device: the row a 16-lane DPP row serves, the seed of a joint column, the local transform of an element at a candidate q, the
//           log-map rotation error, the Jacobian column of an element, the Levenberg - Marquardt bookkeeping and the step scaling.
// The first part is plain C++ against a model view given as a template parameter (tests/ik_tree_host.cpp builds it with g++ and a
// fake model); the rest needs mir_dev.h with G = 16 and mir_query.h in front of it.  Inside no namespace.
#pragma once
#include <stdint.h>
#include <string.h>

#include "mirigid.h"

namespace {

constexpr int IK_LINKS = 4;  // links per call of the multi-link kernel

// the elements of the tree, parents before children (a chain: root first); the first member of both kernels' arguments
struct IkElems {
  int n;                       // elements
  int jtype[G], qcol[G];       // joint type; column of the joint in the (rows, n_arm) arrays, -1 for fixed links
  float pos[G][3], quat[G][4], axis[G][3], lo[G], hi[G];
  int limited[G];              // the joint has a range
};

// what build_ik_tree makes of a list of links
struct IkTree {
  IkElems el;
  int par_el[G];               // the parent element, -1: the world
  int nsteps;                  // pointer-doubling steps that leave an ancestor to compose
  signed char anc[4][G];       // the element whose pose is composed in front of element i's in step s, -1: none (the pose is complete)
  int moving[G];               // the joint may move: scalar, on a chain and in the dof mask
  int link_lane[IK_LINKS];     // the element of each link
  unsigned anc_mask[IK_LINKS]; // bit j: element j lies on the chain of link l
  unsigned long long moving_cols;  // bit k: column k belongs to a moving joint
  int n_arm, arm_qadr[MIR_MAX_DOF];  // scalar joints of the model in body order (the columns); qpos address of column k
};

static void qmul_h(const double* p, const double* q, double* r) {  // r = p q
  r[0] = p[0] * q[0] - p[1] * q[1] - p[2] * q[2] - p[3] * q[3]; r[1] = p[0] * q[1] + p[1] * q[0] + p[2] * q[3] - p[3] * q[2];
  r[2] = p[0] * q[2] - p[1] * q[3] + p[2] * q[0] + p[3] * q[1]; r[3] = p[0] * q[3] + p[1] * q[2] - p[2] * q[1] + p[3] * q[0];
}

// ---- host: the union of the chains world -> link_body[l] as <= 16 elements in order of depth.  A FIXED body that is no link is a
// constant: folded into the base transform of each of its children (pos' = p_f + R_f pos, quat' = q_f quat, accumulated in double and
// cast once) -- for the Panda's hand nine bodies become eight elements, three scan steps instead of four.  View: parent(b), jtype(b),
// qadr(b), body_pos(b), body_quat(b), body_axis(b), limits(b, lo, hi, limited) of a model whose parents precede their children.
// dof_mask (n_arm bytes) may be null.  On failure *what says why (the caller names the entry point); too_many is the text of the
// entry point for more than 16 elements.
template <class View>
static int build_ik_tree(const View& mv, int nbody, const int32_t* link_body, int n_links, const uint8_t* dof_mask, const char* too_many,
                         IkTree& t, const char** what) {
  memset(&t, 0, sizeof t);
  bool inu[MIR_MAX_BODY], target[MIR_MAX_BODY];
  for (int b = 0; b < MIR_MAX_BODY; b++) inu[b] = target[b] = false;
  for (int l = 0; l < n_links; l++) {
    const int lb = link_body[l];
    if (lb <= 0 || lb >= nbody) { *what = "link out of range"; return MIR_E_INVALID; }
    target[lb] = true;
    for (int b = lb; b > 0; b = mv.parent(b)) {
      if (mv.jtype(b) == MIR_JNT_FREE) { *what = "the link hangs off a free body"; return MIR_E_INVALID; }
      inu[b] = true;
    }
  }
  // columns of the scalar joints in the (rows, n_arm) arrays = their rank in body order
  int col_of_body[MIR_MAX_BODY], depth[MIR_MAX_BODY];
  for (int b = 1; b < nbody; b++) {
    const int jt = mv.jtype(b);
    col_of_body[b] = (jt == MIR_JNT_REVOLUTE || jt == MIR_JNT_PRISMATIC) ? t.n_arm++ : -1;
    if (col_of_body[b] >= 0) t.arm_qadr[col_of_body[b]] = mv.qadr(b);
    depth[b] = 0;
    if (inu[b]) for (int c = b; c > 0; c = mv.parent(c)) depth[b]++;
  }
  int el_of[MIR_MAX_BODY], fold_par[MIR_MAX_BODY], nel = 0;
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
      const int c = col_of_body[b];
      if (c >= 0) mv.limits(b, lo, hi, limited);
      const int pb = mv.parent(b);
      int pe = -1;
      if (pb > 0 && folded[pb]) {  // my base transform behind the folded parent's
        const double v[4] = {0, p[0], p[1], p[2]}, *cq = fq[pb];
        double r[4], cqc[4] = {cq[0], -cq[1], -cq[2], -cq[3]}, rv[4], nq[4];
        qmul_h(cq, v, r); qmul_h(r, cqc, rv);
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
      if (nel >= G) { *what = too_many; return MIR_E_CAPACITY; }
      const int i = nel++;
      el_of[b] = i; t.par_el[i] = pe;
      t.el.jtype[i] = mv.jtype(b); t.el.qcol[i] = c;
      for (int k = 0; k < 3; k++) { t.el.pos[i][k] = (float)p[k]; t.el.axis[i][k] = (float)ax[k]; }
      for (int k = 0; k < 4; k++) t.el.quat[i][k] = (float)q[k];
      t.el.lo[i] = (float)lo; t.el.hi[i] = (float)hi; t.el.limited[i] = limited;
      t.moving[i] = c >= 0 && (!dof_mask || dof_mask[c]) ? 1 : 0;
      if (t.moving[i]) t.moving_cols |= 1ull << c;
    }
  t.el.n = nel;
  for (int i = nel; i < G; i++) { t.el.jtype[i] = MIR_JNT_FIXED; t.el.qcol[i] = -1; t.el.quat[i][0] = 1.0f; t.par_el[i] = -1; }
  // pointer doubling: anc[0] = the parent element, anc[s + 1] = anc[s] of anc[s]; as many steps as leave an ancestor to compose
  int cur[G], s = 0;
  for (int i = 0; i < G; i++) cur[i] = t.par_el[i];
  for (; s < 4; s++) {
    bool any = false;
    for (int i = 0; i < G; i++) { t.anc[s][i] = (signed char)cur[i]; any = any || cur[i] >= 0; }
    if (!any) break;
    int nxt[G];
    for (int i = 0; i < G; i++) nxt[i] = cur[i] >= 0 ? cur[cur[i]] : -1;
    for (int i = 0; i < G; i++) cur[i] = nxt[i];
  }
  t.nsteps = s;
  for (int u = s; u < 4; u++) for (int i = 0; i < G; i++) t.anc[u][i] = -1;
  for (int l = 0; l < n_links; l++) {
    t.link_lane[l] = el_of[link_body[l]];
    for (int i = t.link_lane[l]; i >= 0; i = t.par_el[i]) t.anc_mask[l] |= 1u << i;
  }
  return MIR_OK;
}

// ---- the rows and options of a call as both kernels read them
struct IkRowArgs {
  const float* target_pos;   // (rows or B, links, 3)
  const float* target_quat;  // (rows or B or 1, links, 4) or null
  const float* init_qpos;    // (rows or B, init_ncols) or null
  const float* scene_qpos;   // scene state row (B, qst): the seed of every column init_qpos does not hold
  // MirIkRows: output row k is env env_idx[k] (null: env k); inputs by row or by env, ONE quaternion; init_qpos holds columns col0 ..
  const long long* env_idx;
  int n_rows, pos_by_env, quat_by_env, quat_one, init_by_env, init_col0, init_ncols;
  int B, qst, n_arm;
  int arm_qadr[MIR_MAX_DOF]; // qpos address of scalar joint k in the scene row
  int max_iters, respect_limits;
  float inv_pos_tol, inv_rot_tol;
  float damping2, pos_tol, rot_tol, max_step;
};

#ifdef __HIPCC__
// ---- host: validation and filling of IkRowArgs, in three steps because the two entry points report their faults in different orders
// (texts and codes are part of the interface).  What differs between the entries, all of it here:
//   mir_inverse_kinematics_rows       rows may be NULL (the full batch, everything by row); n_rows == 0 returns MIR_OK BEFORE the link
//                                     is looked at; pos_tol / rot_tol <= 0 are not refused (tols_positive = false);
//   mir_inverse_kinematics_multilink  rows is part of the query (never NULL) behind a struct_size check; init_ncols < 0 is refused
//                                     (negative_ncols_bad = true); zero rows return MIR_OK only after everything has been validated.
static int ik_check_rows(const MirIkRows* rows, const char* who) {
  if (rows && (rows->n_rows < 0 || (rows->flags & ~(uint32_t)(MIR_IK_POS_BY_ENV | MIR_IK_QUAT_BY_ENV | MIR_IK_QUAT_ONE | MIR_IK_INIT_BY_ENV))))
    return query_error(MIR_E_INVALID, who, "bad row description");
  return MIR_OK;
}
static int ik_options(const MirIkOptions* opt, bool tols_positive, const char* who, MirIkOptions& o) {
  o = MirIkOptions{20, 1, 0.05, 5e-4, 5e-3, 0.5};
  if (!opt) return MIR_OK;
  o = *opt;
  if (o.max_iters <= 0 || !(o.damping > 0.0) || !(o.max_step > 0.0) || (tols_positive && (!(o.pos_tol > 0.0) || !(o.rot_tol > 0.0))))
    return query_error(MIR_E_INVALID, who, "bad options");
  return MIR_OK;
}
static int fill_ik_rows(MirHandle h, const MirIkRows* rows, const MirIkOptions& o, const IkTree& t, bool negative_ncols_bad, const char* who,
                        const float* target_pos, const float* target_quat, const float* init_qpos, IkRowArgs& r) {
  r.target_pos = target_pos; r.target_quat = target_quat; r.init_qpos = init_qpos; r.scene_qpos = h->qpos;
  r.B = h->B; r.qst = h->pt.qst; r.n_arm = t.n_arm;
  memcpy(r.arm_qadr, t.arm_qadr, sizeof r.arm_qadr);
  r.env_idx = nullptr; r.n_rows = h->B; r.init_col0 = 0; r.init_ncols = t.n_arm;
  r.pos_by_env = r.quat_by_env = r.quat_one = r.init_by_env = 0;
  if (rows) {
    if ((rows->init_ncols > 0 && (rows->init_col0 < 0 || rows->init_col0 + rows->init_ncols > t.n_arm)) || (negative_ncols_bad && rows->init_ncols < 0))
      return query_error(MIR_E_INVALID, who, "init columns outside the joint row");
    r.env_idx = reinterpret_cast<const long long*>(rows->env_idx);
    r.n_rows = rows->env_idx ? rows->n_rows : h->B;
    r.pos_by_env = (rows->flags & MIR_IK_POS_BY_ENV) ? 1 : 0; r.quat_by_env = (rows->flags & MIR_IK_QUAT_BY_ENV) ? 1 : 0;
    r.quat_one = (rows->flags & MIR_IK_QUAT_ONE) ? 1 : 0; r.init_by_env = (rows->flags & MIR_IK_INIT_BY_ENV) ? 1 : 0;
    if (rows->init_ncols > 0) { r.init_col0 = rows->init_col0; r.init_ncols = rows->init_ncols; }
  }
  r.max_iters = o.max_iters; r.respect_limits = o.respect_joint_limit;
  r.damping2 = (float)(o.damping * o.damping); r.pos_tol = (float)o.pos_tol; r.rot_tol = (float)o.rot_tol;
  r.inv_pos_tol = (float)(1.0 / o.pos_tol); r.inv_rot_tol = (float)(1.0 / o.rot_tol); r.max_step = (float)o.max_step;
  return MIR_OK;
}

// ---- device: 16 lanes = one DPP row serve one output row, four rows per wave64.  Whole waves reach every DPP op / gather: the rows
// behind the last one are clamped to it (`valid` predicates their stores).
struct IkRow {
  int row, env, prow, qrow, irow;  // output row; its env; the rows of target_pos, target_quat and init_qpos it reads
  bool valid;
};
__device__ __forceinline__ IkRow ik_row_decode(const IkRowArgs& r) {
  IkRow t;
  const int row_raw = blockIdx.x * 4 + (threadIdx.x >> 4);
  t.valid = row_raw < r.n_rows;
  t.row = t.valid ? row_raw : r.n_rows - 1;
  const int env = r.env_idx ? (int)r.env_idx[t.row] : t.row;
  t.env = env < 0 ? 0 : (env >= r.B ? r.B - 1 : env);  // (an index outside the batch is clamped, not followed: the caller's side checks it)
  t.prow = r.pos_by_env ? t.env : t.row;
  t.qrow = r.quat_one ? 0 : (r.quat_by_env ? t.env : t.row);
  t.irow = r.init_by_env ? t.env : t.row;
  return t;
}

// the seed of joint column k: init_qpos where it holds the column, else the scene state
__device__ __forceinline__ float ik_seed(const IkRowArgs& r, int env, int irow, int k) {
  const bool from_init = r.init_qpos && k >= r.init_col0 && k < r.init_col0 + r.init_ncols;
  return from_init ? r.init_qpos[(size_t)irow * r.init_ncols + (k - r.init_col0)] : r.scene_qpos[(size_t)env * r.qst + r.arm_qadr[k]];
}

// the local transform of an element (the identity where `on` is false) at the joint value q
__device__ __forceinline__ Pose ik_elem_local(bool on, int jt, V3 bpos, Q4 bquat, V3 baxis, float q) {
  V3 P = v3(0, 0, 0);
  Q4 Qx = Q4{1, 0, 0, 0};
  if (on) {
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
  return {P, Qx};
}

// rotvec(tq qe^-1): the rotation taking the current frame qe to the target tq, world axes
__device__ __forceinline__ V3 ik_rot_error(Q4 tq, Q4 qe) {
  Q4 d = qmul(tq, qconj(qe));
  if (d.w < 0.0f) d = Q4{-d.w, -d.x, -d.y, -d.z};
  const float sn = sqrtf(d.x * d.x + d.y * d.y + d.z * d.z);
  const float ang = 2.0f * atan2f(sn, d.w);
  const float k = sn > 1e-9f ? ang / sn : 2.0f;
  return v3(k * d.x, k * d.y, k * d.z);
}

// the Jacobian column of an element whose world pose is (P, Qx) for a point pe of a link behind it (joint frame = the element's pose)
struct JacColumn { V3 jv, jw; };
__device__ __forceinline__ JacColumn ik_jac_column(bool moving, int jt, Q4 Qx, V3 P, V3 baxis, V3 pe) {
  V3 jv = v3(0, 0, 0), jw = v3(0, 0, 0);
  if (moving) {
    const V3 axw = qrot(Qx, baxis);
    if (jt == MIR_JNT_REVOLUTE) { jw = axw; jv = cross(axw, pe - P); }
    else jv = axw;
  }
  return {jv, jw};
}

// ---- device: the Levenberg - Marquardt bookkeeping of include/mirigid.h.  A candidate is accepted when its metric fell below the
// accepted iterate's (always at first): the damping relaxes, and an accepted step that gained less than 1 % counts as stalled (a target
// beyond the joint limits or the reach: without the rule the few unreachable targets of a batch set the time of the whole launch).
// Otherwise it is rejected: back to the accepted iterate with eight times the damping, also stalled.  Three stalls in a row end the row.
constexpr float LM_RELAX = 0.25f, LM_FLOOR = 1.0f / 256.0f;  // lambda^2 on acceptance: x LM_RELAX, not below damping^2 x LM_FLOOR
constexpr float LM_RAISE = 8.0f, LM_CEIL = 64.0f;            // on rejection: x LM_RAISE, not above damping^2 x LM_CEIL
constexpr float LM_STALL_GAIN = 0.99f;                       // an accepted metric above this share of the last one is a stall
constexpr int LM_STALL_LIMIT = 3;
struct LmState { float lam2; int stall; float m_acc; };  // lambda^2; stalled iterations in a row; the accepted iterate's metric
__device__ __forceinline__ bool lm_accepts(LmState s, float metric, bool first) { return first || metric < s.m_acc; }
__device__ __forceinline__ LmState lm_accept(LmState s, float metric, bool first, float damping2) {
  if (!first) {
    s.stall = metric > LM_STALL_GAIN * s.m_acc ? s.stall + 1 : 0;
    s.lam2 = fmaxf(s.lam2 * LM_RELAX, damping2 * LM_FLOOR);
  }
  s.m_acc = metric;
  return s;
}
__device__ __forceinline__ LmState lm_reject(LmState s, float damping2) { return {fminf(s.lam2 * LM_RAISE, damping2 * LM_CEIL), s.stall + 1, s.m_acc}; }
__device__ __forceinline__ bool lm_stalled(LmState s) { return s.stall >= LM_STALL_LIMIT; }

// the factor that brings the row's largest |dq| down to max_step (every lane of the row takes part)
__device__ __forceinline__ float ik_step_scale(float dq, float max_step) {
  const float big = gmaxf(fabsf(dq));
  return big > max_step ? max_step / big : 1.0f;
}

#endif  // __HIPCC__

}  // namespace
