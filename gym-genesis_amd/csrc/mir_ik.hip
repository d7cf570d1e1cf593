// mir_ik.hip — batched damped-least-squares inverse kinematics.
//
// What it replaces: robot.inverse_kinematics(link, pos, quat, ...) of the reference's expert policies
// (/root/reference/examples/franka/pick_cube_state.py:46-51, stack_cube_state.py:78-83), called once per env.step()
// in those loops, i.e. on the callers' side of the hot path.  The algorithm is defined in include/mirigid.h.
//
// Mapping: like the pick kernel, 16 lanes per env (4 envs per wave64, one DPP row each); lane j owns element j of the
// kinematic chain world -> link (<= 16 bodies): its local joint transform, its world pose (prefix of the chain by a log-step DPP
// scan: no depth-serial barriers, no LDS at all since round 6), its Jacobian column.  J J^T + lambda^2 I (6 x 6, symmetric: 21 DPP row
// reductions) ends up in every lane's registers and each lane solves it redundantly (Cholesky, fully unrolled), so the
// update dq_j = J_j . y needs no further communication.  The chain description travels in the kernel arguments
// (built on the host per call: the link is a run-time argument).
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

struct IkArgs {
  IkElems ch;                // the chain world -> link, root first (the tree of one link)
  IkRowArgs r;
  float* qpos_out;           // (rows, n_arm)
  float* err_out;            // (rows, 2) or null
  int32_t* iters_out;        // (rows) or null: iterations the row took (debug: mir_debug_ik_iters)
};

__global__ __launch_bounds__(64) void mir_ik_kernel(IkArgs a) {
  const int tid = threadIdx.x, lane = tid & 15;
  const IkRow t = ik_row_decode(a.r);
  const int row = t.row;
  const bool valid = t.valid;
  const int n = a.ch.n;
  const int eef4 = ((tid & ~15) + n - 1) << 2;  // (lane_gather address of the chain's last element in this env's row)
  const bool onchain = lane < n;
  const int jt = onchain ? a.ch.jtype[lane] : MIR_JNT_FIXED, qc = onchain ? a.ch.qcol[lane] : -1;
  const V3 bpos = ld3(a.ch.pos[lane]), baxis = ld3(a.ch.axis[lane]);
  const Q4 bquat = ld4(a.ch.quat[lane]);
  const bool moving = onchain && qc >= 0 && (jt == MIR_JNT_REVOLUTE || jt == MIR_JNT_PRISMATIC);
  const float lo = a.ch.lo[lane], hi = a.ch.hi[lane];
  const bool lim = moving && a.ch.limited[lane] && a.r.respect_limits;
  // seed: every scalar joint (the result keeps the seed outside the chain)
  for (int k = lane; k < a.r.n_arm; k += G) {
    const float v = ik_seed(a.r, t.env, t.irow, k);
    if (valid) a.qpos_out[(size_t)row * a.r.n_arm + k] = v;
  }
  float q = 0.0f;
  if (moving) q = ik_seed(a.r, t.env, t.irow, qc);
  const V3 tp = ld3(a.r.target_pos + (size_t)t.prow * 3);
  const bool userot = a.r.target_quat != nullptr;
  const Q4 tq = userot ? qnormalize(ld4(a.r.target_quat + (size_t)t.qrow * 4)) : Q4{1, 0, 0, 0};
  bool done = false;
  int my_iters = 0;
  // the ACCEPTED iterate (Levenberg - Marquardt acceptance, include/mirigid.h): this lane's joint angle, Jacobian column; the env's
  // task-space error and scaled error (identical in all of its lanes: they are computed from the same gathered values)
  float q_acc = q, epn = 0.0f, ern = 0.0f;
  LmState lm = {a.r.damping2, 0, 0.0f};
  float J[6] = {0, 0, 0, 0, 0, 0}, e[6] = {0, 0, 0, 0, 0, 0};
  for (int it = 0; it <= a.r.max_iters; it++) {
    // ---- local transform of my chain element (identity off the chain) at the CANDIDATE q, then my own prefix of the chain by a
    // log-step scan over the DPP row: 4 shifted exchanges instead of a walk of up to 15 links, no LDS round trips (the Panda's chain to
    // the hand is eight elements once its fixed base link is folded into joint 1: three steps)
    const Pose x = path_scan(ik_elem_local(onchain, jt, bpos, bquat, baxis, q), lane, n);
    const V3 P = x.P;
    const Q4 Qx = x.Qx;
    // ---- task-space error of the candidate (every lane, redundantly): the pose of the chain's last element comes over the crossbar
    // (seven lane gathers, one trip; round 5 went through LDS: a store, a fence and a load per iteration of a chain that is all latency)
    const V3 pe = gather3(eef4, P);
    const Q4 qe = gather4(eef4, Qx);
    const V3 ep = tp - pe;
    V3 er = v3(0, 0, 0);
    if (userot) er = ik_rot_error(tq, qe);
    const float epn_c = sqrtf(dot(ep, ep)), ern_c = sqrtf(dot(er, er));
    const float metric = epn_c * a.r.inv_pos_tol + ern_c * a.r.inv_rot_tol;
    if (!done) {
      if (lm_accepts(lm, metric, it == 0)) {
        lm = lm_accept(lm, metric, it == 0, a.r.damping2);
        epn = epn_c; ern = ern_c;
        e[0] = ep.x; e[1] = ep.y; e[2] = ep.z; e[3] = er.x; e[4] = er.y; e[5] = er.z;
        q_acc = q;
        // my Jacobian column at the accepted iterate
        const JacColumn c = ik_jac_column(moving, jt, Qx, P, baxis, pe);
        J[0] = c.jv.x; J[1] = c.jv.y; J[2] = c.jv.z; J[3] = userot ? c.jw.x : 0.0f; J[4] = userot ? c.jw.y : 0.0f; J[5] = userot ? c.jw.z : 0.0f;
      } else {
        lm = lm_reject(lm, a.r.damping2);
      }
      if ((epn < a.r.pos_tol && ern < a.r.rot_tol) || lm_stalled(lm)) done = true;
    }
    if (it == a.r.max_iters) break;
    if (!__any(!done)) break;
    // ---- A = J J^T + lambda^2 I in every lane (J, e: the accepted iterate's)
    float A[6][6];
#pragma unroll
    for (int r = 0; r < 6; r++)
#pragma unroll
      for (int c = 0; c <= r; c++) {
        const float v = gsum(J[r] * J[c]) + (r == c ? lm.lam2 : 0.0f);
        A[r][c] = v;
        A[c][r] = v;
      }
    // ---- y = A^-1 e (Cholesky, SPD by the damping)
    float L[6][6], y[6], il[6];  // il = 1 / L[c][c]: one reciprocal per column instead of a division per use
#pragma unroll
    for (int r = 0; r < 6; r++)
#pragma unroll
      for (int c = 0; c <= r; c++) {
        float sacc = A[r][c];
#pragma unroll
        for (int k = 0; k < c; k++) sacc -= L[r][k] * L[c][k];
        if (r == c) {
          const float dd = sqrtf(fmaxf(sacc, 1e-30f));
          float ir = __builtin_amdgcn_rcpf(dd);
          L[r][c] = dd;
          il[r] = ir;
        } else {
          L[r][c] = sacc * il[c];
        }
      }
#pragma unroll
    for (int r = 0; r < 6; r++) {
      float sacc = e[r];
#pragma unroll
      for (int k = 0; k < r; k++) sacc -= L[r][k] * y[k];
      y[r] = sacc * il[r];
    }
#pragma unroll
    for (int r = 5; r >= 0; r--) {
      float sacc = y[r];
#pragma unroll
      for (int k = r + 1; k < 6; k++) sacc -= L[k][r] * y[k];
      y[r] = sacc * il[r];
    }
    float dq = 0.0f;
#pragma unroll
    for (int r = 0; r < 6; r++) dq += J[r] * y[r];
    const float sc = ik_step_scale(dq, a.r.max_step);
    if (!done) my_iters = it + 1;
    q = q_acc;
    if (moving && !done) {
      q = q_acc + sc * dq;
      if (lim) q = fminf(fmaxf(q, lo), hi);
    }
  }
  q = q_acc;
  if (valid && moving) a.qpos_out[(size_t)row * a.r.n_arm + qc] = q;
  if (valid && a.iters_out && lane == 0) a.iters_out[row] = my_iters;
  if (valid && a.err_out && lane == 0) {
    a.err_out[(size_t)row * 2] = epn;
    a.err_out[(size_t)row * 2 + 1] = ern;
  }
}

}  // namespace

extern "C" int mir_inverse_kinematics_rows(MirHandle h, int32_t link_body, const MirIkRows* rows, const float* target_pos, const float* target_quat,
                                           const float* init_qpos, const MirIkOptions* opt, float* qpos_out, float* err_out, void* stream) {
  const char* who = "mir_inverse_kinematics";
  if (!h || !target_pos || !qpos_out) return query_error(MIR_E_INVALID, who, "null argument");
  if (int rc = ik_check_rows(rows, "mir_inverse_kinematics_rows")) return rc;
  if (rows && rows->n_rows == 0) return MIR_OK;
  // the chain world -> link from whichever model serves the scene: the tree of one link
  IkTree t;
  const char* what;
  if (int rc = build_ik_tree(ModelView(h), h->nbody, &link_body, 1, nullptr, "chain longer than 16 bodies", t, &what)) return query_error(rc, who, what);
  MirIkOptions o;
  if (int rc = ik_options(opt, false, who, o)) return rc;
  IkArgs a;
  memset(&a, 0, sizeof a);
  a.ch = t.el;
  if (int rc = fill_ik_rows(h, rows, o, t, false, "mir_inverse_kinematics_rows", target_pos, target_quat, init_qpos, a.r)) return rc;
  a.qpos_out = qpos_out; a.err_out = err_out; a.iters_out = h->dbg_ik_iters;
  return launch_rows(h, mir_ik_kernel, (a.r.n_rows + 3) / 4, stream, a);
}

extern "C" int mir_inverse_kinematics(MirHandle h, int32_t link_body, const float* target_pos, const float* target_quat, const float* init_qpos,
                                      const MirIkOptions* opt, float* qpos_out, float* err_out, void* stream) {
  return mir_inverse_kinematics_rows(h, link_body, nullptr, target_pos, target_quat, init_qpos, opt, qpos_out, err_out, stream);
}

/* debug aid (tools/probes/ik_iters.py): every following mir_inverse_kinematics call also writes the iterations each env took into
 * iters (B x i32, device; NULL switches it off) */
extern "C" int mir_debug_ik_iters(MirHandle h, int32_t* iters) {
  if (!h) return mir_set_error(MIR_E_INVALID, "null MirHandle");
  h->dbg_ik_iters = iters;
  return MIR_OK;
}

/* debug aid (tests/test_gpu_api.py): the row all-reduce of mir_dev.h on n_rows rows of 16 floats -- out[r][l] = what lane l of row r
 * holds after gsum.  Every lane of a row must hold the same bits: decisions of the 16-lane kernel's solver are taken per lane. */
namespace {
__global__ __launch_bounds__(64) void k_debug_row_sum(const float* __restrict__ in, float* __restrict__ out, int n_rows) {
  const int i = blockIdx.x * 64 + threadIdx.x;       // (whole waves: the DPP reads need every lane of the row present)
  const float v = i < n_rows * 16 ? in[i] : 0.0f;
  const float s = gsum(v);
  if (i < n_rows * 16) out[i] = s;
}
}  // namespace
extern "C" int mir_debug_row_sum(const float* in, float* out, int32_t n_rows, int device_id, void* stream) {
  if (!in || !out || n_rows <= 0) return mir_set_error(MIR_E_INVALID, "mir_debug_row_sum: bad argument");
  DeviceGuard guard(device_id);
  hipLaunchKernelGGL(k_debug_row_sum, dim3((n_rows * 16 + 63) / 64), dim3(64), 0, (hipStream_t)stream, in, out, n_rows);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MIR_OK : mir_set_error(MIR_E_HIP, hipGetErrorString(e));
}

