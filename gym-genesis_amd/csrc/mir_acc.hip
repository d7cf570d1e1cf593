// mir_acc.hip — world accelerations of a list of links, the term Jdot qvel and IMU readings in one batched launch
// (mir_link_accelerations, include/mirigid.h; DESIGN.md, link accelerations).
//
// What it serves: entity.get_links_acc(), gs.sensors.IMU (accelerometer + gyro on a link) of Genesis, and the Jdot qvel of
// operational-space control, a = J qacc + Jdot qvel, beside the J of mir_kin.hip.  It reads qpos / qvel, the caller's qacc and the
// compiled model and writes only its own outputs.
//
// Mapping (the one of mir_kin.hip): 16 lanes = one DPP row serve one (row, link) PAIR, four pairs per wave64.  Lane j owns element j of
// the path world -> link (root first, <= 16 bodies); after the pose scan of mir_kin.hip it knows its element's world pose o_j, Q_j, its
// world axis a_j and its qd_j, qdd_j.  From there everything is additive along the path (no composition of motion jets):
//     w_j     = sum_{k <= j} s_k,   s_k = a_k qd_k (revolute), the free root's angular velocity, 0 otherwise        (row prefix sum)
//     da_j/dt = w_{j-1} x a_j: the axis of element j turns with its parent's angular velocity, the exclusive prefix
//     alpha_j = sum_{k <= j} dw_k,  dw_k = a_k qdd_k + (w_{k-1} x a_k) qd_k  (the free root: its angular qacc)     (row prefix sum)
//     o_j - o_{j-1} = d_j is fixed in element j-1 up to a prismatic slide along a_j, so
//     o_j'' - o_{j-1}'' = alpha_{j-1} x d_j + w_{j-1} x (w_{j-1} x d_j) [+ a_j qdd_j + 2 (w_{j-1} x a_j) qd_j, prismatic]
//     (the free root: its linear qacc), and the point p = o_n + r of the last element adds alpha_n x r + w_n x (w_n x r).
// The sum of the per-element terms is a row all-reduce (gsum of mir_dev.h).  Everything is kept in two parts, the one that is linear in
// qacc and the rest: the rest alone is bias_acc = Jdot qvel, the same bits whether or not a qacc was given.
//
// Stores: 6 floats per pair and output, lane k of a row stores component k; the pairs of a wave are neighbours in memory.  No atomics,
// no LDS.  Whole waves reach every DPP op / gather: the pairs behind the last one are clamped to it and their stores predicated.
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

namespace {

struct AccArgs {
  LinkPaths paths;
  float local_point[MIR_MAX_BODY][3];
  float quat_offset[MIR_MAX_BODY][4];  // unit
  int n_links;
  int n_rows, B, qst, vst, nv;
  float gx, gy, gz;
  const long long* env_idx;
  const float *qpos, *qvel;         // the scene's state (storage layout)
  const float* qacc;                // the caller's rows (public layout), nullable: zeros
  JointPtrs m;
  float *acc, *bias, *imu;
};
static_assert(sizeof(AccArgs) <= 4096, "kernel arguments");

__device__ __forceinline__ float pick6(int lane, V3 lin, V3 ang) {
  return lane == 0 ? lin.x : (lane == 1 ? lin.y : (lane == 2 ? lin.z : (lane == 3 ? ang.x : (lane == 4 ? ang.y : ang.z))));
}

// inclusive prefix sum of a vector over the row (row_shr shifts zeros in: no lane test); n_max is uniform over the launch
template <int D>
__device__ __forceinline__ V3 psum_step(V3 v) { return v + v3(row_shr<D>(v.x), row_shr<D>(v.y), row_shr<D>(v.z)); }
__device__ __forceinline__ V3 psum3(V3 v, int n_max) {
  if (n_max > 1) v = psum_step<1>(v);
  if (n_max > 2) v = psum_step<2>(v);
  if (n_max > 4) v = psum_step<4>(v);
  if (n_max > 8) v = psum_step<8>(v);
  return v;
}

__global__ __launch_bounds__(64) void mir_acc_kernel(AccArgs a) {
  const PairLane t = pair_decode(a, a.n_links);
  const int lane = t.lane, pair = t.pair, row = t.row, li = t.item;
  const bool valid = t.valid;
  const PathLane e = path_lane(a.paths, li, lane);
  const int last4 = e.last4, jt = e.jt, dof = e.dof;
  const bool onpath = e.onpath;
  const float* const qrow = a.qpos + (size_t)t.env * a.qst;
  const float* const vrow = a.qvel + (size_t)t.env * a.vst;
  const float* const arow = a.qacc ? a.qacc + (size_t)row * a.nv : nullptr;
  // ---- local transform of my path element (identity off the path), my prefix of the path
  const JointLocal jl0 = joint_local(onpath, e.body, jt, qrow, a.m);
  const V3 baxis = jl0.baxis;
  const Pose me = path_scan(Pose{jl0.P, jl0.Qx}, lane, a.paths.n_max);
  const V3 P = me.P;
  const Q4 Qx = me.Qx;
  // ---- the link's rotation in every lane of the row, the queried point relative to the link's origin
  const Q4 ql = qnormalize(gather4(last4, Qx));
  const V3 r = qrot(ql, ld3(a.local_point[li]));
  // ---- my element's joint: world axis, qd, qdd (a free root: its four vectors)
  const bool hasdof = onpath && dof != NO_DOF;
  const bool rev = hasdof && jt == MIR_JNT_REVOLUTE, pri = hasdof && jt == MIR_JNT_PRISMATIC, free6 = hasdof && jt == MIR_JNT_FREE;
  V3 axw = v3(0, 0, 0), s = v3(0, 0, 0), fvd = v3(0, 0, 0), fwd = v3(0, 0, 0);
  float qd = 0.0f, qdd = 0.0f;
  if (rev || pri) {
    axw = qrot(Qx, baxis);
    qd = vrow[a.m.d_lane[dof]];
    qdd = arow ? arow[dof] : 0.0f;
    if (rev) s = qd * axw;
  }
  if (free6) {
    s = v3(vrow[a.m.d_lane[dof + 3]], vrow[a.m.d_lane[dof + 4]], vrow[a.m.d_lane[dof + 5]]);
    if (arow) {
      fvd = ld3(arow + dof);
      fwd = ld3(arow + dof + 3);
    }
  }
  // ---- angular velocities: w_j inclusive, w_{j-1} exclusive
  V3 wi = s;
  wi = psum3(wi, a.paths.n_max);
  const V3 wp = shr1(wi);
  // ---- angular accelerations, the part without qacc (b) and the part linear in it (a)
  const V3 wxa = cross(wp, axw);
  V3 ab = v3(0, 0, 0), aa = fwd;
  if (rev) {
    ab = qd * wxa;
    aa = qdd * axw;
  }
  ab = psum3(ab, a.paths.n_max);
  aa = psum3(aa, a.paths.n_max);
  const V3 abp = shr1(ab), aap = shr1(aa);
  // ---- my element's step of the origin's acceleration
  const V3 d = P - shr1(P);  // (lane 0: from the world's origin, which does not move)
  V3 tb = v3(0, 0, 0), ta = fvd;
  if (onpath && jt != MIR_JNT_FREE) {
    tb = cross(abp, d) + cross(wp, cross(wp, d));
    ta = cross(aap, d);
    if (pri) {
      tb = tb + (2.0f * qd) * wxa;
      ta = ta + qdd * axw;
    }
  }
  // ---- the link's w, alpha (the prefixes at the path's last element) and the point's acceleration (row all-reduce)
  const V3 w = gather3(last4, wi), alb = gather3(last4, ab), ala = gather3(last4, aa);
  const V3 lb = gsum3(tb) + cross(alb, r) + cross(w, cross(w, r));
  const V3 lin = lb + (gsum3(ta) + cross(ala, r));
  const V3 ang = alb + ala;
  if (!valid || lane >= 6) return;  // (no cross-lane op below)
  const size_t o = (size_t)pair * 6 + lane;
  if (a.bias) a.bias[o] = pick6(lane, lb, alb);
  if (a.acc) a.acc[o] = pick6(lane, lin, ang);
  if (a.imu) {
    const Q4 qs = qmul(ql, ld4(a.quat_offset[li]));
    const Q4 qc = Q4{qs.w, -qs.x, -qs.y, -qs.z};
    a.imu[o] = pick6(lane, qrot(qc, lin - v3(a.gx, a.gy, a.gz)), qrot(qc, w));
  }
}

}  // namespace

extern "C" int mir_acc_query_sizeof(void) { return (int)sizeof(MirAccQuery); }

extern "C" int mir_link_accelerations(MirHandle h, const MirAccQuery* q, const int64_t* env_idx, int32_t n_rows, const float* qacc, float* acc,
                                      float* bias_acc, float* imu, void* stream) {
  if (!h || !q) return mir_set_error(MIR_E_INVALID, "mir_link_accelerations: null argument");
  if (q->struct_size != (int32_t)sizeof(MirAccQuery)) return mir_set_error(MIR_E_INVALID, "mir_link_accelerations: struct_size is not sizeof(MirAccQuery)");
  if (q->flags != 0) return mir_set_error(MIR_E_INVALID, "mir_link_accelerations: unknown flag bit");
  if (q->n_links < 1 || q->n_links > MIR_MAX_BODY) return mir_set_error(MIR_E_INVALID, "mir_link_accelerations: n_links outside 1 .. MIR_MAX_BODY");
  for (int l = 0; l < q->n_links; l++) {
    if (q->link_body[l] <= 0 || q->link_body[l] >= h->nbody) return mir_set_error(MIR_E_INVALID, "mir_link_accelerations: link out of range");
    for (int k = 0; k < 3; k++)
      if (!std::isfinite(q->local_point[l][k])) return mir_set_error(MIR_E_INVALID, "mir_link_accelerations: local_point is not finite");
    for (int k = 0; k < 4; k++)
      if (!std::isfinite(q->quat_offset[l][k])) return mir_set_error(MIR_E_INVALID, "mir_link_accelerations: quat_offset is not finite");
  }
  if ((acc || imu) && !qacc) return mir_set_error(MIR_E_INVALID, "mir_link_accelerations: acc and imu need qacc");
  if (h->pending) return mir_set_error(MIR_E_INVALID, "mir_link_accelerations: a step is pending (mir_step_end first)");
  if (env_idx && n_rows < 0) return mir_set_error(MIR_E_INVALID, "mir_link_accelerations: negative n_rows");
  AccArgs a;
  memset(&a, 0, sizeof a);
  // (only here: a free body's qvel is a world velocity whatever is above it, so a free joint below another body is refused)
  if (int rc = build_link_paths(h, q->link_body, q->n_links, "mir_link_accelerations", true, a.paths)) return rc;
  for (int l = 0; l < q->n_links; l++) {
    for (int k = 0; k < 3; k++) a.local_point[l][k] = q->local_point[l][k];
    double n2 = 0.0;
    for (int k = 0; k < 4; k++) n2 += (double)q->quat_offset[l][k] * q->quat_offset[l][k];
    const double inv = n2 > 0.0 ? 1.0 / std::sqrt(n2) : 0.0;
    for (int k = 0; k < 4; k++) a.quat_offset[l][k] = n2 > 0.0 ? (float)(q->quat_offset[l][k] * inv) : (k == 0 ? 1.0f : 0.0f);
  }
  const int R = env_idx ? n_rows : h->B;
  if (R == 0 || (!acc && !bias_acc && !imu)) return MIR_OK;  // (nothing asked for)
  a.n_links = q->n_links;
  a.n_rows = R; a.B = h->B; a.qst = h->pt.qst; a.vst = h->pt.vst; a.nv = h->nv;
  const ModelView mv(h);
  mv.gravity(a.gx, a.gy, a.gz);
  a.env_idx = reinterpret_cast<const long long*>(env_idx);
  a.qpos = h->qpos; a.qvel = h->qvel; a.qacc = qacc;
  a.m = mv.joint_pointers();
  a.acc = acc; a.bias = bias_acc; a.imu = imu;
  const long long n_pairs = (long long)R * q->n_links;
  if (n_pairs > 0x7fffffffLL - 4) return mir_set_error(MIR_E_CAPACITY, "mir_link_accelerations: rows x links reaches 2^31");
  return launch_rows(h, mir_acc_kernel, (n_pairs + 3) / 4, stream, a);
}
