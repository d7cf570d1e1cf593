// mir_kin.hip — link poses, velocities and geometric Jacobians of a list of links in one batched launch (mir_link_kinematics,
// include/mirigid.h; DESIGN.md sensor-2).
//
// What it serves: robot.get_jacobian(link), entity.get_links_vel / get_links_ang / get_links_pos / get_links_quat and link.get_vel()
// of Genesis's RigidEntity / RigidLink -- differential kinematics of a few links of a few envs, without the step kernel's mode-2
// launch over every body of every env.  It reads qpos / qvel and the compiled model and writes only its own outputs.
//
// Mapping (the one mir_ik.hip proves out): 16 lanes = one DPP row serve one (row, link) PAIR, four pairs per wave64.  Lane j owns
// element j of the path world -> link (root first, <= 16 bodies): its local joint transform from qpos (a free root's "local transform"
// is its qpos pose), its world pose as the prefix of the path by the log-step DPP row scan, its Jacobian column(s) and its share of
// J qvel in registers.  The link's pose reaches all 16 lanes over the crossbar; vel is the row all-reduce of the partial products.
// The path description (body indices, joint types, dof addresses: 4 bytes per element) is built on the host per call and travels in
// the kernel arguments; the per-body constants come from the device model of whichever step kernel serves the scene (both models
// hold the same per-body arrays; the launch passes their addresses), the state rows are 16 or 64 floats wide.
//
// Stores: a Jacobian block is 6 x n_dofs floats, mostly zeros.  The four blocks of a wave are assembled in LDS (4 x 6 x 48 x 4 B at
// most), where every lane can reach them, and written out as ONE contiguous span, 16 bytes per lane: the span of wave w starts at
// float 24 n_dofs w of the array, a multiple of 16 bytes whatever n_dofs is.  No atomics.  Whole waves reach every DPP / gather: the
// pairs behind the last one are clamped to it and their stores predicated.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <cstring>

#include "mir_model.h"
#include "mir_model64.h"
#include "mir_scene.h"

#define G 16
#include "mir_dev.h"

#include "mir_query.h"

namespace {

struct KinArgs {
  LinkPaths paths;
  float local_point[MIR_MAX_BODY][3];
  int n_links;
  int dof0, n_dofs;
  int n_rows, B, qst, vst;
  int vec4;                         // jac is 16-byte aligned: the span goes out as float4
  const long long* env_idx;
  const float *qpos, *qvel;
  JointPtrs m;
  float *pos, *quat, *vel, *jac;
};
static_assert(sizeof(KinArgs) <= 4096, "kernel arguments");

__global__ __launch_bounds__(64) void mir_kin_kernel(KinArgs a) {
  __shared__ float4 jl4[4 * 6 * MIR_MAX_DOF / 4];
  float* const jl = reinterpret_cast<float*>(jl4);
  const PairLane t = pair_decode(a, a.n_links);
  const int tid = threadIdx.x, lane = t.lane, grp = t.grp, pair = t.pair, li = t.item;
  const bool valid = t.valid;
  const int n_pairs = a.n_rows * a.n_links;
  const PathLane e = path_lane(a.paths, li, lane);
  const int last4 = e.last4, jt = e.jt, dof = e.dof;
  const bool onpath = e.onpath;
  const float* const qrow = a.qpos + (size_t)t.env * a.qst;
  const float* const vrow = a.qvel + (size_t)t.env * a.vst;
  // ---- local transform of my path element (identity off the path), my prefix of the path
  const JointLocal jl0 = joint_local(onpath, e.body, jt, qrow, a.m);
  const V3 baxis = jl0.baxis;
  const Pose me = path_scan(Pose{jl0.P, jl0.Qx}, lane, a.paths.n_max);
  const V3 P = me.P;
  const Q4 Qx = me.Qx;
  // ---- the link's pose in every lane of the row (seven lane gathers), the queried point
  const V3 ol = gather3(last4, P);
  const Q4 ql = qnormalize(gather4(last4, Qx));
  const V3 p = ol + qrot(ql, ld3(a.local_point[li]));
  // ---- my column(s) and my share of J qvel
  const V3 r = p - P;
  float c0[6] = {0, 0, 0, 0, 0, 0}, pv[6] = {0, 0, 0, 0, 0, 0};
  const bool scalar = onpath && dof != NO_DOF && (jt == MIR_JNT_REVOLUTE || jt == MIR_JNT_PRISMATIC);
  const bool free6 = onpath && dof != NO_DOF && jt == MIR_JNT_FREE;
  if (scalar) {
    const V3 axw = qrot(Qx, baxis);
    V3 jv = axw, jw = v3(0, 0, 0);
    if (jt == MIR_JNT_REVOLUTE) { jw = axw; jv = cross(axw, r); }
    c0[0] = jv.x; c0[1] = jv.y; c0[2] = jv.z; c0[3] = jw.x; c0[4] = jw.y; c0[5] = jw.z;
    const float qd = vrow[a.m.d_lane[dof]];
#pragma unroll
    for (int k = 0; k < 6; k++) pv[k] = c0[k] * qd;
  }
  if (free6) {
    const V3 v = v3(vrow[a.m.d_lane[dof]], vrow[a.m.d_lane[dof + 1]], vrow[a.m.d_lane[dof + 2]]);
    const V3 w = v3(vrow[a.m.d_lane[dof + 3]], vrow[a.m.d_lane[dof + 4]], vrow[a.m.d_lane[dof + 5]]);
    const V3 u = v + cross(w, r);
    pv[0] = u.x; pv[1] = u.y; pv[2] = u.z; pv[3] = w.x; pv[4] = w.y; pv[5] = w.z;
  }
  float vel[6];
#pragma unroll
  for (int k = 0; k < 6; k++) vel[k] = gsum(pv[k]);
  // ---- pose and velocity: the pairs of a wave are neighbours in every output, lane k of a row stores component k
  if (valid) {
    if (a.pos && lane < 3) a.pos[(size_t)pair * 3 + lane] = lane == 0 ? p.x : (lane == 1 ? p.y : p.z);
    if (a.quat && lane < 4) a.quat[(size_t)pair * 4 + lane] = lane == 0 ? ql.w : (lane == 1 ? ql.x : (lane == 2 ? ql.y : ql.z));
    if (a.vel && lane < 6) {
      float s = vel[0];
#pragma unroll
      for (int k = 1; k < 6; k++) s = lane == k ? vel[k] : s;
      a.vel[(size_t)pair * 6 + lane] = s;
    }
  }
  if (!a.jac) return;  // (uniform over the launch)
  // ---- the Jacobian blocks of the wave's four pairs, assembled in LDS: zeros, then every path lane's column(s) inside the range
  const int nd = a.n_dofs, blk = 6 * nd;
  float* const mine = jl + grp * blk;
  for (int i = lane; i < blk; i += G) mine[i] = 0.0f;
  WSYNC();
  if (scalar) {
    const int c = dof - a.dof0;
    if (c >= 0 && c < nd) {
#pragma unroll
      for (int k = 0; k < 6; k++) mine[k * nd + c] = c0[k];
    }
  }
  if (free6) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const int cl = dof + k - a.dof0, ca = cl + 3;
      if (cl >= 0 && cl < nd) mine[k * nd + cl] = 1.0f;  // [e_k; 0]
      if (ca >= 0 && ca < nd) {                          // [e_k x r; e_k]
        const V3 ek = v3(k == 0 ? 1.0f : 0.0f, k == 1 ? 1.0f : 0.0f, k == 2 ? 1.0f : 0.0f);
        const V3 jv = cross(ek, r);
        mine[0 * nd + ca] = jv.x; mine[1 * nd + ca] = jv.y; mine[2 * nd + ca] = jv.z;
        mine[(3 + k) * nd + ca] = 1.0f;
      }
    }
  }
  WSYNC();
  // ---- ... and written out as one contiguous span (the valid pairs of a wave are its first ones)
  const int first = blockIdx.x * 4;
  const int n_here = n_pairs - first < 4 ? n_pairs - first : 4;
  const int span = n_here * blk;  // floats
  float* const out = a.jac + (size_t)first * blk;
  int done = 0;
  if (a.vec4) {
    const int span4 = span >> 2;
    float4* const out4 = reinterpret_cast<float4*>(out);
    for (int i = tid; i < span4; i += 64) out4[i] = jl4[i];
    done = span4 << 2;
  }
  for (int i = done + tid; i < span; i += 64) out[i] = jl[i];
}

}  // namespace

extern "C" int mir_kin_query_sizeof(void) { return (int)sizeof(MirKinQuery); }

extern "C" int mir_link_kinematics(MirHandle h, const MirKinQuery* q, const int64_t* env_idx, int32_t n_rows, float* pos, float* quat, float* vel,
                                   float* jac, void* stream) {
  if (!h || !q) return mir_set_error(MIR_E_INVALID, "mir_link_kinematics: null argument");
  if (q->struct_size != (int32_t)sizeof(MirKinQuery)) return mir_set_error(MIR_E_INVALID, "mir_link_kinematics: struct_size is not sizeof(MirKinQuery)");
  if (q->n_links < 1 || q->n_links > MIR_MAX_BODY) return mir_set_error(MIR_E_INVALID, "mir_link_kinematics: n_links outside 1 .. MIR_MAX_BODY");
  for (int l = 0; l < q->n_links; l++)
    if (q->link_body[l] <= 0 || q->link_body[l] >= h->nbody) return mir_set_error(MIR_E_INVALID, "mir_link_kinematics: link out of range");
  if (q->dof0 < 0 || q->n_dofs < 0 || q->dof0 > h->nv || q->n_dofs > h->nv - q->dof0)
    return mir_set_error(MIR_E_INVALID, "mir_link_kinematics: dof columns outside [0, nv]");
  if (h->pending) return mir_set_error(MIR_E_INVALID, "mir_link_kinematics: a step is pending (mir_step_end first)");
  if (env_idx && n_rows < 0) return mir_set_error(MIR_E_INVALID, "mir_link_kinematics: negative n_rows");
  KinArgs a;
  memset(&a, 0, sizeof a);
  if (int rc = build_link_paths(h, q->link_body, q->n_links, "mir_link_kinematics", false, a.paths)) return rc;
  for (int l = 0; l < q->n_links; l++)
    for (int k = 0; k < 3; k++) a.local_point[l][k] = q->local_point[l][k];
  const int R = env_idx ? n_rows : h->B;
  if (q->n_dofs == 0) jac = nullptr;  // (an empty block)
  if (R == 0 || (!pos && !quat && !vel && !jac)) return MIR_OK;  // (nothing asked for)
  a.n_links = q->n_links; a.dof0 = q->dof0; a.n_dofs = q->n_dofs;
  a.n_rows = R; a.B = h->B; a.qst = h->pt.qst; a.vst = h->pt.vst;
  a.vec4 = ((uintptr_t)jac & 15) == 0;
  a.env_idx = reinterpret_cast<const long long*>(env_idx);
  a.qpos = h->qpos; a.qvel = h->qvel;
  a.m = ModelView(h).joint_pointers();
  a.pos = pos; a.quat = quat; a.vel = vel; a.jac = jac;
  const long long n_pairs = (long long)R * q->n_links;
  if (n_pairs > 0x7fffffffLL - 4) return mir_set_error(MIR_E_CAPACITY, "mir_link_kinematics: rows x links reaches 2^31");
  return launch_rows(h, mir_kin_kernel, (n_pairs + 3) / 4, stream, a);
}
