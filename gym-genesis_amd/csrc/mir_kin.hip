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

namespace {

constexpr int KIN_NO_DOF = 0xff;

struct KinArgs {
  // element j of link l's path: body | jtype << 8 | first dof of the body << 16 (KIN_NO_DOF: none)
  uint32_t elem[MIR_MAX_BODY][G];
  uint8_t n[MIR_MAX_BODY];          // bodies on the path of link l
  float local_point[MIR_MAX_BODY][3];
  int n_links, n_max;               // n_max: the longest path (how many scan steps the wave takes)
  int dof0, n_dofs;
  int n_rows, B, qst, vst;
  int vec4;                         // jac is 16-byte aligned: the span goes out as float4
  const long long* env_idx;
  const float *qpos, *qvel;
  // per-body constants of the device model (DevModel or DevModel64: same shapes)
  const float *b_pos, *b_quat, *b_axis;  // [.][3], [.][4], [.][3]
  const int32_t* b_qadr;
  const int32_t* d_lane;            // PlumbTab::d_lane: dof -> column of the qvel row
  float *pos, *quat, *vel, *jac;
};

__global__ __launch_bounds__(64) void mir_kin_kernel(KinArgs a) {
  __shared__ float4 jl4[4 * 6 * MIR_MAX_DOF / 4];
  float* const jl = reinterpret_cast<float*>(jl4);
  const int tid = threadIdx.x, lane = tid & 15, grp = tid >> 4;
  const int n_pairs = a.n_rows * a.n_links;
  const int pair_raw = blockIdx.x * 4 + grp;
  const bool valid = pair_raw < n_pairs;
  const int pair = valid ? pair_raw : n_pairs - 1;
  const int row = pair / a.n_links, li = pair - row * a.n_links;
  int env = a.env_idx ? (int)a.env_idx[row] : row;
  env = env < 0 ? 0 : (env >= a.B ? a.B - 1 : env);  // (an index outside the batch is clamped, not followed: the caller's side checks it)
  const int n = a.n[li];
  const int last4 = ((tid & ~15) + n - 1) << 2;  // (lane_gather address of the path's last element in this pair's row)
  const bool onpath = lane < n;
  const uint32_t el = onpath ? a.elem[li][lane] : (uint32_t)(MIR_JNT_FIXED << 8 | KIN_NO_DOF << 16);
  const int body = el & 0xff, jt = (el >> 8) & 0xff, dof = (el >> 16) & 0xff;
  const float* const qrow = a.qpos + (size_t)env * a.qst;
  const float* const vrow = a.qvel + (size_t)env * a.vst;
  // ---- local transform of my path element (identity off the path)
  V3 P = v3(0, 0, 0), baxis = v3(0, 0, 0);
  Q4 Qx = Q4{1, 0, 0, 0};
  if (onpath) {
    const int qa = a.b_qadr[body];
    if (jt == MIR_JNT_FREE) {
      P = ld3(qrow + qa);
      Qx = qnormalize(ld4(qrow + qa + 3));
    } else {
      const Q4 bquat = ld4(a.b_quat + body * 4);
      P = ld3(a.b_pos + body * 3);
      Qx = bquat;
      baxis = ld3(a.b_axis + body * 3);
      if (jt == MIR_JNT_REVOLUTE) {
        float sn, cs;
        sincos_pi2(0.5f * qrow[qa], &sn, &cs);
        Qx = qmul(bquat, Q4{cs, baxis.x * sn, baxis.y * sn, baxis.z * sn});
      } else if (jt == MIR_JNT_PRISMATIC) {
        P = P + qrot(bquat, qrow[qa] * baxis);
      }
    }
  }
  // ---- my prefix of the path by a log-step scan over the DPP row ((P,Q) o (p,q) = (P + Q p, Q q) is associative)
#define KIN_SCAN_STEP(D)                                                                                       \
  {                                                                                                            \
    const V3 pp = v3(row_shr<D>(P.x), row_shr<D>(P.y), row_shr<D>(P.z));                                       \
    const Q4 pq = Q4{row_shr<D>(Qx.w), row_shr<D>(Qx.x), row_shr<D>(Qx.y), row_shr<D>(Qx.z)};                  \
    if (lane >= D) {                                                                                           \
      P = pp + qrot(pq, P);                                                                                    \
      Qx = qmul(pq, Qx);                                                                                       \
    }                                                                                                          \
  }
  if (a.n_max > 1) KIN_SCAN_STEP(1)
  if (a.n_max > 2) KIN_SCAN_STEP(2)
  if (a.n_max > 4) KIN_SCAN_STEP(4)
  if (a.n_max > 8) KIN_SCAN_STEP(8)
#undef KIN_SCAN_STEP
  // ---- the link's pose in every lane of the row (seven lane gathers), the queried point
  const V3 ol = v3(lane_gather(last4, P.x), lane_gather(last4, P.y), lane_gather(last4, P.z));
  const Q4 ql = qnormalize(Q4{lane_gather(last4, Qx.w), lane_gather(last4, Qx.x), lane_gather(last4, Qx.y), lane_gather(last4, Qx.z)});
  const V3 p = ol + qrot(ql, ld3(a.local_point[li]));
  // ---- my column(s) and my share of J qvel
  const V3 r = p - P;
  float c0[6] = {0, 0, 0, 0, 0, 0}, pv[6] = {0, 0, 0, 0, 0, 0};
  const bool scalar = onpath && dof != KIN_NO_DOF && (jt == MIR_JNT_REVOLUTE || jt == MIR_JNT_PRISMATIC);
  const bool free6 = onpath && dof != KIN_NO_DOF && jt == MIR_JNT_FREE;
  if (scalar) {
    const V3 axw = qrot(Qx, baxis);
    V3 jv = axw, jw = v3(0, 0, 0);
    if (jt == MIR_JNT_REVOLUTE) { jw = axw; jv = cross(axw, r); }
    c0[0] = jv.x; c0[1] = jv.y; c0[2] = jv.z; c0[3] = jw.x; c0[4] = jw.y; c0[5] = jw.z;
    const float qd = vrow[a.d_lane[dof]];
#pragma unroll
    for (int k = 0; k < 6; k++) pv[k] = c0[k] * qd;
  }
  if (free6) {
    const V3 v = v3(vrow[a.d_lane[dof]], vrow[a.d_lane[dof + 1]], vrow[a.d_lane[dof + 2]]);
    const V3 w = v3(vrow[a.d_lane[dof + 3]], vrow[a.d_lane[dof + 4]], vrow[a.d_lane[dof + 5]]);
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
  const bool k16 = h->kernel == 16;
  auto parent = [&](int b) { return k16 ? h->hm.b_parent[b] : h->hm64.b_parent[b]; };
  auto jtype = [&](int b) { return k16 ? h->hm.b_jtype[b] : h->hm64.b_jtype[b]; };
  // first dof of a body in the scene's dof order (the wave kernel's model addresses dofs by lane: d_dof maps back)
  auto dofadr = [&](int b) { return k16 ? h->hm.b_dofadr[b] : h->hm64.d_dof[h->hm64.b_dofadr[b]]; };
  for (int l = 0; l < q->n_links; l++) {
    int path[G], n = 0;
    for (int b = q->link_body[l]; b > 0; b = parent(b)) {
      if (n >= G) return mir_set_error(MIR_E_CAPACITY, "mir_link_kinematics: path longer than 16 bodies");
      path[n++] = b;
    }
    for (int i = 0; i < n; i++) {
      const int b = path[n - 1 - i], jt = jtype(b);
      const int d = jt == MIR_JNT_FIXED ? KIN_NO_DOF : dofadr(b);
      a.elem[l][i] = (uint32_t)b | (uint32_t)jt << 8 | (uint32_t)d << 16;
    }
    a.n[l] = (uint8_t)n;
    if (n > a.n_max) a.n_max = n;
    for (int k = 0; k < 3; k++) a.local_point[l][k] = q->local_point[l][k];
  }
  const int R = env_idx ? n_rows : h->B;
  if (q->n_dofs == 0) jac = nullptr;  // (an empty block)
  if (R == 0 || (!pos && !quat && !vel && !jac)) return MIR_OK;  // (nothing asked for)
  a.n_links = q->n_links; a.dof0 = q->dof0; a.n_dofs = q->n_dofs;
  a.n_rows = R; a.B = h->B; a.qst = h->pt.qst; a.vst = h->pt.vst;
  a.vec4 = ((uintptr_t)jac & 15) == 0;
  a.env_idx = reinterpret_cast<const long long*>(env_idx);
  a.qpos = h->qpos; a.qvel = h->qvel;
  const char* const dm = k16 ? reinterpret_cast<const char*>(h->dm) : reinterpret_cast<const char*>(h->dm64);
  a.b_pos = reinterpret_cast<const float*>(dm + (k16 ? offsetof(DevModel, b_pos) : offsetof(DevModel64, b_pos)));
  a.b_quat = reinterpret_cast<const float*>(dm + (k16 ? offsetof(DevModel, b_quat) : offsetof(DevModel64, b_quat)));
  a.b_axis = reinterpret_cast<const float*>(dm + (k16 ? offsetof(DevModel, b_axis) : offsetof(DevModel64, b_axis)));
  a.b_qadr = reinterpret_cast<const int32_t*>(dm + (k16 ? offsetof(DevModel, b_qadr) : offsetof(DevModel64, b_qadr)));
  a.d_lane = reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(h->dpt) + offsetof(PlumbTab, d_lane));
  a.pos = pos; a.quat = quat; a.vel = vel; a.jac = jac;
  const long long n_pairs = (long long)R * q->n_links;
  if (n_pairs > 0x7fffffffLL - 4) return mir_set_error(MIR_E_CAPACITY, "mir_link_kinematics: rows x links reaches 2^31");
  int prev = -1;
  (void)hipGetDevice(&prev);
  if (prev != h->device) (void)hipSetDevice(h->device);
  hipLaunchKernelGGL(mir_kin_kernel, dim3((unsigned)((n_pairs + 3) / 4)), dim3(64), 0, (hipStream_t)stream, a);
  hipError_t e = hipGetLastError();
  if (prev != h->device && prev >= 0) (void)hipSetDevice(prev);
  if (e != hipSuccess) return mir_set_error(MIR_E_HIP, hipGetErrorString(e));
  return MIR_OK;
}
