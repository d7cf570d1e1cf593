// mir_query.h — the front end the batched query kernels share (mir_kin.hip, mir_acc.hip, mir_dyn.hip and mir_osc.hip on the device side,
// mir_ik.hip and mir_ikm.hip for the pose scan and the gathers; those and mir_ray.hip on the host side).
//   device: the (row, item) pair a 16-lane DPP row serves, the local joint transform of one body from a qpos row, the log-step pose scan
//           along a world -> link path, and the path element of a lane;
//   host:   a view of whichever compiled model serves the scene (DevModel or DevModel64), the addresses of its per-body / per-dof arrays
//           on the device, the world -> link paths of a list of links, error texts that name the entry point, and the launch.
// Included after mir_dev.h with G = 16, inside no namespace.
#pragma once
#include <stddef.h>
#include <stdio.h>

#include "mir_guard.h"

namespace {

// ---- addresses in the device model (DevModel or DevModel64: same shapes; per-dof arrays are indexed by the dof's lane,
// PlumbTab::d_lane) and in PlumbTab, as the kernels read them, in three groups so that a kernel's arguments carry what it reads.
// Filled by ModelView::joint_pointers() / inertia_pointers() / control_pointers().
struct JointPtrs {  // what joint_local() and the qvel look-ups read: every query kernel
  const float *b_pos, *b_quat, *b_axis;  // [.][3], [.][4], [.][3]
  const int32_t* b_qadr;
  const int32_t* d_lane;                 // PlumbTab: dof -> column of the qvel row
};
struct InertiaPtrs {  // the M block: mir_dyn_phases.inc
  const float *b_ipos, *b_inertia, *b_mass, *d_armature;  // [.][3], [.][6], [.], [lane]
};
struct ControlPtrs {  // the PD torque of mir_dynamics
  const float *d_kp, *d_kv, *d_frclo, *d_frchi;
  const int32_t *d_ctrl, *d_qadr;  // d_qadr: PlumbTab, dof -> qpos address
};

constexpr int NO_DOF = 0xff;  // "no dof" in a path element

// the paths world -> link of a list of links (root first, <= 16 bodies each); filled by build_link_paths()
struct LinkPaths {
  uint32_t elem[MIR_MAX_BODY][G];  // element j of link l's path: body | jtype << 8 | first dof of the body << 16 (NO_DOF: none)
  uint8_t n[MIR_MAX_BODY];         // bodies on the path of link l
  int n_max;                       // the longest path (how many scan steps the wave takes)
};

// ---- device: 16 lanes = one DPP row serve one (row, item) PAIR, four pairs per wave64.  Whole waves reach every DPP op / gather: the
// pairs behind the last one are clamped to it (`valid` predicates their stores).
struct PairLane {
  int lane, grp, pair, row, item, env;
  bool valid;
};
template <class Args>
__device__ __forceinline__ PairLane pair_decode(const Args& a, int n_items) {  // Args has n_rows, B, env_idx; n_items: links or trees
  PairLane t;
  const int tid = threadIdx.x;
  t.lane = tid & 15;
  t.grp = tid >> 4;
  const int n_pairs = a.n_rows * n_items;
  const int pair_raw = blockIdx.x * 4 + t.grp;
  t.valid = pair_raw < n_pairs;
  t.pair = t.valid ? pair_raw : n_pairs - 1;
  t.row = t.pair / n_items;
  t.item = t.pair - t.row * n_items;
  const int env = a.env_idx ? (int)a.env_idx[t.row] : t.row;
  t.env = env < 0 ? 0 : (env >= a.B ? a.B - 1 : env);  // (an index outside the batch is clamped, not followed: the caller's side checks it)
  return t;
}

// ---- device: what a lane is on the path of link `li`: element `lane` of it, or nothing (a fixed joint without a dof) behind its end
struct PathLane {
  int n, last4;  // bodies on the path; lane_gather address of the path's last element in this pair's row
  bool onpath;
  int body, jt, dof;
};
__device__ __forceinline__ PathLane path_lane(const LinkPaths& p, int li, int lane) {
  PathLane e;
  e.n = p.n[li];
  e.last4 = ((threadIdx.x & ~15) + e.n - 1) << 2;
  e.onpath = lane < e.n;
  const uint32_t el = e.onpath ? p.elem[li][lane] : (uint32_t)(MIR_JNT_FIXED << 8 | NO_DOF << 16);
  e.body = el & 0xff;
  e.jt = (el >> 8) & 0xff;
  e.dof = (el >> 16) & 0xff;
  return e;
}

// ---- device: the local transform of one body from the qpos row (a free body's "local transform" is its qpos pose); the identity and a
// zero axis where `on` is false.  Returned by value (see path_scan).
struct JointLocal {
  V3 P;      // position and rotation of the body in its parent's frame (a free body: in the world's)
  Q4 Qx;
  V3 baxis;  // the joint's axis in the body's frame
};
__device__ __forceinline__ JointLocal joint_local(bool on, int body, int jt, const float* qrow, const JointPtrs& m) {
  V3 P = v3(0, 0, 0), baxis = v3(0, 0, 0);
  Q4 Qx = Q4{1, 0, 0, 0};
  if (on) {
    const int qa = m.b_qadr[body];
    if (jt == MIR_JNT_FREE) {
      P = ld3(qrow + qa);
      Qx = qnormalize(ld4(qrow + qa + 3));
    } else {
      const Q4 bquat = ld4(m.b_quat + body * 4);
      P = ld3(m.b_pos + body * 3);
      Qx = bquat;
      baxis = ld3(m.b_axis + body * 3);
      if (jt == MIR_JNT_REVOLUTE) {
        float sn, cs;
        sincos_pi2(0.5f * qrow[qa], &sn, &cs);
        Qx = qmul(bquat, Q4{cs, baxis.x * sn, baxis.y * sn, baxis.z * sn});
      } else if (jt == MIR_JNT_PRISMATIC) {
        P = P + qrot(bquat, qrow[qa] * baxis);
      }
    }
  }
  return {P, Qx, baxis};
}

// ---- device: small vector forms of the row primitives of mir_dev.h
__device__ __forceinline__ V3 shr1(V3 v) { return v3(row_shr<1>(v.x), row_shr<1>(v.y), row_shr<1>(v.z)); }
__device__ __forceinline__ V3 gather3(int src4, V3 v) { return v3(lane_gather(src4, v.x), lane_gather(src4, v.y), lane_gather(src4, v.z)); }
__device__ __forceinline__ Q4 gather4(int src4, Q4 q) {
  return Q4{lane_gather(src4, q.w), lane_gather(src4, q.x), lane_gather(src4, q.y), lane_gather(src4, q.z)};
}
__device__ __forceinline__ V3 gsum3(V3 v) { return v3(gsum(v.x), gsum(v.y), gsum(v.z)); }

// ---- device: my prefix of the path by a log-step scan over the DPP row ((P,Q) o (p,q) = (P + Q p, Q q) is associative); n_max is
// uniform over the launch.  (Like joint_local, by value in and out: with reference parameters the compiler keeps the poses in memory
// until after inlining, and the kernels come out with another register allocation.)
struct Pose {
  V3 P;
  Q4 Qx;
};
template <int D>
__device__ __forceinline__ Pose path_scan_step(Pose x, int lane) {
  const V3 pp = v3(row_shr<D>(x.P.x), row_shr<D>(x.P.y), row_shr<D>(x.P.z));
  const Q4 pq = Q4{row_shr<D>(x.Qx.w), row_shr<D>(x.Qx.x), row_shr<D>(x.Qx.y), row_shr<D>(x.Qx.z)};
  if (lane >= D) {
    x.P = pp + qrot(pq, x.P);
    x.Qx = qmul(pq, x.Qx);
  }
  return x;
}
__device__ __forceinline__ Pose path_scan(Pose x, int lane, int n_max) {
  if (n_max > 1) x = path_scan_step<1>(x, lane);
  if (n_max > 2) x = path_scan_step<2>(x, lane);
  if (n_max > 4) x = path_scan_step<4>(x, lane);
  if (n_max > 8) x = path_scan_step<8>(x, lane);
  return x;
}

// ---- host: the compiled model that serves the scene, whichever of the two it is
struct ModelView {
  const MirHandle h;
  const bool k16;  // the 16-lane kernel's model (DevModel), else the wave kernel's (DevModel64)
  explicit ModelView(MirHandle h_) : h(h_), k16(h_->kernel == 16) {}
  template <class F>
  auto on(F f) const { return k16 ? f(h->hm) : f(h->hm64); }
  int parent(int b) const { return on([&](const auto& m) { return (int)m.b_parent[b]; }); }
  int jtype(int b) const { return on([&](const auto& m) { return (int)m.b_jtype[b]; }); }
  int qadr(int b) const { return on([&](const auto& m) { return (int)m.b_qadr[b]; }); }
  int ndof(int b) const { const int jt = jtype(b); return jt == MIR_JNT_FREE ? 6 : (jt == MIR_JNT_FIXED ? 0 : 1); }
  // first dof of a body in the scene's dof order (the wave kernel's model addresses dofs by lane: d_dof maps back)
  int dofadr(int b) const { return k16 ? h->hm.b_dofadr[b] : h->hm64.d_dof[h->hm64.b_dofadr[b]]; }
  void gravity(float& gx, float& gy, float& gz) const { on([&](const auto& m) { gx = m.gx; gy = m.gy; gz = m.gz; return 0; }); }
  const float* body_pos(int b) const { return on([&](const auto& m) { return (const float*)m.b_pos[b]; }); }
  const float* body_quat(int b) const { return on([&](const auto& m) { return (const float*)m.b_quat[b]; }); }
  const float* body_axis(int b) const { return on([&](const auto& m) { return (const float*)m.b_axis[b]; }); }
  // the limits of the body's first dof
  void limits(int b, double& lo, double& hi, int& limited) const {
    on([&](const auto& m) { const int d = m.b_dofadr[b]; lo = m.d_lo[d]; hi = m.d_hi[d]; limited = m.d_limited[d]; return 0; });
  }
  // the addresses of the model's per-body / per-dof arrays on the device
  const char* dev_model() const { return k16 ? reinterpret_cast<const char*>(h->dm) : reinterpret_cast<const char*>(h->dm64); }
#define MODEL_F(name) reinterpret_cast<const float*>(dev_model() + (k16 ? offsetof(DevModel, name) : offsetof(DevModel64, name)))
#define MODEL_I(name) reinterpret_cast<const int32_t*>(dev_model() + (k16 ? offsetof(DevModel, name) : offsetof(DevModel64, name)))
#define PLUMB_I(name) reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(h->dpt) + offsetof(PlumbTab, name))
  JointPtrs joint_pointers() const { return {MODEL_F(b_pos), MODEL_F(b_quat), MODEL_F(b_axis), MODEL_I(b_qadr), PLUMB_I(d_lane)}; }
  InertiaPtrs inertia_pointers() const { return {MODEL_F(b_ipos), MODEL_F(b_inertia), MODEL_F(b_mass), MODEL_F(d_armature)}; }
  ControlPtrs control_pointers() const {
    return {MODEL_F(d_kp), MODEL_F(d_kv), MODEL_F(d_frclo), MODEL_F(d_frchi), MODEL_I(d_ctrl), PLUMB_I(d_qadr)};
  }
#undef MODEL_F
#undef MODEL_I
#undef PLUMB_I
};

// ---- host: an error whose text names the entry point, "<who>: <what>"
static int query_error(int code, const char* who, const char* what) {
  char msg[256];
  snprintf(msg, sizeof msg, "%s: %s", who, what);
  return mir_set_error(code, msg);
}

// ---- host: the paths world -> link_body[l], root first
static int build_link_paths(MirHandle h, const int32_t* link_body, int n_links, const char* who, bool free_must_be_root, LinkPaths& out) {
  const ModelView mv(h);
  out.n_max = 0;
  for (int l = 0; l < n_links; l++) {
    int path[G], n = 0;
    for (int b = link_body[l]; b > 0; b = mv.parent(b)) {
      if (n >= G) return query_error(MIR_E_CAPACITY, who, "path longer than 16 bodies");
      // (a free body's qvel is a world velocity whatever is above it: below another body the path would mix two conventions)
      if (free_must_be_root && mv.jtype(b) == MIR_JNT_FREE && mv.parent(b) != 0) return query_error(MIR_E_INVALID, who, "a free joint below another body");
      path[n++] = b;
    }
    for (int i = 0; i < n; i++) {
      const int b = path[n - 1 - i], jt = mv.jtype(b);
      const int d = jt == MIR_JNT_FIXED ? NO_DOF : mv.dofadr(b);
      out.elem[l][i] = (uint32_t)b | (uint32_t)jt << 8 | (uint32_t)d << 16;
    }
    out.n[l] = (uint8_t)n;
    if (n > out.n_max) out.n_max = n;
  }
  return MIR_OK;
}

// ---- host: one launch of n_groups workgroups of TPB threads (and dyn_lds bytes of dynamic LDS each) on the scene's device
template <int TPB = 64, class Args>
static int launch_rows(MirHandle h, void (*kernel)(Args), long long n_groups, void* stream, const Args& a, size_t dyn_lds = 0) {
  DeviceGuard guard(h->device);
  hipLaunchKernelGGL(kernel, dim3((unsigned)n_groups), dim3(TPB), dyn_lds, (hipStream_t)stream, a);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MIR_OK : mir_set_error(MIR_E_HIP, hipGetErrorString(e));
}

}  // namespace
