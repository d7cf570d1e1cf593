// mir_dyn.hip — joint-space mass matrix, bias forces, gravity forces, inverse dynamics and PD control forces of a window of scene dofs
// in one batched launch (mir_dynamics, include/mirigid.h; DESIGN.md sensor-4).
//
// What it serves: entity.get_mass_mat() and entity.get_dofs_control_force() of Genesis's RigidEntity, and gravity compensation /
// feed-forward torques tau = M qacc + c along a planned trajectory -- the objects operational-space and impedance controllers are
// written on beside the Jacobian of mir_kin.hip -- without mir_forward's full step-kernel launch over every env (collision, constraint
// rows, Newton solve).  It reads qpos / qvel / targets and the compiled model and writes only its own outputs.
//
// Definitions: the oracle's (oracle/orc_rigid.c: orc_fk, orc_crb, orc_rne, orc_smooth).  Spatial quantities live in the per-tree frame
// the step kernels use -- world axes, origin at the tree's root body -- so float32 error stays where theirs is.
//
// Mapping: 16 lanes = one DPP row serve one (row, kinematic tree) PAIR, four pairs per wave64.  In the first half lane j is BODY j of
// the tree (body order, so a parent comes before its children): local joint transform from qpos, world pose level by level through
// LDS (the composition order of the serial walk), spatial inertia about the tree origin, the motion subspaces of its own dofs, and the
// Newton-Euler velocities / accelerations / forces root to leaf.  In the second half lane i is DOF i of the tree: the composite
// inertia and the force of its body's subtree are sums over the subtree's bodies (a 16-bit mask per body, ascending order: no
// leaf-to-root pass in which two children would meet at their parent, hence no atomics), M[i][j] is walked up dof_parent and written
// to both triangles of the tree's 16 x 16 block in LDS by lane i alone.  The tree description (4 bytes per body, 4 per dof, a subtree
// mask per body) is built on the host per call and travels in the kernel arguments; the per-body and per-dof constants come from the
// device model of whichever step kernel serves the scene (both hold the same arrays; the launch passes their addresses).
// A single free body is a tree of one body and six dofs: the general path with r = 0 IS its closed form (M = diag(m 1, R I R^T) about
// the MIR_JNT_FREE origin convention when the centre of mass is at the origin, bias = -m g plus the gyroscopic term).
//
// Stores: row i of the M window belongs to the tree of dof i, which writes all n_dofs columns of it -- its own block from LDS, exact
// zeros for the dofs of other trees -- as contiguous runs, 16 lanes side by side.  Every element is written exactly once.  No atomics,
// no scratch.  Whole waves reach every phase separator: the pairs behind the last one are clamped to it and their stores predicated.
//
// Bias and gravity are the SAME instructions run twice (a loop the compiler is told not to unroll), the second time with zeros in the
// place of qvel: gravity is bit for bit the bias of the state with qvel = 0.
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

#include "mir_dyn_body.h"

namespace {

struct DynArgs {
  DynTree tree[DYN_MAX_TREE];
  int n_trees, nb_max, nd_max, depth_max;
  int dof0, n_dofs;
  int n_rows, B, qst, vst, nq, nv;
  float gx, gy, gz;
  const long long* env_idx;
  const float *qpos, *qvel, *target;      // the scene's state (storage layout)
  const float *qpos_o, *qvel_o, *qacc_o;  // the caller's rows (public layout), nullable
  JointPtrs m;
  InertiaPtrs mi;
  ControlPtrs mc;
  float *M, *bias, *gravity, *tau, *ctrl;
};
static_assert(sizeof(DynArgs) <= 4096, "kernel arguments");

struct DynLds {
  float xp[G][4], xq[G][4];  // world pose per body
  float ci[G][12];           // spatial inertia per body {m, h, xx yy zz xy xz yz}
  float cd[G][8];            // motion subspace per dof {w, v}
  float cv[G][8], ca[G][8];  // spatial velocity / acceleration per body
  float cf[G][8];            // spatial force per body {t, f}
  float M[G][G];
  int pd[G], sd[G];          // parent dof (local), scene dof
  uint8_t inv[MIR_MAX_DOF];  // scene dof -> local dof, 0xff: another tree's
};

__global__ __launch_bounds__(64) void mir_dyn_kernel(DynArgs a) {
  __shared__ __attribute__((aligned(16))) DynLds lds[4];
  DynLds& L = lds[threadIdx.x >> 4];
  const bool want_mass = a.M || a.tau;
  // ---- what my lane is, poses, spatial inertias, motion subspaces, the M block (shared with mir_osc.hip)
#include "mir_dyn_phases.inc"
  const float* const vrow = a.qvel + (size_t)env * a.vst;
  const float* const vrow_o = a.qvel_o ? a.qvel_o + (size_t)row * a.nv : nullptr;
  // ---- bias forces: recursive Newton-Euler at qacc = 0 with gravity; a second time with qvel = 0 for the gravity forces
  float qd[6] = {0, 0, 0, 0, 0, 0};
  if (isbody && dof1 != DYN_NONE) {
    const int n = jt == MIR_JNT_FREE ? 6 : 1, d0 = L.sd[dof1];
#pragma unroll
    for (int k = 0; k < 6; k++)
      if (k < n) qd[k] = vrow_o ? vrow_o[d0 + k] : vrow[a.m.d_lane[d0 + k]];
  }
  float frc_b = 0.0f, frc_g = 0.0f;
  const int pass0 = (a.bias || a.tau) ? 0 : 1, pass1 = a.gravity ? 1 : 0;
#pragma unroll 1
  for (int pass = pass0; pass <= pass1; pass++) {
    float u[6];
#pragma unroll
    for (int k = 0; k < 6; k++) u[k] = pass ? 0.0f : qd[k];
    Sp cv = {v3(0, 0, 0), v3(0, 0, 0)}, ca = {v3(0, 0, 0), v3(-a.gx, -a.gy, -a.gz)};
    for (int lvl = 0; lvl <= a.depth_max; lvl++) {
      if (isbody && depth == lvl) {
        if (lvl > 0) {
          cv = lds6(L.cv[par]);
          ca = lds6(L.ca[par]);
        }
        if (jt == MIR_JNT_FREE && dof1 != DYN_NONE) {
#pragma unroll
          for (int k = 0; k < 3; k++) axpy6(cv, u[k], lds6(L.cd[dof1 + k]));
          Sp dt[3];
#pragma unroll
          for (int k = 0; k < 3; k++) dt[k] = cross_motion(cv, lds6(L.cd[dof1 + 3 + k]));
#pragma unroll
          for (int k = 0; k < 3; k++) {
            axpy6(ca, u[3 + k], dt[k]);
            axpy6(cv, u[3 + k], lds6(L.cd[dof1 + 3 + k]));
          }
        } else if (jt != MIR_JNT_FIXED && dof1 != DYN_NONE) {
          const Sp s = lds6(L.cd[dof1]);
          axpy6(ca, u[0], cross_motion(cv, s));
          axpy6(cv, u[0], s);
        }
        sts6(L.cv[lane], cv);
        sts6(L.ca[lane], ca);
      }
      WSYNC();
    }
    {
      Sp f = {v3(0, 0, 0), v3(0, 0, 0)};
      if (isbody) {
        const Inert I = ldI(L.ci[lane]);
        Sp Ia, Iv;
        imul(I, ca.a, ca.b, Ia.a, Ia.b);
        imul(I, cv.a, cv.b, Iv.a, Iv.b);
        const Sp x = cross_force(cv, Iv);
        f = Sp{Ia.a + x.a, Ia.b + x.b};
      }
      sts6(L.cf[lane], f);
    }
    WSYNC();
    Sp fs = {v3(0, 0, 0), v3(0, 0, 0)};
    for (int b = 0; b < a.nb_max; b++) {
      if (isdof && (sub >> b & 1)) {
        const Sp f = lds6(L.cf[b]);
        fs.a = fs.a + f.a;
        fs.b = fs.b + f.b;
      }
    }
    const float fr = dot6(S, fs);
    frc_b = pass ? frc_b : fr;
    frc_g = pass ? fr : frc_g;
    WSYNC();  // (the next pass writes cv / ca / cf again)
  }
  WSYNC();  // (the M block is complete)
  // ---- per-dof outputs
  const int nw = a.n_dofs, col = sdof - a.dof0;
  const bool mine = valid && isdof && col >= 0 && col < nw;
  const size_t o = (size_t)row * nw + (mine ? col : 0);
  if (mine) {
    if (a.bias) a.bias[o] = frc_b;
    if (a.gravity) a.gravity[o] = frc_g;
  }
  if (a.tau) {  // inverse dynamics: M_full qacc + bias (the other trees' columns of my row are zeros)
    const float* const arow = a.qacc_o + (size_t)row * a.nv;
    float s = 0.0f;
    for (int j = 0; j < a.nd_max; j++) {
      const float qa = j < nd ? arow[L.sd[j]] : 0.0f;
      s = fmaf(L.M[lane][j], qa, s);
    }
    if (mine) a.tau[o] = frc_b + s;
  }
  if (a.ctrl && mine) {  // the PD torque of orc_smooth: clamp(kp (target - q) - kv qvel, force range), position-controlled dofs only
    const int l = a.m.d_lane[sdof];
    float f = 0.0f;
    if (a.mc.d_ctrl[l] == MIR_CTRL_POSITION) {
      const float v = vrow_o ? vrow_o[sdof] : vrow[l];
      f = a.mc.d_kp[l] * (a.target[(size_t)env * a.vst + l] - qrow[a.mc.d_qadr[sdof]]) - a.mc.d_kv[l] * v;
      f = fmaxf(f, a.mc.d_frclo[l]);
      f = fminf(f, a.mc.d_frchi[l]);
    }
    a.ctrl[o] = f;
  }
  // ---- the rows of the M window that belong to my tree: all n_dofs columns of each, zeros where the column is another tree's
  if (a.M) {
    for (int i = 0; i < a.nd_max; i++) {
      const int r = (i < nd ? L.sd[i] : -1) - a.dof0;
      if (!valid || i >= nd || r < 0 || r >= nw) continue;  // (uniform over the 16 lanes)
      float* const out = a.M + ((size_t)row * nw + r) * nw;
      for (int c = lane; c < nw; c += G) {
        const int t = L.inv[a.dof0 + c];
        out[c] = t != 0xff ? L.M[i][t] : 0.0f;
      }
    }
  }
}

}  // namespace

extern "C" int mir_dyn_query_sizeof(void) { return (int)sizeof(MirDynQuery); }

extern "C" int mir_dynamics(MirHandle h, const MirDynQuery* q, const int64_t* env_idx, int32_t n_rows, const float* qpos, const float* qvel,
                            const float* qacc, float* M, float* bias, float* gravity, float* tau, float* ctrl_force, void* stream) {
  if (!h || !q) return mir_set_error(MIR_E_INVALID, "mir_dynamics: null argument");
  if (q->struct_size != (int32_t)sizeof(MirDynQuery)) return mir_set_error(MIR_E_INVALID, "mir_dynamics: struct_size is not sizeof(MirDynQuery)");
  if (q->flags != 0) return mir_set_error(MIR_E_INVALID, "mir_dynamics: unknown flag bit");
  if (q->dof0 < 0 || q->n_dofs < 0 || q->dof0 > h->nv || q->n_dofs > h->nv - q->dof0)
    return mir_set_error(MIR_E_INVALID, "mir_dynamics: dof window outside [0, nv]");
  if (tau && !qacc) return mir_set_error(MIR_E_INVALID, "mir_dynamics: tau needs qacc");
  if (h->pending) return mir_set_error(MIR_E_INVALID, "mir_dynamics: a step is pending (mir_step_end first)");
  if (env_idx && n_rows < 0) return mir_set_error(MIR_E_INVALID, "mir_dynamics: negative n_rows");
  const int R = env_idx ? n_rows : h->B;
  if ((long long)R * q->n_dofs * q->n_dofs > 0x7fffffffLL) return mir_set_error(MIR_E_CAPACITY, "mir_dynamics: rows x n_dofs^2 reaches 2^31");
  if (R == 0 || q->n_dofs == 0 || (!M && !bias && !gravity && !tau && !ctrl_force)) return MIR_OK;  // (nothing asked for)
  DynArgs a;
  memset(&a, 0, sizeof a);
  DynTrees T;
  if (int rc = dyn_build_trees(h, a.tree, T, "mir_dynamics")) return rc;
  a.n_trees = T.n_trees; a.nb_max = T.nb_max; a.nd_max = T.nd_max; a.depth_max = T.depth_max;
  a.dof0 = q->dof0; a.n_dofs = q->n_dofs;
  a.n_rows = R; a.B = h->B; a.qst = h->pt.qst; a.vst = h->pt.vst; a.nq = h->nq; a.nv = h->nv;
  const ModelView mv(h);
  mv.gravity(a.gx, a.gy, a.gz);
  a.env_idx = reinterpret_cast<const long long*>(env_idx);
  a.qpos = h->qpos; a.qvel = h->qvel; a.target = h->target;
  a.qpos_o = qpos; a.qvel_o = qvel; a.qacc_o = qacc;
  a.m = mv.joint_pointers(); a.mi = mv.inertia_pointers(); a.mc = mv.control_pointers();
  a.M = M; a.bias = bias; a.gravity = gravity; a.tau = tau; a.ctrl = ctrl_force;
  const long long n_pairs = (long long)R * T.n_trees;
  if (n_pairs > 0x7fffffffLL - 4) return mir_set_error(MIR_E_CAPACITY, "mir_dynamics: rows x trees reaches 2^31");
  return launch_rows(h, mir_dyn_kernel, (n_pairs + 3) / 4, stream, a);
}
