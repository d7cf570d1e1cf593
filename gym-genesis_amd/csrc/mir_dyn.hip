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

namespace {

constexpr int DYN_MAX_TREE = 20;  // trees with dofs in one scene (the kernel arguments are 4 KB)
constexpr int DYN_NONE = 15;      // "no dof" in a 4-bit field (a tree has at most 15 dofs)

struct DynTree {
  uint32_t body[G];  // body | jtype << 8 | local parent << 10 | depth << 14 | first local dof << 18 (DYN_NONE: none)
  uint32_t dof[G];   // scene dof | local body << 8 | local parent dof << 12 (DYN_NONE: none) | free-joint component 0..5 << 16
  uint16_t sub[G];   // local bodies in the subtree of local body j, j included
  uint8_t nb, nd, pad[2];
};

struct DynArgs {
  DynTree tree[DYN_MAX_TREE];
  int n_trees, nb_max, nd_max, depth_max;
  int dof0, n_dofs;
  int n_rows, B, qst, vst, nq, nv;
  float gx, gy, gz;
  const long long* env_idx;
  const float *qpos, *qvel, *target;      // the scene's state (storage layout)
  const float *qpos_o, *qvel_o, *qacc_o;  // the caller's rows (public layout), nullable
  // per-body constants of the device model (DevModel or DevModel64: same shapes)
  const float *b_pos, *b_quat, *b_axis, *b_ipos, *b_inertia, *b_mass;
  const int32_t* b_qadr;
  // per-dof constants, indexed by the dof's lane (PlumbTab::d_lane)
  const float *d_armature, *d_kp, *d_kv, *d_frclo, *d_frchi;
  const int32_t *d_ctrl, *d_lane, *d_qadr;
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

struct Sp {  // spatial motion {w, v} or force {t, f}
  V3 a, b;
};
__device__ __forceinline__ Sp lds6(const float* p) { return {ld3(p), ld3(p + 3)}; }
__device__ __forceinline__ void sts6(float* p, const Sp& s) { st3(p, s.a); st3(p + 3, s.b); }
__device__ __forceinline__ Sp cross_motion(const Sp& x, const Sp& y) { return {cross(x.a, y.a), cross(x.a, y.b) + cross(x.b, y.a)}; }
__device__ __forceinline__ Sp cross_force(const Sp& x, const Sp& f) { return {cross(x.a, f.a) + cross(x.b, f.b), cross(x.a, f.b)}; }
__device__ __forceinline__ float dot6(const Sp& x, const Sp& y) { return dot(x.a, y.a) + dot(x.b, y.b); }
__device__ __forceinline__ void axpy6(Sp& y, float s, const Sp& x) { y.a = y.a + s * x.a; y.b = y.b + s * x.b; }

__global__ __launch_bounds__(64) void mir_dyn_kernel(DynArgs a) {
  __shared__ __attribute__((aligned(16))) DynLds lds[4];
  const int tid = threadIdx.x, lane = tid & 15, grp = tid >> 4;
  DynLds& L = lds[grp];
  const int n_pairs = a.n_rows * a.n_trees;
  const int pair_raw = blockIdx.x * 4 + grp;
  const bool valid = pair_raw < n_pairs;
  const int pair = valid ? pair_raw : n_pairs - 1;
  const int row = pair / a.n_trees, ti = pair - row * a.n_trees;
  int env = a.env_idx ? (int)a.env_idx[row] : row;
  env = env < 0 ? 0 : (env >= a.B ? a.B - 1 : env);  // (an index outside the batch is clamped, not followed)
  const int nb = a.tree[ti].nb, nd = a.tree[ti].nd;
  const bool isbody = lane < nb, isdof = lane < nd;
  const uint32_t bw = isbody ? a.tree[ti].body[lane] : 0u;
  const uint32_t dw = isdof ? a.tree[ti].dof[lane] : 0u;
  const int body = bw & 0xff, jt = (bw >> 8) & 3, par = (bw >> 10) & 15, depth = (bw >> 14) & 15, dof1 = isbody ? (int)((bw >> 18) & 15) : DYN_NONE;
  const int sdof = dw & 0xff, dbody = (dw >> 8) & 15, pdof = isdof ? (int)((dw >> 12) & 15) : DYN_NONE;
  const float* const qrow = a.qpos_o ? a.qpos_o + (size_t)row * a.nq : a.qpos + (size_t)env * a.qst;
  const float* const vrow = a.qvel + (size_t)env * a.vst;
  const float* const vrow_o = a.qvel_o ? a.qvel_o + (size_t)row * a.nv : nullptr;
  // ---- tables of the tree every lane can reach, an empty M block
  L.pd[lane] = pdof;
  L.sd[lane] = sdof;
  for (int i = lane; i < MIR_MAX_DOF; i += G) L.inv[i] = 0xff;
#pragma unroll
  for (int j = 0; j < G; j++) L.M[lane][j] = 0.0f;
  WSYNC();
  if (isdof) L.inv[sdof] = (uint8_t)lane;
  // ---- local transform of my body (as mir_kin.hip)
  V3 P = v3(0, 0, 0), baxis = v3(0, 0, 0);
  Q4 Qx = Q4{1, 0, 0, 0};
  if (isbody) {
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
  // ---- world poses, one level of the tree at a time (a free body's pose is its qpos row, as in orc_fk)
  for (int lvl = 0; lvl <= a.depth_max; lvl++) {
    if (isbody && depth == lvl) {
      if (lvl > 0 && jt != MIR_JNT_FREE) {
        const V3 pp = ld3(L.xp[par]);
        const Q4 pq = ld4(L.xq[par]);
        P = pp + qrot(pq, P);
        Qx = qmul(pq, Qx);
      }
      st3(L.xp[lane], P);
      st4(L.xq[lane], Qx);
    }
    WSYNC();
  }
  // ---- spatial inertia about the tree origin (the root body's origin), world axes; motion subspaces of my body's dofs
  const V3 cref = ld3(L.xp[0]);
  {
    float c[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (isbody) {
      const M3 R = q2m(Qx);
      const float* const ib = a.b_inertia + body * 6;
      const V3 i0 = v3(ib[0], ib[3], ib[4]), i1 = v3(ib[3], ib[1], ib[5]), i2 = v3(ib[4], ib[5], ib[2]);
      const V3 t0 = R.r0.x * i0 + R.r0.y * i1 + R.r0.z * i2;
      const V3 t1 = R.r1.x * i0 + R.r1.y * i1 + R.r1.z * i2;
      const V3 t2 = R.r2.x * i0 + R.r2.y * i1 + R.r2.z * i2;
      const V3 r = P + mmul(R, ld3(a.b_ipos + body * 3)) - cref;
      const float ms = a.b_mass[body], rr = dot(r, r);
      c[0] = ms; c[1] = ms * r.x; c[2] = ms * r.y; c[3] = ms * r.z;
      c[4] = dot(t0, R.r0) + ms * (rr - r.x * r.x);
      c[5] = dot(t1, R.r1) + ms * (rr - r.y * r.y);
      c[6] = dot(t2, R.r2) + ms * (rr - r.z * r.z);
      c[7] = dot(t0, R.r1) - ms * r.x * r.y;
      c[8] = dot(t0, R.r2) - ms * r.x * r.z;
      c[9] = dot(t1, R.r2) - ms * r.y * r.z;
      const V3 rc = cref - P;
      if (jt == MIR_JNT_REVOLUTE || jt == MIR_JNT_PRISMATIC) {
        const V3 axw = mmul(R, baxis);
        const Sp s = jt == MIR_JNT_REVOLUTE ? Sp{axw, cross(axw, rc)} : Sp{v3(0, 0, 0), axw};
        if (dof1 != DYN_NONE) sts6(L.cd[dof1], s);
      } else if (jt == MIR_JNT_FREE && dof1 != DYN_NONE) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
          const V3 ek = v3(k == 0 ? 1.0f : 0.0f, k == 1 ? 1.0f : 0.0f, k == 2 ? 1.0f : 0.0f);
          sts6(L.cd[dof1 + k], Sp{v3(0, 0, 0), ek});
          sts6(L.cd[dof1 + 3 + k], Sp{ek, cross(ek, rc)});
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 10; k++) L.ci[lane][k] = c[k];
  }
  WSYNC();
  const Sp S = isdof ? lds6(L.cd[lane]) : Sp{v3(0, 0, 0), v3(0, 0, 0)};
  const int sub = a.tree[ti].sub[isdof ? dbody : 0];
  // ---- mass matrix: composite inertia of my dof's body, M[i][j] up dof_parent, armature on the diagonal
  if (a.M || a.tau) {
    float c[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int b = 0; b < a.nb_max; b++) {
      if (isdof && (sub >> b & 1)) {
#pragma unroll
        for (int k = 0; k < 10; k++) c[k] += L.ci[b][k];
      }
    }
    if (isdof) {
      const Inert I = {c[0], {c[1], c[2], c[3]}, c[4], c[5], c[6], c[7], c[8], c[9]};
      Sp f;
      imul(I, S.a, S.b, f.a, f.b);
      const float arm = a.d_armature[a.d_lane[sdof]];
      for (int j = lane; j != DYN_NONE; j = L.pd[j]) {
        float v = dot6(lds6(L.cd[j]), f);
        if (j == lane) v += arm;
        L.M[lane][j] = v;
        L.M[j][lane] = v;
      }
    }
  }
  // ---- bias forces: recursive Newton-Euler at qacc = 0 with gravity; a second time with qvel = 0 for the gravity forces
  float qd[6] = {0, 0, 0, 0, 0, 0};
  if (isbody && dof1 != DYN_NONE) {
    const int n = jt == MIR_JNT_FREE ? 6 : 1, d0 = L.sd[dof1];
#pragma unroll
    for (int k = 0; k < 6; k++)
      if (k < n) qd[k] = vrow_o ? vrow_o[d0 + k] : vrow[a.d_lane[d0 + k]];
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
    const int l = a.d_lane[sdof];
    float f = 0.0f;
    if (a.d_ctrl[l] == MIR_CTRL_POSITION) {
      const float v = vrow_o ? vrow_o[sdof] : vrow[l];
      f = a.d_kp[l] * (a.target[(size_t)env * a.vst + l] - qrow[a.d_qadr[sdof]]) - a.d_kv[l] * v;
      f = fmaxf(f, a.d_frclo[l]);
      f = fminf(f, a.d_frchi[l]);
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
  // ---- the scene's kinematic trees with dofs, bodies and dofs in body order (the dof order of the spec)
  DynArgs a;
  memset(&a, 0, sizeof a);
  const bool k16 = h->kernel == 16;
  auto parent = [&](int b) { return k16 ? h->hm.b_parent[b] : h->hm64.b_parent[b]; };
  auto jtype = [&](int b) { return k16 ? h->hm.b_jtype[b] : h->hm64.b_jtype[b]; };
  auto ndof = [&](int b) { const int jt = jtype(b); return jt == MIR_JNT_FREE ? 6 : (jt == MIR_JNT_FIXED ? 0 : 1); };
  int dofadr[MIR_MAX_BODY], root[MIR_MAX_BODY], local[MIR_MAX_BODY], ldof[MIR_MAX_BODY];
  int nv = 0;
  for (int b = 0; b < h->nbody; b++) {
    dofadr[b] = nv;
    nv += b ? ndof(b) : 0;
    root[b] = (b == 0 || parent(b) == 0) ? b : root[parent(b)];
  }
  if (nv != h->nv) return mir_set_error(MIR_E_INVALID, "mir_dynamics: the model's joints do not add up to nv");
  int nt = 0;
  for (int r = 1; r < h->nbody; r++) {
    if (root[r] != r) continue;
    int dofs = 0, bodies = 0;
    for (int b = r; b < h->nbody; b++)
      if (root[b] == r) { dofs += ndof(b); bodies++; }
    if (!dofs) continue;  // (a tree welded to the world)
    if (bodies > G || dofs > DYN_NONE) return mir_set_error(MIR_E_CAPACITY, "mir_dynamics: a kinematic tree of more than 16 bodies or 15 dofs");
    if (nt >= DYN_MAX_TREE) return mir_set_error(MIR_E_CAPACITY, "mir_dynamics: more than 20 kinematic trees");
    DynTree& t = a.tree[nt];
    int nbq = 0, ndq = 0;
    for (int b = r; b < h->nbody; b++) {
      if (root[b] != r) continue;
      const int j = nbq++, p = b == r ? 0 : local[parent(b)];
      const int depth = b == r ? 0 : (int)((t.body[p] >> 14) & 15) + 1;
      const int n = ndof(b);
      // (a free body's pose is its qpos row whatever is above it, as in orc_fk: below another body its velocity would mix two conventions)
      if (jtype(b) == MIR_JNT_FREE && b != r) return mir_set_error(MIR_E_INVALID, "mir_dynamics: a free joint below another body");
      local[b] = j;
      int pd = DYN_NONE;  // the last dof of the nearest ancestor that has one
      for (int c = b == r ? 0 : parent(b); c > 0; c = parent(c))
        if (ndof(c)) { pd = ldof[c] + ndof(c) - 1; break; }
      ldof[b] = n ? ndq : DYN_NONE;
      t.body[j] = (uint32_t)b | (uint32_t)jtype(b) << 8 | (uint32_t)p << 10 | (uint32_t)depth << 14 | (uint32_t)ldof[b] << 18;
      for (int k = 0; k < n; k++, ndq++)
        t.dof[ndq] = (uint32_t)(dofadr[b] + k) | (uint32_t)j << 8 | (uint32_t)(k ? ndq - 1 : pd) << 12 | (uint32_t)k << 16;
      for (int c = b;; c = parent(c)) {  // b is in the subtree of each of its ancestors and its own
        t.sub[local[c]] |= (uint16_t)(1u << j);
        if (c == r) break;
      }
      if (depth > a.depth_max) a.depth_max = depth;
    }
    t.nb = (uint8_t)nbq; t.nd = (uint8_t)ndq;
    if (nbq > a.nb_max) a.nb_max = nbq;
    if (ndq > a.nd_max) a.nd_max = ndq;
    nt++;
  }
  if (!nt) return mir_set_error(MIR_E_INVALID, "mir_dynamics: the scene has no dofs");
  a.n_trees = nt;
  a.dof0 = q->dof0; a.n_dofs = q->n_dofs;
  a.n_rows = R; a.B = h->B; a.qst = h->pt.qst; a.vst = h->pt.vst; a.nq = h->nq; a.nv = h->nv;
  a.gx = k16 ? h->hm.gx : h->hm64.gx; a.gy = k16 ? h->hm.gy : h->hm64.gy; a.gz = k16 ? h->hm.gz : h->hm64.gz;
  a.env_idx = reinterpret_cast<const long long*>(env_idx);
  a.qpos = h->qpos; a.qvel = h->qvel; a.target = h->target;
  a.qpos_o = qpos; a.qvel_o = qvel; a.qacc_o = qacc;
  const char* const dm = k16 ? reinterpret_cast<const char*>(h->dm) : reinterpret_cast<const char*>(h->dm64);
#define DYN_F(name) reinterpret_cast<const float*>(dm + (k16 ? offsetof(DevModel, name) : offsetof(DevModel64, name)))
#define DYN_I(name) reinterpret_cast<const int32_t*>(dm + (k16 ? offsetof(DevModel, name) : offsetof(DevModel64, name)))
  a.b_pos = DYN_F(b_pos); a.b_quat = DYN_F(b_quat); a.b_axis = DYN_F(b_axis); a.b_ipos = DYN_F(b_ipos);
  a.b_inertia = DYN_F(b_inertia); a.b_mass = DYN_F(b_mass); a.b_qadr = DYN_I(b_qadr);
  a.d_armature = DYN_F(d_armature); a.d_kp = DYN_F(d_kp); a.d_kv = DYN_F(d_kv); a.d_frclo = DYN_F(d_frclo); a.d_frchi = DYN_F(d_frchi);
  a.d_ctrl = DYN_I(d_ctrl);
#undef DYN_F
#undef DYN_I
  a.d_lane = reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(h->dpt) + offsetof(PlumbTab, d_lane));
  a.d_qadr = reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(h->dpt) + offsetof(PlumbTab, d_qadr));
  a.M = M; a.bias = bias; a.gravity = gravity; a.tau = tau; a.ctrl = ctrl_force;
  const long long n_pairs = (long long)R * nt;
  if (n_pairs > 0x7fffffffLL - 4) return mir_set_error(MIR_E_CAPACITY, "mir_dynamics: rows x trees reaches 2^31");
  int prev = -1;
  (void)hipGetDevice(&prev);
  if (prev != h->device) (void)hipSetDevice(h->device);
  hipLaunchKernelGGL(mir_dyn_kernel, dim3((unsigned)((n_pairs + 3) / 4)), dim3(64), 0, (hipStream_t)stream, a);
  hipError_t e = hipGetLastError();
  if (prev != h->device && prev >= 0) (void)hipSetDevice(prev);
  if (e != hipSuccess) return mir_set_error(MIR_E_HIP, hipGetErrorString(e));
  return MIR_OK;
}
