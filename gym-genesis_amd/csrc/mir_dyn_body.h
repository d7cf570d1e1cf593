// mir_dyn_body.h — the first phases of mir_dyn.hip (mir_dynamics) as functions: the table of the scene's kinematic trees that travels
// in the kernel arguments, the host code that builds it, and the device code for world poses level by level, spatial inertias about the
// tree origin, motion subspaces and the composite-rigid-body M block in LDS.  The same arithmetic in the same order as mir_dyn.hip,
// statement for statement.  mir_osc.hip (mir_task_dynamics) is built on it.  mir_dyn.hip itself still carries these phases inline:
// calling them from here changed the register allocation and the schedule of mir_dyn_kernel (the arithmetic stayed), and that kernel's
// code object was to stay the parent's, so it was left alone (profiles/task_dynamics/README.md).  A change to either copy belongs in both.
// The functions are templates over the kernel's argument and LDS structs and use the fields named in their comments.
// Included after mir_dev.h with G = 16, inside no namespace.
#pragma once
#include <stdio.h>

namespace {

constexpr int DYN_MAX_TREE = 20;  // trees with dofs in one scene (the kernel arguments are 4 KB)
constexpr int DYN_NONE = 15;      // "no dof" in a 4-bit field (a tree has at most 15 dofs)

struct DynTree {
  uint32_t body[G];  // body | jtype << 8 | local parent << 10 | depth << 14 | first local dof << 18 (DYN_NONE: none)
  uint32_t dof[G];   // scene dof | local body << 8 | local parent dof << 12 (DYN_NONE: none) | free-joint component 0..5 << 16
  uint16_t sub[G];   // local bodies in the subtree of local body j, j included
  uint8_t nb, nd, pad[2];
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

// ---- device: what a lane is in its (row, tree) pair.  Args needs tree[], n_rows, n_trees, B, env_idx.
struct DynLane {
  int lane, row, ti, env, nb, nd;
  bool valid, isbody, isdof;
  int body, jt, par, depth, dof1;  // lane as BODY lane of the tree
  int sdof, dbody, pdof;           // lane as DOF lane of the tree
};
template <class Args>
__device__ __forceinline__ DynLane dyn_lane(const Args& a) {
  DynLane t;
  const int tid = threadIdx.x, grp = tid >> 4;
  t.lane = tid & 15;
  const int n_pairs = a.n_rows * a.n_trees;
  const int pair_raw = blockIdx.x * 4 + grp;
  t.valid = pair_raw < n_pairs;
  const int pair = t.valid ? pair_raw : n_pairs - 1;
  t.row = pair / a.n_trees;
  t.ti = pair - t.row * a.n_trees;
  int env = a.env_idx ? (int)a.env_idx[t.row] : t.row;
  t.env = env < 0 ? 0 : (env >= a.B ? a.B - 1 : env);  // (an index outside the batch is clamped, not followed)
  t.nb = a.tree[t.ti].nb;
  t.nd = a.tree[t.ti].nd;
  t.isbody = t.lane < t.nb;
  t.isdof = t.lane < t.nd;
  const uint32_t bw = t.isbody ? a.tree[t.ti].body[t.lane] : 0u;
  const uint32_t dw = t.isdof ? a.tree[t.ti].dof[t.lane] : 0u;
  t.body = bw & 0xff; t.jt = (bw >> 8) & 3; t.par = (bw >> 10) & 15; t.depth = (bw >> 14) & 15;
  t.dof1 = t.isbody ? (int)((bw >> 18) & 15) : DYN_NONE;
  t.sdof = dw & 0xff; t.dbody = (dw >> 8) & 15;
  t.pdof = t.isdof ? (int)((dw >> 12) & 15) : DYN_NONE;
  return t;
}

// ---- device: tables of the tree every lane can reach, an empty M block; the local transform of my body (as mir_kin.hip); world poses,
// one level of the tree at a time (a free body's pose is its qpos row, as in orc_fk).  Lds needs pd, sd, inv, M, xp, xq.
template <class Args, class Lds>
__device__ __forceinline__ void dyn_poses(const Args& a, Lds& L, const DynLane& t, const float* qrow, V3& P, Q4& Qx, V3& baxis) {
  const int lane = t.lane, body = t.body, jt = t.jt;
  L.pd[lane] = t.pdof;
  L.sd[lane] = t.sdof;
  for (int i = lane; i < MIR_MAX_DOF; i += G) L.inv[i] = 0xff;
#pragma unroll
  for (int j = 0; j < G; j++) L.M[lane][j] = 0.0f;
  WSYNC();
  if (t.isdof) L.inv[t.sdof] = (uint8_t)lane;
  P = v3(0, 0, 0); baxis = v3(0, 0, 0);
  Qx = Q4{1, 0, 0, 0};
  if (t.isbody) {
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
  for (int lvl = 0; lvl <= a.depth_max; lvl++) {
    if (t.isbody && t.depth == lvl) {
      if (lvl > 0 && jt != MIR_JNT_FREE) {
        const V3 pp = ld3(L.xp[t.par]);
        const Q4 pq = ld4(L.xq[t.par]);
        P = pp + qrot(pq, P);
        Qx = qmul(pq, Qx);
      }
      st3(L.xp[lane], P);
      st4(L.xq[lane], Qx);
    }
    WSYNC();
  }
}

// ---- device: spatial inertia about the tree origin (the root body's origin), world axes, into ci; motion subspaces of my body's dofs
// into cd.  Ends with the phase separator.
template <class Args, class Lds>
__device__ __forceinline__ void dyn_inertia(const Args& a, Lds& L, const DynLane& t, V3 P, Q4 Qx, V3 baxis) {
  const int lane = t.lane, body = t.body, jt = t.jt, dof1 = t.dof1;
  const V3 cref = ld3(L.xp[0]);
  {
    float c[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (t.isbody) {
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
}

// ---- device: mass matrix: composite inertia of my dof's body (the sum over its subtree's bodies, ascending), M[i][j] up dof_parent,
// armature on the diagonal; both triangles of the tree's block in LDS, by lane i alone.  No separator after it.
template <class Args, class Lds>
__device__ __forceinline__ void dyn_mass(const Args& a, Lds& L, const DynLane& t, const Sp& S, int sub) {
  const int lane = t.lane;
  float c[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int b = 0; b < a.nb_max; b++) {
    if (t.isdof && (sub >> b & 1)) {
#pragma unroll
      for (int k = 0; k < 10; k++) c[k] += L.ci[b][k];
    }
  }
  if (t.isdof) {
    const Inert I = {c[0], {c[1], c[2], c[3]}, c[4], c[5], c[6], c[7], c[8], c[9]};
    Sp f;
    imul(I, S.a, S.b, f.a, f.b);
    const float arm = a.d_armature[a.d_lane[t.sdof]];
    for (int j = lane; j != DYN_NONE; j = L.pd[j]) {
      float v = dot6(lds6(L.cd[j]), f);
      if (j == lane) v += arm;
      L.M[lane][j] = v;
      L.M[j][lane] = v;
    }
  }
}

// ---- host: the scene's kinematic trees with dofs, bodies and dofs in body order (the dof order of the spec)
struct DynTrees {
  int n_trees, nb_max, nd_max, depth_max;
  int tree_of[MIR_MAX_BODY];  // per scene body: its tree in tree[] (-1: the world, or a tree welded to it), and its local index there
  int local[MIR_MAX_BODY];
};

static int dyn_error(int code, const char* who, const char* what) {
  char msg[256];
  snprintf(msg, sizeof msg, "%s: %s", who, what);
  return mir_set_error(code, msg);
}

static int dyn_build_trees(MirHandle h, DynTree* tree, DynTrees& T, const char* who) {
  const bool k16 = h->kernel == 16;
  auto parent = [&](int b) { return k16 ? h->hm.b_parent[b] : h->hm64.b_parent[b]; };
  auto jtype = [&](int b) { return k16 ? h->hm.b_jtype[b] : h->hm64.b_jtype[b]; };
  auto ndof = [&](int b) { const int jt = jtype(b); return jt == MIR_JNT_FREE ? 6 : (jt == MIR_JNT_FIXED ? 0 : 1); };
  int dofadr[MIR_MAX_BODY], root[MIR_MAX_BODY], ldof[MIR_MAX_BODY];
  int* const local = T.local;
  T.n_trees = T.nb_max = T.nd_max = T.depth_max = 0;
  int nv = 0;
  for (int b = 0; b < h->nbody; b++) {
    dofadr[b] = nv;
    nv += b ? ndof(b) : 0;
    root[b] = (b == 0 || parent(b) == 0) ? b : root[parent(b)];
    T.tree_of[b] = -1;
    local[b] = 0;
  }
  if (nv != h->nv) return dyn_error(MIR_E_INVALID, who, "the model's joints do not add up to nv");
  int nt = 0;
  for (int r = 1; r < h->nbody; r++) {
    if (root[r] != r) continue;
    int dofs = 0, bodies = 0;
    for (int b = r; b < h->nbody; b++)
      if (root[b] == r) { dofs += ndof(b); bodies++; }
    if (!dofs) continue;  // (a tree welded to the world)
    if (bodies > G || dofs > DYN_NONE) return dyn_error(MIR_E_CAPACITY, who, "a kinematic tree of more than 16 bodies or 15 dofs");
    if (nt >= DYN_MAX_TREE) return dyn_error(MIR_E_CAPACITY, who, "more than 20 kinematic trees");
    DynTree& t = tree[nt];
    int nbq = 0, ndq = 0;
    for (int b = r; b < h->nbody; b++) {
      if (root[b] != r) continue;
      const int j = nbq++, p = b == r ? 0 : local[parent(b)];
      const int depth = b == r ? 0 : (int)((t.body[p] >> 14) & 15) + 1;
      const int n = ndof(b);
      // (a free body's pose is its qpos row whatever is above it, as in orc_fk: below another body its velocity would mix two conventions)
      if (jtype(b) == MIR_JNT_FREE && b != r) return dyn_error(MIR_E_INVALID, who, "a free joint below another body");
      local[b] = j;
      T.tree_of[b] = nt;
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
      if (depth > T.depth_max) T.depth_max = depth;
    }
    t.nb = (uint8_t)nbq; t.nd = (uint8_t)ndq;
    if (nbq > T.nb_max) T.nb_max = nbq;
    if (ndq > T.nd_max) T.nd_max = ndq;
    nt++;
  }
  if (!nt) return dyn_error(MIR_E_INVALID, who, "the scene has no dofs");
  T.n_trees = nt;
  return MIR_OK;
}

// the addresses of the per-body / per-dof constants of the device model (DevModel or DevModel64: same shapes); Args has the fields
template <class Args>
static void dyn_model_pointers(MirHandle h, Args& a) {
  const bool k16 = h->kernel == 16;
  const char* const dm = k16 ? reinterpret_cast<const char*>(h->dm) : reinterpret_cast<const char*>(h->dm64);
#define DYN_F(name) reinterpret_cast<const float*>(dm + (k16 ? offsetof(DevModel, name) : offsetof(DevModel64, name)))
#define DYN_I(name) reinterpret_cast<const int32_t*>(dm + (k16 ? offsetof(DevModel, name) : offsetof(DevModel64, name)))
  a.b_pos = DYN_F(b_pos); a.b_quat = DYN_F(b_quat); a.b_axis = DYN_F(b_axis); a.b_ipos = DYN_F(b_ipos);
  a.b_inertia = DYN_F(b_inertia); a.b_mass = DYN_F(b_mass); a.b_qadr = DYN_I(b_qadr);
  a.d_armature = DYN_F(d_armature);
#undef DYN_F
#undef DYN_I
  a.d_lane = reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(h->dpt) + offsetof(PlumbTab, d_lane));
}

}  // namespace
