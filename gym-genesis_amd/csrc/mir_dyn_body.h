// mir_dyn_body.h — what mir_dyn.hip (mir_dynamics) and mir_osc.hip (mir_task_dynamics) have in common beside the device phases of
// mir_dyn_phases.inc: the table of the scene's kinematic trees that travels in the kernel arguments, the host code that builds it, and
// the spatial-vector helpers of the device code.  Included after mir_query.h (mir_dev.h with G = 16), inside no namespace.
#pragma once

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

// ---- host: the scene's kinematic trees with dofs, bodies and dofs in body order (the dof order of the spec)
struct DynTrees {
  int n_trees, nb_max, nd_max, depth_max;
  int tree_of[MIR_MAX_BODY];  // per scene body: its tree in tree[] (-1: the world, or a tree welded to it), and its local index there
  int local[MIR_MAX_BODY];
};

static int dyn_build_trees(MirHandle h, DynTree* tree, DynTrees& T, const char* who) {
  const ModelView mv(h);
  int dofadr[MIR_MAX_BODY], root[MIR_MAX_BODY], ldof[MIR_MAX_BODY];
  int* const local = T.local;
  T.n_trees = T.nb_max = T.nd_max = T.depth_max = 0;
  int nv = 0;
  for (int b = 0; b < h->nbody; b++) {
    dofadr[b] = nv;
    nv += b ? mv.ndof(b) : 0;
    root[b] = (b == 0 || mv.parent(b) == 0) ? b : root[mv.parent(b)];
    T.tree_of[b] = -1;
    local[b] = 0;
  }
  if (nv != h->nv) return query_error(MIR_E_INVALID, who, "the model's joints do not add up to nv");
  int nt = 0;
  for (int r = 1; r < h->nbody; r++) {
    if (root[r] != r) continue;
    int dofs = 0, bodies = 0;
    for (int b = r; b < h->nbody; b++)
      if (root[b] == r) { dofs += mv.ndof(b); bodies++; }
    if (!dofs) continue;  // (a tree welded to the world)
    if (bodies > G || dofs > DYN_NONE) return query_error(MIR_E_CAPACITY, who, "a kinematic tree of more than 16 bodies or 15 dofs");
    if (nt >= DYN_MAX_TREE) return query_error(MIR_E_CAPACITY, who, "more than 20 kinematic trees");
    DynTree& t = tree[nt];
    int nbq = 0, ndq = 0;
    for (int b = r; b < h->nbody; b++) {
      if (root[b] != r) continue;
      const int j = nbq++, p = b == r ? 0 : local[mv.parent(b)];
      const int depth = b == r ? 0 : (int)((t.body[p] >> 14) & 15) + 1;
      const int n = mv.ndof(b);
      // (a free body's pose is its qpos row whatever is above it, as in orc_fk: below another body its velocity would mix two conventions)
      if (mv.jtype(b) == MIR_JNT_FREE && b != r) return query_error(MIR_E_INVALID, who, "a free joint below another body");
      local[b] = j;
      T.tree_of[b] = nt;
      int pd = DYN_NONE;  // the last dof of the nearest ancestor that has one
      for (int c = b == r ? 0 : mv.parent(b); c > 0; c = mv.parent(c))
        if (mv.ndof(c)) { pd = ldof[c] + mv.ndof(c) - 1; break; }
      ldof[b] = n ? ndq : DYN_NONE;
      t.body[j] = (uint32_t)b | (uint32_t)mv.jtype(b) << 8 | (uint32_t)p << 10 | (uint32_t)depth << 14 | (uint32_t)ldof[b] << 18;
      for (int k = 0; k < n; k++, ndq++)
        t.dof[ndq] = (uint32_t)(dofadr[b] + k) | (uint32_t)j << 8 | (uint32_t)(k ? ndq - 1 : pd) << 12 | (uint32_t)k << 16;
      for (int c = b;; c = mv.parent(c)) {  // b is in the subtree of each of its ancestors and its own
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
  if (!nt) return query_error(MIR_E_INVALID, who, "the scene has no dofs");
  T.n_trees = nt;
  return MIR_OK;
}

}  // namespace
