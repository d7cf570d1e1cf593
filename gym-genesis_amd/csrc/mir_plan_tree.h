// mir_plan_tree.h — the tree loop of the planner with the goal tree started as a forest, for mir_goal.hip (mir_plan_path_goals: a set of
// goals): the two trees in dynamic LDS with node / add / nearest, and plan_grow_and_store(): RRT-Connect from the
// tree set-up to the meeting, the extraction of the polyline, the shortcut smoothing, the resampling and every store of a row.  Tb
// starts as a FOREST of `nroots` roots, each with PLAN_NO_PARENT: nodes 0 .. nroots - 1.  With one root this is the loop of
// mir_plan_kernel (mir_plan.hip), statement for statement: the set-up adds the same node 0, `nearest` walks the same nodes in the same
// order, and the parent walk ends at the only root; tests/test_gpu_goal.py pins the bytes.  The arithmetic and its order are those of
// include/mirigid.h, "motion planning".
// mir_plan.hip still holds its own text of this loop (the random numbers, plan_u, are shared through mir_plan_row.h).  Calling this header from mir_plan_kernel with one root gave the same bytes on
// every planner case but cost its four instantiations 7 VGPRs each and 3 % of a detour's time ("Goal sets"), so that fold
// waits until it is free.
// Needs mir_plan_row.h in front of it.  Inside no namespace.
#pragma once

namespace {

// the two trees of a row at the head of dynamic LDS: coordinates [tree][dof][node], then a 16-bit parent [tree][node]
struct PlanTrees {
  PlanLds& L;
  float* tree;
  uint16_t* parent;
  int lane, D, MN, dj;
  bool isd;

  __device__ __forceinline__ PlanTrees(PlanLds& lds, float* dyn, int lane_, int D_, int MN_)
      : L(lds), tree(dyn), parent(reinterpret_cast<uint16_t*>(dyn + (size_t)2 * D_ * MN_)), lane(lane_), D(D_), MN(MN_), dj(lane_ < D_ ? lane_ : 0),
        isd(lane_ < D_) {}
  // the floats of dynamic LDS the trees take (2 MN 16-bit parents are MN floats): what follows them starts here
  __device__ __forceinline__ static size_t floats(int D_, int MN_) { return (size_t)(2 * D_ + 1) * MN_; }

  __device__ __forceinline__ float node(int t, int n) const { return isd ? tree[((size_t)t * D + dj) * MN + n] : 0.0f; }
  __device__ __forceinline__ void add(int t, int n, float v, int par) {
    if (isd) tree[((size_t)t * D + dj) * MN + n] = v;
    if (lane == 0) parent[t * MN + n] = (uint16_t)par;
    WSYNC();
  }
  // nearest node of tree t (cnt nodes) to q: squared L2 distance over the planned dofs, j ascending; the lower index wins a tie
  __device__ __forceinline__ int nearest(int t, int cnt, float q, float& d2) {
    if (isd) L.qs[lane] = q;
    WSYNC();
    float bd = INFINITY;
    int bi = 0x7fffffff;
    for (int n = lane; n < cnt; n += 64) {
      float acc = 0.0f;
      for (int j = 0; j < D; j++) {
        const float e = tree[((size_t)t * D + j) * MN + n] - L.qs[j];
        acc = acc + e * e;
      }
      if (acc < bd) { bd = acc; bi = n; }  // (nodes ascend: the lower index keeps a tie)
    }
    const ArgMin m = wave_argmin(bd, bi);
    WSYNC();
    d2 = m.v;
    bi = __builtin_amdgcn_readfirstlane(m.i);
    return bi < cnt ? bi : 0;
  }
};

// What a row has decided before its trees: `status` (MIR_PLAN_OK: a plan is still possible); `npoly` (2: the direct edge held and
// L.poly[0 .. 1] is the polyline; 1 with MIR_PLAN_OK: the trees have to be grown).  plan_grow_and_store() does the rest of the row:
// grows the trees when they are needed (Ta = {sv}; Tb = the forest its caller has already written: nodes 0 .. nroots - 1 of tree 1,
// each added with PLAN_NO_PARENT), extracts,
// smooths, resamples and stores path, poly, n_poly, status and stats.  Returns the index of the root the polyline ends at when the
// trees met, else -1.
template <class Row>
__device__ __forceinline__ int plan_grow_and_store(Row& r, PlanTrees& T, int row, int env, float sv, float lo, float hi, int status, int npoly,
                                                   int nroots) {
  const PlanArgs& a = r.a;
  PlanLds& L = r.L;
  const int lane = r.lane, D = a.D, MN = a.max_nodes, dj = T.dj;
  const bool isd = T.isd;
  uint16_t* const parent = T.parent;
  int iterations = 0, na = 1, nb = 1, reached = -1;
  if (status == MIR_PLAN_OK && npoly == 1) {
    T.add(0, 0, sv, PLAN_NO_PARENT);
    nb = nroots;
    status = MIR_PLAN_ITERATION_LIMIT;
    for (int it = 0; it < a.max_iter; it++) {
      iterations = it + 1;
      const int t = it & 1, o = t ^ 1;
      int ct = t ? nb : na, co = t ? na : nb;
      const float qr = isd ? lo + plan_u(a.seed, (uint32_t)env, (uint32_t)it, (uint32_t)dj) * (hi - lo) : 0.0f;
      float d2;
      const int near = T.nearest(t, ct, qr, d2);
      const float nv = T.node(t, near);
      const float qn = nv + fminf(1.0f, a.step / sqrtf(d2)) * (qr - nv);
      if (!r.edge(nv, qn)) continue;
      if (ct >= MN) { status = MIR_PLAN_NODE_LIMIT; break; }
      T.add(t, ct, qn, near);
      const int inew = ct++;
      // connect: from the other tree's nearest node towards q_new, at most `step` at a time
      int ci = T.nearest(o, co, qn, d2);
      float cv = T.node(o, ci);
      bool met = false, full = false;
      for (int k = 0; k < MN; k++) {  // (every pass adds a node or leaves)
        const float diff = qn - cv;
        const float d = sqrtf(r.norm2(diff));
        const bool last = d <= a.step;
        const float tv = last ? qn : cv + (a.step / d) * diff;
        if (!r.edge(cv, tv)) break;
        if (co >= MN) { full = true; break; }
        T.add(o, co, tv, ci);
        ci = co++;
        cv = tv;
        if (last) { met = true; break; }
      }
      na = t ? co : ct;
      nb = t ? ct : co;
      if (full) { status = MIR_PLAN_NODE_LIMIT; break; }
      if (!met) continue;
      // extract: the parents of both trees into one polyline, start first; Tb's walk ends at whichever root it reaches
      const int ia = t ? ci : inew, ib = t ? inew : ci;
      int la = 0, lb = 0, rootb = ib;
      for (int n = ia; n != PLAN_NO_PARENT && la <= MN; n = __builtin_amdgcn_readfirstlane((int)parent[n])) la++;
      for (int n = ib; n != PLAN_NO_PARENT && lb <= MN; n = __builtin_amdgcn_readfirstlane((int)parent[MN + n])) { lb++; rootb = n; }
      if (la + lb - 1 > MIR_PLAN_MAX_POLY) { status = MIR_PLAN_PATH_TOO_LONG; break; }
      int n = ia;
      for (int p = la - 1; p >= 0; p--) {
        if (isd) L.poly[p][lane] = T.node(0, n);
        n = __builtin_amdgcn_readfirstlane((int)parent[n]);
      }
      n = __builtin_amdgcn_readfirstlane((int)parent[MN + ib]);  // (the meeting node is in both trees: once)
      for (int p = la; p < la + lb - 1; p++) {
        if (isd) L.poly[p][lane] = T.node(1, n);
        n = __builtin_amdgcn_readfirstlane((int)parent[MN + n]);
      }
      npoly = la + lb - 1;
      status = MIR_PLAN_OK;
      reached = rootb < nroots ? rootb : -1;  // (a walk cut short by its bound names no root)
      break;
    }
  }
  if (status != MIR_PLAN_OK) {  // the arm stays put: the start W times, a polyline of one node
    if (isd) L.poly[0][lane] = sv;
    npoly = 1;
    reached = -1;
  }
  WSYNC();

  // ---- smooth: shortcuts between two nodes of the polyline
  for (int s = 0; s < a.smooth && npoly >= 3; s++) {
    const float u0 = plan_u(a.seed, (uint32_t)env, 0x80000000u | (uint32_t)s, 0u), u1 = plan_u(a.seed, (uint32_t)env, 0x80000000u | (uint32_t)s, 1u);
    const int i = min((int)(u0 * (float)(npoly - 2)), npoly - 3);
    const int j = i + 2 + min((int)(u1 * (float)(npoly - 2 - i)), npoly - 3 - i);
    if (!r.edge(isd ? L.poly[i][lane] : 0.0f, isd ? L.poly[j][lane] : 0.0f)) continue;
    for (int k = j; k < npoly; k++)  // (every lane moves its own column)
      if (isd) L.poly[i + 1 + k - j][lane] = L.poly[k][lane];
    npoly -= j - i - 1;
  }
  WSYNC();

  // ---- resample: W configurations at equal steps of the cumulative L2 length
  float total = 0.0f;
  for (int k = 0; k + 1 < npoly; k++) {
    const float d = sqrtf(r.norm2(isd ? L.poly[k + 1][lane] - L.poly[k][lane] : 0.0f));
    if (lane == 0) L.cum[k] = total;
    total = total + d;
    if (lane == 0) L.cum[k + 1] = total;
  }
  WSYNC();
  {
    float* const out = a.path + (size_t)row * a.W * D;
    int k = 0;
    for (int w = 0; w < a.W; w++) {
      float q;
      if (npoly == 1 || w == 0) q = isd ? L.poly[0][lane] : 0.0f;
      else if (w == a.W - 1) q = isd ? L.poly[npoly - 1][lane] : 0.0f;
      else {
        const float f = div_refined((float)w, (float)(a.W - 1));
        float t = f;  // (a polyline of one segment: the fraction itself, no length enters)
        if (npoly > 2) {
          const float s = f * total;
          while (k < npoly - 2 && L.cum[k + 1] <= s) k++;
          const float c0 = L.cum[k], len = L.cum[k + 1] - c0;
          t = len > 0.0f ? fminf(div_refined(s - c0, len), 1.0f) : 0.0f;
        }
        const float p0 = isd ? L.poly[k][lane] : 0.0f, p1 = isd ? L.poly[k + 1][lane] : 0.0f;
        q = p0 + t * (p1 - p0);
      }
      if (isd) out[(size_t)w * D + lane] = q;
    }
  }
  if (a.poly) {
    float* const out = a.poly + (size_t)row * MIR_PLAN_MAX_POLY * D;
    for (int k = 0; k < MIR_PLAN_MAX_POLY; k++)
      if (isd) out[(size_t)k * D + lane] = k < npoly ? L.poly[k][lane] : 0.0f;
  }
  if (lane == 0) {
    a.status[row] = status;
    if (a.n_poly) a.n_poly[row] = npoly;
    if (a.stats) {
      int32_t* const st = a.stats + (size_t)row * 4;
      st[0] = iterations; st[1] = na; st[2] = nb; st[3] = r.checked;
    }
  }
  return reached;
}

}  // namespace
