// mir_osc.hip — operational-space dynamics of a list of links in one batched launch: the inverse mass matrix M^-1, M^-1 x, the
// task-space mobility J M^-1 J^T, the operational-space inertia (J M^-1 J^T + damping^2 I)^-1 and the dynamically consistent
// generalised inverse J-bar = M^-1 J^T lambda (mir_task_dynamics, include/mirigid.h; DESIGN.md, operational-space dynamics).
//
// What it serves: the step from M (mir_dyn.hip), J (mir_kin.hip) and Jdot qvel (mir_acc.hip) to an operational-space or impedance
// controller, and forward dynamics qacc = M^-1 (tau - bias).  It reads qpos and the compiled model and writes only its own outputs.
//
// Mapping (the one of mir_dyn.hip): 16 lanes = one DPP row serve one (row, kinematic tree) PAIR, four pairs per wave64.
//   1. poses, spatial inertias, motion subspaces and the composite-rigid-body M block of the tree in LDS: mir_dyn_phases.inc, the
//      fragment mir_dyn.hip includes too.  No Newton-Euler pass.
//   2. Cholesky M = L L^T in place (lower triangle), left-looking: lane i is ROW i; column j is a dot product of row i with row j
//      (the latter a broadcast read), the diagonal leaves through LDS as 1 / L[j][j].  M is SPD by the armature.
//   3. per queried link of THIS tree (the links of other trees are skipped: every (row, link) has one owner, no atomics): the
//      Jacobian column of local dof i is [v_i + w_i x (p - o_tree); w_i] from the motion subspace already in LDS (evaluated as
//      w_i x (p - o_body) for a turning dof), for the dofs whose body's subtree holds the link, zero otherwise -- no second
//      kinematics pass.  Lane a < 6 is TASK ROW a: it solves
//      L y = J[a,:]^T and L^T z = y by itself, y and z in registers (fully unrolled, the factor read as broadcasts: no cross-lane
//      traffic and no separator inside a solve).  lambda_inv = y^T y: entry (a, b), a <= b, belongs to one lane, which writes both
//      triangles.  Every lane then factors the 6 x 6 matrix (+ damping^2 on the diagonal) by Cholesky without pivoting in registers;
//      lane c < 6 solves for column c of lambda; lane i (DOF i again) forms its row of J-bar = z lambda, and the link's owner writes
//      the rows of the other trees' dofs as zeros.
//   4. M^-1 and M^-1 x on the same factor: lane c < 15 solves for column c (right-hand side e_c), lane 15 -- a tree has at most 15
//      dofs -- for x.  Entry (r, c) of M^-1 is taken from lane min(r, c), so the block is bitwise symmetric; it replaces the factor
//      in LDS and leaves like the M window of mir_dyn.hip.
// Loops whose trip count depends on the tree (pivot columns, substitution rows, links) run to the launch-wide maximum with
// predication: WSYNC is wave-level and the four pairs of a wave are different trees.  The pairs behind the last one are clamped to
// it and their stores predicated.
//
// Stores: 4-byte, every element written exactly once.  No atomics, no scratch.
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

#include "mir_dyn_body.h"

namespace {

constexpr int OSC_N = 15;            // dofs of a tree at most (DYN_NONE)
constexpr float OSC_PIVOT = 1e-5f;   // relative pivot at or below which lambda and jbar are NaN (the rule of the header)

struct OscArgs {
  DynTree tree[DYN_MAX_TREE];
  uint16_t link[MIR_MAX_BODY];  // tree of queried link l | local body << 8
  float local_point[MIR_MAX_BODY][3];
  int n_trees, nb_max, nd_max, depth_max;
  int n_links, dof0, n_dofs;
  int n_rows, B, qst, nq, nv;
  float damping2;
  const long long* env_idx;
  const float *qpos, *qpos_o, *x;
  JointPtrs m;
  InertiaPtrs mi;
  float *minv, *solve, *lambda_inv, *lambda, *jbar;
};
static_assert(sizeof(OscArgs) <= 4096, "kernel arguments");
static_assert(MIR_MAX_BODY <= 256 && DYN_MAX_TREE <= 256, "OscArgs::link");

struct OscLds {
  float xp[G][4], xq[G][4];  // world pose per body
  float ci[G][12];           // spatial inertia per body {m, h, xx yy zz xy xz yz}
  float cd[G][8];            // motion subspace per dof {w, v}
  float M[G][G + 1];         // the M block, then its Cholesky factor (lower triangle), then M^-1; rows padded (lane i reads row i)
  float dinv[G];             // 1 / L[k][k], 0 behind the tree's dofs
  float Jt[6][G];            // task row a: J[a][i]
  float Y[6][G], Z[6][G];    // L^-1 J^T and M^-1 J^T per task row; Y[0] carries M^-1 x in phase 4
  float A[6][8], Lam[6][8];  // lambda_inv, lambda
  int pd[G], sd[G];          // parent dof (local), scene dof
  uint8_t inv[MIR_MAX_DOF];  // scene dof -> local dof, 0xff: another tree's
};

// The library is built with approximate division and square root (csrc/Makefile: v_rcp / v_sqrt + one refinement, <= 2.5 ulp).  A
// factorisation feeds every such error through |M^-1| ~ 1 / armature, so here each gets one more Newton step, which leaves them
// within an ulp of the correctly rounded value: d ~ sqrt(s), r ~ 1 / d, and s / d from both.
__device__ __forceinline__ float sqrt_nr(float s) {
  const float d = sqrtf(s);
  return fmaf(fmaf(-d, d, s), 0.5f / d, d);
}
__device__ __forceinline__ float rcp_nr(float d) {
  const float r = 1.0f / d;
  return fmaf(fmaf(-d, r, 1.0f), r, r);
}
__device__ __forceinline__ float div_nr(float s, float d, float r) {  // s / d with r ~ 1 / d (d = r = 0: 0)
  const float q = s * r;
  return fmaf(fmaf(-q, d, s), r, q);
}

// v: right-hand side in, L^-T L^-1 v out; y: L^-1 v.  Rows / columns from n on (uniform) are skipped and give zeros; inside n, the
// rows behind a smaller tree's dofs are zero rows of the factor with dinv = 0.  Forward by rows (the serial order), backward by columns.
__device__ __forceinline__ void chol_solve(const OscLds& L, int n, float (&v)[OSC_N], float (&y)[OSC_N]) {
#pragma unroll
  for (int i = 0; i < OSC_N; i++) {
    y[i] = 0.0f;
    if (i < n) {
      float s = v[i];
#pragma unroll
      for (int k = 0; k < i; k++) s = fmaf(-L.M[i][k], y[k], s);
      y[i] = div_nr(s, L.M[i][i], L.dinv[i]);
    }
  }
#pragma unroll
  for (int i = 0; i < OSC_N; i++) v[i] = y[i];
#pragma unroll
  for (int k = OSC_N - 1; k >= 0; k--) {
    if (k < n) {
      v[k] = div_nr(v[k], L.M[k][k], L.dinv[k]);
#pragma unroll
      for (int i = 0; i < k; i++) v[i] = fmaf(-L.M[k][i], v[k], v[i]);
    }
  }
}

__global__ __launch_bounds__(64) void mir_osc_kernel(OscArgs a) {
  __shared__ __attribute__((aligned(16))) OscLds lds[4];
  OscLds& L = lds[threadIdx.x >> 4];
  L.dinv[threadIdx.x & 15] = 0.0f;
  const bool want_mass = true;
  // ---- 1. poses, inertias, motion subspaces, the M block
#include "mir_dyn_phases.inc"
  WSYNC();  // (the M block is complete)
  // ---- 2. Cholesky in place: lane i is row i
  const int nmax = a.nd_max;
  for (int j = 0; j < nmax; j++) {
    float s = L.M[lane][j];
    for (int k = 0; k < j; k++) s = fmaf(-L.M[lane][k], L.M[j][k], s);
    if (lane == j && j < nd) {
      const float d = sqrt_nr(s);
      L.M[j][j] = d;
      L.dinv[j] = rcp_nr(d);
    }
    WSYNC();
    if (lane > j && lane < nd) L.M[lane][j] = div_nr(s, L.M[j][j], L.dinv[j]);
    WSYNC();
  }
  const int nw = a.n_dofs, col = sdof - a.dof0;
  const bool mine = valid && isdof && col >= 0 && col < nw;
  // ---- 3. the queried links of my tree
  const V3 obody = ld3(L.xp[isdof ? dbody : 0]);
  const int jtd = (a.tree[ti].body[isdof ? dbody : 0] >> 8) & 3, comp = isdof ? (int)((a.tree[ti].dof[lane] >> 16) & 7) : 0;
  const bool slides = jtd == MIR_JNT_PRISMATIC || (jtd == MIR_JNT_FREE && comp < 3);  // (a dof that translates: its column is [v; 0])
  const bool want_lambda = a.lambda || a.jbar;
  for (int l = 0; l < a.n_links; l++) {
    const int lw = a.link[l];
    const bool own = (lw & 0xff) == ti;
    if (__builtin_amdgcn_ballot_w64(own) == 0) continue;  // (uniform: no pair of this wave owns the link)
    const int lb = own ? lw >> 8 : 0;
    const bool st = own && valid;
    const size_t pl = (size_t)row * a.n_links + l;
    // the Jacobian column of my dof at p = o_link + R_link local_point (the point of mir_kin.hip): [v + w x (p - o_tree); w] of my
    // motion subspace {w, v}.  For a turning dof v = w x (o_tree - o_body), so the column is w x (p - o_body) with my body's origin
    // from LDS -- the lever arm of mir_kin.hip, one cross product and its rounding fewer than the sum through the tree origin.
    const V3 p = ld3(L.xp[lb]) + qrot(qnormalize(ld4(L.xq[lb])), ld3(a.local_point[l]));
    const bool on = isdof && (sub >> lb & 1);
    const V3 lin = !on ? v3(0, 0, 0) : (slides ? S.b : cross(S.a, p - obody)), ang = on ? S.a : v3(0, 0, 0);
    L.Jt[0][lane] = lin.x; L.Jt[1][lane] = lin.y; L.Jt[2][lane] = lin.z;
    L.Jt[3][lane] = ang.x; L.Jt[4][lane] = ang.y; L.Jt[5][lane] = ang.z;
    WSYNC();
    // lane a < 6 is task row a (the others repeat row 0 and store nothing)
    const int ta = lane < 6 ? lane : 0;
    float v[OSC_N], y[OSC_N];
#pragma unroll
    for (int i = 0; i < OSC_N; i++) v[i] = L.Jt[ta][i];
    chol_solve(L, nmax, v, y);
    if (lane < 6) {
#pragma unroll
      for (int i = 0; i < OSC_N; i++) { L.Y[lane][i] = y[i]; L.Z[lane][i] = v[i]; }
    }
    WSYNC();
    // lambda_inv = y^T y: the 21 entries a <= b over the lanes, both triangles by the owner
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int e = lane + 16 * h;
      if (e < 21) {
        const int ra = (e >= 6) + (e >= 11) + (e >= 15) + (e >= 18) + (e >= 20);
        const int rb = ra + e - (ra * 6 - ra * (ra - 1) / 2);
        float s = 0.0f;
        for (int i = 0; i < nmax; i++) s = fmaf(L.Y[ra][i], L.Y[rb][i], s);
        L.A[ra][rb] = s;
        L.A[rb][ra] = s;
        if (a.lambda_inv && st) {
          a.lambda_inv[pl * 36 + ra * 6 + rb] = s;
          a.lambda_inv[pl * 36 + rb * 6 + ra] = s;
        }
      }
    }
    WSYNC();
    if (want_lambda) {  // (uniform)
      // Cholesky of lambda_inv + damping^2 I without pivoting, in every lane; a pivot at or below OSC_PIVOT x the largest diagonal
      // entry: NaN
      float c[6][6];
      float dmax = 0.0f;
#pragma unroll
      for (int i = 0; i < 6; i++) {
#pragma unroll
        for (int j = 0; j <= i; j++) c[i][j] = L.A[i][j];
        c[i][i] += a.damping2;
        dmax = fmaxf(dmax, c[i][i]);
      }
      const float thr = OSC_PIVOT * dmax;
      bool ok = true;
      float ci[6];  // 1 / c[j][j]
#pragma unroll
      for (int j = 0; j < 6; j++) {
        float s = c[j][j];
#pragma unroll
        for (int k = 0; k < j; k++) s = fmaf(-c[j][k], c[j][k], s);
        ok = ok && s > thr;
        c[j][j] = sqrt_nr(s);
        ci[j] = rcp_nr(c[j][j]);
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
          float u = c[i][j];
#pragma unroll
          for (int k = 0; k < j; k++) u = fmaf(-c[i][k], c[j][k], u);
          c[i][j] = div_nr(u, c[j][j], ci[j]);
        }
      }
      // lane cc < 6: column cc of lambda (the others repeat column 0)
      const int cc = lane < 6 ? lane : 0;
      float w[6];
#pragma unroll
      for (int i = 0; i < 6; i++) {
        float s = i == cc ? 1.0f : 0.0f;
#pragma unroll
        for (int k = 0; k < i; k++) s = fmaf(-c[i][k], w[k], s);
        w[i] = div_nr(s, c[i][i], ci[i]);
      }
#pragma unroll
      for (int i = 5; i >= 0; i--) {
        float s = w[i];
#pragma unroll
        for (int k = i + 1; k < 6; k++) s = fmaf(-c[k][i], w[k], s);
        w[i] = div_nr(s, c[i][i], ci[i]);
      }
      const float qnan = __builtin_nanf("");
      if (lane < 6) {
#pragma unroll
        for (int i = 0; i < 6; i++) {
          const float u = ok ? w[i] : qnan;
          L.Lam[i][lane] = w[i];
          if (a.lambda && st) a.lambda[pl * 36 + lane * 6 + i] = u;  // (row `lane` = column `lane`: lambda is symmetric)
        }
      }
      WSYNC();
      if (a.jbar) {  // (uniform) my dof's row of z lambda
        float zr[6];
#pragma unroll
        for (int k = 0; k < 6; k++) zr[k] = L.Z[k][lane];
#pragma unroll
        for (int b = 0; b < 6; b++) {
          float s = 0.0f;
#pragma unroll
          for (int k = 0; k < 6; k++) s = fmaf(zr[k], L.Lam[k][b], s);
          if (mine && own) a.jbar[(pl * nw + col) * 6 + b] = ok ? s : qnan;
        }
        // the rows of the other trees' dofs: zeros (NaN with the rest where the task space is singular), by the link's owner
        if (st) {
          for (int c = lane; c < nw; c += G) {
            if (L.inv[a.dof0 + c] != 0xff) continue;
#pragma unroll
            for (int b = 0; b < 6; b++) a.jbar[(pl * nw + c) * 6 + b] = ok ? 0.0f : qnan;
          }
        }
      }
    }
    WSYNC();  // (the next link writes Jt / Y / Z / A / Lam again)
  }
  // ---- 4. M^-1 and M^-1 x: lane c < 15 solves for column c, lane 15 for x
  if (a.minv || a.solve) {  // (uniform)
    float v[OSC_N], y[OSC_N];
    const float* const xrow = a.solve ? a.x + (size_t)row * a.nv : nullptr;
#pragma unroll
    for (int i = 0; i < OSC_N; i++) {
      v[i] = i == lane ? 1.0f : 0.0f;
      if (lane == OSC_N && xrow && i < nd) v[i] = xrow[L.sd[i]];
    }
    chol_solve(L, nmax, v, y);
    WSYNC();  // (every lane has read the factor)
#pragma unroll
    for (int i = 0; i < OSC_N; i++) {
      if (lane == OSC_N) {
        L.Y[0][i] = v[i];
      } else if (i >= lane) {
        L.M[lane][i] = v[i];
        L.M[i][lane] = v[i];
      }
    }
    WSYNC();
    if (a.solve && mine) a.solve[(size_t)row * nw + col] = L.Y[0][lane];
    // the rows of the window that belong to my tree: all n_dofs columns of each, zeros where the column is another tree's
    if (a.minv) {
      for (int i = 0; i < nmax; i++) {
        const int rr = (i < nd ? L.sd[i] : -1) - a.dof0;
        if (!valid || i >= nd || rr < 0 || rr >= nw) continue;  // (uniform over the 16 lanes)
        float* const out = a.minv + ((size_t)row * nw + rr) * nw;
        for (int c = lane; c < nw; c += G) {
          const int tt = L.inv[a.dof0 + c];
          out[c] = tt != 0xff ? L.M[i][tt] : 0.0f;
        }
      }
    }
  }
}

}  // namespace

extern "C" int mir_task_query_sizeof(void) { return (int)sizeof(MirTaskQuery); }

extern "C" int mir_task_dynamics(MirHandle h, const MirTaskQuery* q, const int64_t* env_idx, int32_t n_rows, const float* qpos, const float* x,
                                 float* minv, float* solve, float* lambda_inv, float* lambda, float* jbar, void* stream) {
  const char* const who = "mir_task_dynamics";
  if (!h || !q) return query_error(MIR_E_INVALID, who, "null argument");
  if (q->struct_size != (int32_t)sizeof(MirTaskQuery)) return query_error(MIR_E_INVALID, who, "struct_size is not sizeof(MirTaskQuery)");
  if (q->flags != 0) return query_error(MIR_E_INVALID, who, "unknown flag bit");
  if (q->n_links < 0 || q->n_links > MIR_MAX_BODY) return query_error(MIR_E_INVALID, who, "n_links outside 0 .. MIR_MAX_BODY");
  for (int l = 0; l < q->n_links; l++) {
    if (q->link_body[l] <= 0 || q->link_body[l] >= h->nbody) return query_error(MIR_E_INVALID, who, "link out of range");
    for (int k = 0; k < 3; k++)
      if (!std::isfinite(q->local_point[l][k])) return query_error(MIR_E_INVALID, who, "local_point is not finite");
  }
  if (!std::isfinite(q->damping) || q->damping < 0.0f) return query_error(MIR_E_INVALID, who, "damping is negative or not finite");
  if (q->dof0 < 0 || q->n_dofs < 0 || q->dof0 > h->nv || q->n_dofs > h->nv - q->dof0) return query_error(MIR_E_INVALID, who, "dof window outside [0, nv]");
  if (solve && !x) return query_error(MIR_E_INVALID, who, "solve needs x");
  if ((lambda_inv || lambda || jbar) && q->n_links == 0) return query_error(MIR_E_INVALID, who, "lambda_inv, lambda and jbar need a link");
  if (h->pending) return query_error(MIR_E_INVALID, who, "a step is pending (mir_step_end first)");
  if (env_idx && n_rows < 0) return query_error(MIR_E_INVALID, who, "negative n_rows");
  const long long R = env_idx ? n_rows : h->B, n = q->n_dofs, nl = q->n_links;
  OscArgs a;
  memset(&a, 0, sizeof a);
  DynTrees T;
  if (int rc = dyn_build_trees(h, a.tree, T, who)) return rc;
  for (int l = 0; l < q->n_links; l++) {
    const int b = q->link_body[l];
    if (T.tree_of[b] < 0) return query_error(MIR_E_INVALID, who, "a link whose kinematic tree has no dofs");
    a.link[l] = (uint16_t)(T.tree_of[b] | T.local[b] << 8);
    for (int k = 0; k < 3; k++) a.local_point[l][k] = q->local_point[l][k];
  }
  const long long lim = 0x7fffffffLL;
  if ((minv && R * n * n > lim) || (solve && R * n > lim) || ((lambda_inv || lambda) && R * nl * 36 > lim) || (jbar && R * nl * n * 6 > lim))
    return query_error(MIR_E_CAPACITY, who, "an output of 2^31 elements or more");
  // (what is asked for and empty is not computed)
  if (n == 0) minv = solve = jbar = nullptr;
  if (R == 0 || (!minv && !solve && !lambda_inv && !lambda && !jbar)) return MIR_OK;  // (nothing asked for)
  a.n_trees = T.n_trees; a.nb_max = T.nb_max; a.nd_max = T.nd_max; a.depth_max = T.depth_max;
  a.n_links = (lambda_inv || lambda || jbar) ? q->n_links : 0;
  a.dof0 = q->dof0; a.n_dofs = q->n_dofs;
  a.n_rows = (int)R; a.B = h->B; a.qst = h->pt.qst; a.nq = h->nq; a.nv = h->nv;
  a.damping2 = q->damping * q->damping;
  a.env_idx = reinterpret_cast<const long long*>(env_idx);
  a.qpos = h->qpos; a.qpos_o = qpos; a.x = x;
  const ModelView mv(h);
  a.m = mv.joint_pointers(); a.mi = mv.inertia_pointers();
  a.minv = minv; a.solve = solve; a.lambda_inv = lambda_inv; a.lambda = lambda; a.jbar = jbar;
  const long long n_pairs = R * T.n_trees;
  if (n_pairs > 0x7fffffffLL - 4) return query_error(MIR_E_CAPACITY, who, "rows x trees reaches 2^31");
  return launch_rows(h, mir_osc_kernel, (n_pairs + 3) / 4, stream, a);
}
