// mir_cert.hip — certified swept clearance of joint paths (mir_certify_path, mir_certify_path_self, mir_certify_path_carry);
// include/mirigid.h and DESIGN.md, "Certified clearance" and "Certified clearance: self and carried object".
//
// What it serves: "is this trajectory I already have clear?", answered for the whole of every segment, not for samples of it.  For a
// list of envs, one launch brackets the continuous minimum clearance of the sphere model against the static scene on every segment of
// each row's joint-space path: the signed distance is 1-Lipschitz in a sphere's centre, a centre moves no faster along a segment than
// v_i = sum_j |dq_j| rho_ij, so one evaluation at the midpoint of an interval bounds the clearance on all of it, and the interval is
// bisected where that bound does not decide.
//   With a self query (SELF) the same bisection carries a second bracket: the distance s_ij of two spheres changes no faster than
//   v_ij = rel(i, c) + rel(j, c), where c is the lowest common ancestor of their links and rel sums |dq_k| rho_ik over the planned dofs
//   strictly below c only -- a joint above both spheres turns them together and leaves their distance alone.  With a carried body
//   (CARRY) its spheres are spheres of the attach link at a distance of at most |p_G| + |c_i| from its origin.
//
// Mapping: one kernel, mir_cert_kernel<SELF, CARRY>, one workgroup of one wave64 per row, as mir_path_clear_kernel, on the row machinery
// of mir_plan_row.h (PlanRow<SELF, CARRY>, plan_setup), which is unchanged: the start row, every body's pose, the geom records, and the
// forward kinematics of the bodies below a planned dof (PlanRow::fk).  Lane j < D holds dof j of the segment's ends; lane = body for the
// chain lengths S and the sums A, B, P (parents before children, one round per tree depth, through LDS); lane = probe in chunks of 64
// for the speed bounds v_i (LDS, one float per probe) and for the evaluation.
//   The evaluation is a reduction of its own beside PlanRow::clearance_at_poses: probe_world and dist_probe_min give d_i, and one pass
//   yields u = min_i d_i and min_i (d_i - hw v_i) with the not-finite ballot of the planner.  An endpoint (hw = 0) returns m = u.
//   The bisection is stackless: the node (l, k) and its dyadic successor are two scalars (mir_cert_front.h, which also holds the
//   recurrences and the host checks; mir_certrel_front.h holds the relative rule and the status order; the CPU tests build both with g++).
//   What the template adds, and nothing of it exists in an instantiation that does not read it:
//   SELF or CARRY  per row cn_i per sphere (with |p_G| of the row's grasp for the spheres on the carried body), and v behind it, in
//                  dynamic LDS; without either, |c_i| is taken anew per segment, v is 4 KB of static LDS and there is no dynamic LDS.
//   CARRY          the carried body's S, A, B, P are its attach link's.
//   SELF           per row the LCA table (nbody x nbody bytes, built by the host) and each body's chain depth go to LDS.  Per segment
//                  lane = body walks a, parent(a), ... and stores the three branch sums (dA, dSB, dP) after 0 .. depth + 1 bodies:
//                  U[a][t], 17 x 16 bytes per body.  Per evaluation the scene half also writes the sphere list; then the pair loop in
//                  the shape of self_probe_min: lane = sphere i, j wave-uniform through v_readlane, and per pair three LDS reads: the
//                  LCA byte of the two links and the two table rows U[a][t_i], U[b][t_j].  It keeps the lowest s and the lowest
//                  min(s, self_max) - hw v_ij.
// Bounds: every loop is bounded by K, the tree depth (<= 16), N + E, max_depth (through the successor) or max_evaluations: the
//   evaluation counter is compared before every evaluation, so no input can keep a wave running.
// Stores: plain dword stores by lane 0 (outputs, leaves) or into LDS.  No atomics, no scratch, no cross-wave barrier.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <cstring>
#include <type_traits>

#include "mir_model.h"
#include "mir_model64.h"
#include "mir_scene.h"

#define G 16
#include "mir_dev.h"

#include "mir_query.h"
#include "mir_sphere_front.h"  // (brings mir_dist_body.h)

#include "mir_self_body.h"

#include "mir_plan_row.h"

#include "mir_certrel_front.h"  // (brings mir_cert_front.h)

namespace {

struct CertArgs {
  PlanArgs p;  // the clearance side, as mir_path_clearance and its _self / _carry forms fill it
  int K, max_depth, max_eval, max_leaves, bracket;
  float tol, guard;
  const float* paths;
  float *seg_lower, *seg_upper, *seg_self_lower, *seg_self_upper, *row_lower, *row_upper, *row_self_lower, *row_self_upper;
  int32_t *seg_status, *row_status, *row_first, *leaves, *stats;
  uint8_t lca[MIR_MAX_BODY * MIR_MAX_BODY];  // SELF: certrel_lca_table, row stride MIR_MAX_BODY
};
static_assert(sizeof(CertArgs) <= 4096, "kernel arguments");

// what the rule keeps in LDS beside the row's: the ends of the segment per dof, the chains per body.  SELF only: per body its planned
// dof's |dq|, kind and |axis|, its parent and the chain depth of the link it counts as (-1: the world); the branch sums; the LCA table.
// Without SELF and CARRY only: the speed bound per probe (with either, it follows cn in dynamic LDS)
struct CertChainLds {
  float adq[PLAN_MAX_DOF], amax[PLAN_MAX_DOF];
  float S[MIR_MAX_BODY], A[MIR_MAX_BODY], B[MIR_MAX_BODY], P[MIR_MAX_BODY];
};
struct CertPairLds {
  float badq[MIR_MAX_BODY], baxl[MIR_MAX_BODY];
  int bkind[MIR_MAX_BODY], bdep[MIR_MAX_BODY], bpar[MIR_MAX_BODY];
  float U[MIR_MAX_BODY][CERTREL_STEPS][4];
  uint8_t lca[MIR_MAX_BODY * MIR_MAX_BODY];
};
struct CertSpeedLds {
  float v[DIST_MAX_PROBES];
};
struct CertNoPairLds {};
struct CertNoSpeedLds {};
template <bool SELF, bool CARRY>
struct CertLds : CertChainLds, std::conditional_t<SELF, CertPairLds, CertNoPairLds>, std::conditional_t<SELF || CARRY, CertNoSpeedLds, CertSpeedLds> {};
template <bool SELF, bool CARRY>
constexpr size_t CERT_FIXED_LDS = sizeof(PlanLds) + sizeof(CertLds<SELF, CARRY>);
static_assert(sizeof(CertLds<false, true>) == sizeof(CertChainLds), "the pair part and the speed bounds are empty with a carried body alone");

// the dynamic LDS of a row with SELF or CARRY (certrel_lds_bytes): SELF: the sphere list (16 bytes x NS); cn (NS); v (N)
extern __shared__ float cert_dyn[];

// one evaluation: u = min_i d_i, m = min_i (d_i - hw v_i); SELF: us = min(self_max, min s_ij), ms = min(self_max, min(min(s_ij,
// self_max) - hw v_ij)); nf: a centre is not finite
struct CertEval {
  float u, m, us, ms;
  bool nf;
};

template <bool SELF, bool CARRY>
__global__ __launch_bounds__(64) void mir_cert_kernel(CertArgs a) {
  constexpr bool REL = SELF || CARRY;
  __shared__ PlanLds L;
  __shared__ CertLds<SELF, CARRY> C;
  const int lane = threadIdx.x, row = blockIdx.x, D = a.p.D, N = a.p.N, NS = a.p.NS, K = a.K;
  float* const sph = cert_dyn;
  float* const cnl = cert_dyn + (SELF ? 4 * NS : 0);
  float* vl;
  if constexpr (REL)
    vl = cnl + NS;
  else
    vl = C.v;
  PlanRow<SELF, CARRY> r{a.p, L, lane, 0, 0, false, SELF ? sph : nullptr, SELF_LIST};
  plan_setup(r, row, sphere_row_env(a.p.r, row));
  const bool isd = lane < D;

  // ---- what a body keeps through the launch (lane = body): its word, |pos|, |axis|, its planned dof, the slide of an unplanned
  // prismatic joint in the row
  const bool isb = lane > 0 && lane < a.p.r.nbody;
  const int b = isb ? lane : 0;
  const uint32_t bw = a.p.r.body[b];
  const int par = bw & 0xff, jt = (bw >> 8) & 3, depth = (bw >> 10) & 31;
  float pos_len = 0.0f, axis_len = 0.0f, slide = 0.0f;
  int jd = -1;
  if (isb && jt != MIR_JNT_FREE) {
    const V3 bp = ld3(a.p.r.m.b_pos + b * 3);
    pos_len = sqrtf(bp.x * bp.x + bp.y * bp.y + bp.z * bp.z);
    if (jt == MIR_JNT_REVOLUTE || jt == MIR_JNT_PRISMATIC) {
      const int qa = a.p.r.m.b_qadr[b];
      for (int j = 0; j < D; j++)
        if (a.p.qadr[j] == qa) jd = j;
      if (jt == MIR_JNT_PRISMATIC) {
        const V3 ax = ld3(a.p.r.m.b_axis + b * 3);
        axis_len = sqrtf(ax.x * ax.x + ax.y * ax.y + ax.z * ax.z);
        slide = fabsf(L.qrow[qa]);
      }
    }
  }
  const int kind = jd < 0 ? 0 : (jt == MIR_JNT_REVOLUTE ? 1 : 2);
  const bool root = depth == 0;
  // the link this body counts as: the carried body rides on its attach link
  const int eb = CARRY && isb && b == a.p.carry_body ? a.p.carry_link : b;
  // |c_i| of a sphere in its link's frame
  const auto centre_len = [&](int i) {
    const V3 c = ld3(a.p.r.probes + (size_t)i * 4);
    return sqrtf(c.x * c.x + c.y * c.y + c.z * c.z);
  };

  // ---- per row: the tables that do not depend on the segment
  if constexpr (SELF) {
    if (lane < MIR_MAX_BODY) {
      C.bkind[lane] = isb ? kind : 0;
      C.baxl[lane] = axis_len;
      C.bpar[lane] = par;
      C.bdep[lane] = eb > 0 ? (int)((a.p.r.body[eb] >> 10) & 31) : -1;
    }
    for (int i = lane; i < MIR_MAX_BODY * MIR_MAX_BODY / 4; i += 64)
      reinterpret_cast<uint32_t*>(C.lca)[i] = reinterpret_cast<const uint32_t*>(a.lca)[i];
  }
  if constexpr (REL) {
    float grasp_len = 0.0f;
    if constexpr (CARRY) grasp_len = sqrtf(r.gp.x * r.gp.x + r.gp.y * r.gp.y + r.gp.z * r.gp.z);
    for (int i = lane; i < NS; i += 64) {
      const float cn = centre_len(i);
      cnl[i] = CARRY && a.p.r.link[i] == a.p.carry_body ? certrel_cn_carried(grasp_len, cn) : cn;
    }
    WSYNC();
  }

  // the pair half of one evaluation on the sphere list (SELF): TRACK: hw > 0 (an endpoint has hw = 0: its bound is the capped distance itself)
  const auto pairs = [&](float hw, auto track, float& us, float& ms) {
    constexpr bool TRACK = decltype(track)::value;
    if constexpr (SELF) {  // (the pair part of C exists)
      float lo_s = INFINITY, lo_b = INFINITY;
      for (int base = 0; base < NS; base += 64) {
        const bool valid = base + lane < NS;
        const int i = valid ? base + lane : NS - 1;
        const int la = a.p.r.link[i];
        const uint32_t mask = valid ? a.p.link_mask[la] : 0u;
        const float xi = sph[4 * i], yi = sph[4 * i + 1], zi = sph[4 * i + 2], ri = sph[4 * i + 3];
        const float cni = cnl[i];
        const int di = C.bdep[la];
        for (int cb = base; cb < NS; cb += 64) {  // (s and v are symmetric: the pairs with j in an earlier chunk were seen from the other side)
          const int mine = cb + lane < NS ? cb + lane : NS - 1;
          const float xm = sph[4 * mine], ym = sph[4 * mine + 1], zm = sph[4 * mine + 2], rm = sph[4 * mine + 3];
          const int lm = a.p.r.link[mine];
          const float cnm = cnl[mine];
          const int dm = C.bdep[lm];
          const int cnt = NS - cb < 64 ? NS - cb : 64;
          for (int k = 0; k < cnt; k++) {
            const float s = self_pair(xi, yi, zi, ri, lane_bcast(xm, k), lane_bcast(ym, k), lane_bcast(zm, k), lane_bcast(rm, k));
            const int lj = __builtin_amdgcn_readlane(lm, k);
            const bool on = (mask >> lj) & 1u;
            lo_s = fminf(lo_s, on ? s : INFINITY);
            if constexpr (TRACK) {
              const int lc = C.lca[la * MIR_MAX_BODY + lj];
              const int ti = certrel_steps(di, lc), tj = certrel_steps(__builtin_amdgcn_readlane(dm, k), lc);
              const V3 ui = ld3(C.U[la][ti]), uj = ld3(C.U[lj][tj]);
              const float v = certrel_speed(certrel_rel(cni, ui.x, ui.y, ui.z), certrel_rel(lane_bcast(cnm, k), uj.x, uj.y, uj.z));
              lo_b = fminf(lo_b, on ? certrel_pair_bound(s, a.p.self_max, hw, v) : INFINITY);
            }
          }
        }
      }
      us = fminf(a.p.self_max, wave_min(lo_s));
      ms = TRACK ? fminf(a.p.self_max, wave_min(lo_b)) : us;
    }
  };

  // one evaluation at the configuration q (lane j: dof j), finite by the caller's tests
  const auto evaluate = [&](float q, float hw) {
    if (isd) L.qrow[a.p.qadr[lane]] = q;
    WSYNC();
    r.fk(false);
    float u = INFINITY, m = INFINITY;
    unsigned long long nan = 0ull;
    for (int base = 0; base < N; base += 64) {
      const bool valid = base + lane < N;
      const int probe = valid ? base + lane : N - 1;
      const ProbeWorld p = probe_world(a.p.r, probe, L.xp, L.xq);
      const DistBest w = dist_probe_min(L.rec, r.count, a.p.t.planes, a.p.t.tris, p.c, p.radius, a.p.max_distance);
      const bool hit = w.bestk >= 0 && w.best <= a.p.max_distance;
      const float dist = hit ? w.best : a.p.max_distance;
      nan |= probe_nonfinite(valid, p.c);
      if (valid) {
        const float reach = hw * vl[probe];  // (a power of two times v: exact)
        u = fminf(u, dist);
        m = fminf(m, dist - reach);
      }
      if constexpr (SELF)
        if (valid) sphere_store(sph, probe, p.c, &p.radius);
    }
    CertEval e{wave_min(u), wave_min(m), INFINITY, INFINITY, nan != 0ull};
    if (!(hw > 0.0f)) e.m = e.u;  // (an endpoint's bound is the distance itself, whatever v holds)
    if constexpr (SELF) {
      e.nf = e.nf || sphere_list_fill(a.p.r, N, NS, lane, L.xp, L.xq, sph) != 0ull;  // the extra probes: no scene test
      WSYNC();  // (the list is written)
      if (!e.nf) {
        if (hw > 0.0f)
          pairs(hw, std::true_type{}, e.us, e.ms);
        else
          pairs(hw, std::false_type{}, e.us, e.ms);
      }
      WSYNC();  // (before the next configuration overwrites the list)
    }
    return e;
  };

  const float* const path = a.paths + (size_t)row * K * D;
  int32_t* const leaves = a.leaves ? a.leaves + (size_t)row * a.max_leaves * 3 : nullptr;
  const float margin = a.p.margin, self_margin = a.p.self_margin;
  const bool bracket = a.bracket != 0;
  int evals = 0, n_leaves = 0, deepest = 0, finished = 0, first = -1, rstatus = MIR_CERT_CLEAR;
  bool spent = false;
  float rlower = INFINITY, rupper = INFINITY, rlower_s = INFINITY, rupper_s = INFINITY;
  float av = isd ? path[lane] : 0.0f;
  for (int s = 0; s + 1 < K; s++) {
    const float bv = isd ? path[(size_t)(s + 1) * D + lane] : 0.0f;
    const float dq = bv - av;
    float lower = INFINITY, upper = INFINITY, lower_s = INFINITY, upper_s = INFINITY;
    bool nf = r.bad, budget = false, depth_hit = false, done = false;
    if (a.p.ignore) {
      lower = upper = a.p.max_distance;
      if constexpr (SELF) lower_s = upper_s = a.p.self_max;
      nf = false;
      done = true;
      finished++;
    } else if (!nf && __ballot(isd && (nonfinite(av) || nonfinite(bv) || nonfinite(dq))) != 0ull) {
      nf = true;
    }
    if (!done && !nf && spent) budget = true;
    if (!done && !nf && !budget) {
      // ---- 1., 2. the chain lengths and the speed bounds of this segment
      if (isd) {
        C.adq[lane] = fabsf(dq);
        C.amax[lane] = fmaxf(fabsf(av), fabsf(bv));
      }
      WSYNC();
      {
        const float adq = jd >= 0 ? C.adq[jd] : 0.0f;
        const float pris = jt == MIR_JNT_PRISMATIC ? (jd >= 0 ? C.amax[jd] : slide) * axis_len : 0.0f;
        if constexpr (SELF)
          if (lane < MIR_MAX_BODY) C.badq[lane] = isb ? adq : 0.0f;
        if (lane == 0) C.S[0] = C.A[0] = C.B[0] = C.P[0] = 0.0f;
        for (int lvl = 0; lvl <= a.p.r.depth_max; lvl++) {
          if (isb && depth == lvl) {
            const float sb = cert_chain(root, root ? 0.0f : C.S[par], pos_len, pris);
            C.S[b] = sb;
            C.A[b] = cert_sum_a(root, root ? 0.0f : C.A[par], kind, adq);
            C.B[b] = cert_sum_b(root, root ? 0.0f : C.B[par], kind, adq, sb);
            C.P[b] = cert_sum_p(root, root ? 0.0f : C.P[par], kind, adq, axis_len);
          }
          WSYNC();
        }
        if constexpr (CARRY) {  // the carried body counts as its attach link
          if (isb && eb != b) {
            C.S[b] = C.S[eb];
            C.A[b] = C.A[eb];
            C.B[b] = C.B[eb];
            C.P[b] = C.P[eb];
          }
          WSYNC();
        }
      }
      for (int i = lane; i < N; i += 64) {
        const int lk = a.p.r.link[i];
        float cn;
        if constexpr (REL)
          cn = cnl[i];
        else
          cn = centre_len(i);
        vl[i] = cert_speed(C.S[lk], cn, C.A[lk], C.B[lk], C.P[lk]);
      }
      if constexpr (SELF) {  // the branch sums: lane = body, walking upward from the link it counts as
        if (lane < MIR_MAX_BODY) {
          float dA = 0.0f, dSB = 0.0f, dP = 0.0f;
          const float s_link = C.S[eb];
          int k = eb;
          bool walking = isb;
          float* const u0 = C.U[lane][0];
          u0[0] = u0[1] = u0[2] = 0.0f;
          for (int t = 0; t <= a.p.r.depth_max; t++) {
            if (walking) {
              const int kk = C.bkind[k];
              const float ad = C.badq[k];
              dA = certrel_step_a(dA, kk, ad);
              dSB = certrel_step_sb(dSB, kk, ad, s_link, C.S[k]);
              dP = certrel_step_p(dP, kk, ad, C.baxl[k]);
              float* const u = C.U[lane][t + 1];
              u[0] = dA; u[1] = dSB; u[2] = dP;
              walking = t < C.bdep[lane];
              k = C.bpar[k];
            }
          }
        }
      }
      WSYNC();

      // ---- 3. the endpoints: P_0 for segment 0 only, P_{s+1} for every segment
      bool ended = false;
      for (int e = s == 0 ? 0 : 1; e < 2 && !ended; e++) {
        if (evals >= a.max_eval) {
          budget = true;
          ended = true;
          break;
        }
        evals++;
        const CertEval w = evaluate(e == 0 ? av : bv, 0.0f);
        if (w.nf) {
          nf = true;
          ended = true;
          break;
        }
        upper = fminf(upper, w.u);
        if constexpr (SELF) upper_s = fminf(upper_s, w.us);
        if (!bracket && (w.u < margin || (SELF && w.us < self_margin))) {  // a witness
          lower = fminf(lower, cert_lo(w.m, a.guard));
          if constexpr (SELF) lower_s = fminf(lower_s, cert_lo(w.ms, a.guard));
          ended = true;
        }
      }
      // ---- 4. the bisection, depth first, left child first; (l, k) is all its state
      int l = 0, k = 0;
      while (!ended) {
        if (evals >= a.max_eval) {
          budget = true;
          break;
        }
        evals++;
        const float hw = cert_half(l);
        const CertEval w = evaluate(fmaf(cert_mid(l, k), dq, av), hw);
        if (w.nf) {
          nf = true;
          break;
        }
        if (l > deepest) deepest = l;
        const float lo = cert_lo(w.m, a.guard);
        const float lo_s = SELF ? cert_lo(w.ms, a.guard) : 0.0f;
        upper = fminf(upper, w.u);
        if constexpr (SELF) upper_s = fminf(upper_s, w.us);
        if (!bracket && (w.u < margin || (SELF && w.us < self_margin))) {  // a witness
          lower = fminf(lower, lo);
          if constexpr (SELF) lower_s = fminf(lower_s, lo_s);
          break;
        }
        bool leaf = cert_leaf(lo, upper, margin, a.tol, bracket);
        if constexpr (SELF) leaf = leaf && cert_leaf(lo_s, upper_s, self_margin, a.tol, bracket);
        if (l >= a.max_depth && !leaf) {
          depth_hit = true;
          leaf = true;
        }
        if (leaf) {
          lower = fminf(lower, lo);
          if constexpr (SELF) lower_s = fminf(lower_s, lo_s);
          if (n_leaves < a.max_leaves && lane == 0) {
            int32_t* const o = leaves + (size_t)n_leaves * 3;
            o[0] = s; o[1] = l; o[2] = k;
          }
          n_leaves++;
          if (cert_next(&l, &k)) {
            finished++;
            break;
          }
        } else {
          l++;
          k *= 2;
        }
      }
    }
    if (budget) spent = true;
    if (nf || budget) lower = lower_s = -INFINITY;
    const int status = certrel_status(nf, budget, depth_hit, lower, upper, margin, SELF, lower_s, upper_s, self_margin);
    if (lane == 0) {
      const size_t o = (size_t)row * (K - 1) + s;
      if (a.seg_lower) a.seg_lower[o] = lower;
      if (a.seg_upper) a.seg_upper[o] = upper;
      if (a.seg_status) a.seg_status[o] = status;
      if constexpr (SELF) {
        if (a.seg_self_lower) a.seg_self_lower[o] = lower_s;
        if (a.seg_self_upper) a.seg_self_upper[o] = upper_s;
      }
    }
    rlower = fminf(rlower, lower);
    rupper = fminf(rupper, upper);
    rlower_s = fminf(rlower_s, lower_s);
    rupper_s = fminf(rupper_s, upper_s);
    if (status > rstatus) rstatus = status;
    if (first < 0 && status != MIR_CERT_CLEAR) first = s;
    av = bv;
  }
  if (lane == 0) {
    if (a.row_lower) a.row_lower[row] = rlower;
    if (a.row_upper) a.row_upper[row] = rupper;
    if constexpr (SELF) {
      if (a.row_self_lower) a.row_self_lower[row] = rlower_s;
      if (a.row_self_upper) a.row_self_upper[row] = rupper_s;
    }
    if (a.row_status) a.row_status[row] = rstatus;
    if (a.row_first) a.row_first[row] = first;
    if (a.stats) {
      int32_t* const st = a.stats + (size_t)row * 4;
      st[0] = evals; st[1] = n_leaves; st[2] = deepest; st[3] = finished;
    }
  }
}

// ---- host
struct CertOut {
  float *seg_lower, *seg_upper, *seg_self_lower, *seg_self_upper;
  int32_t* seg_status;
  float *row_lower, *row_upper, *row_self_lower, *row_self_upper;
  int32_t *row_status, *row_first;
  float* grasp_used;
  int32_t *leaves, *stats;
};
enum CertForm { CERT_SCENE, CERT_SELF, CERT_CARRY };  // the entry point: mir_certify_path (neither query), _self, _carry

int cert_entry(const char* who, CertForm form, MirHandle h, const MirCertQuery* q, const MirPlanQuery* pq, const MirSelfQuery* sq,
               const MirCarryQuery* cq, const float* probes, const int32_t* probe_link, const int32_t* dof_qadr, const int64_t* env_idx,
               int32_t n_rows, const float* qpos_start, const float* grasp, const float* paths, const CertOut& o, void* stream) {
  const auto refuse = [&](int code, const char* what) { return query_error(code, who, what); };
  const CertCall cc{h != nullptr, q, pq, probes, dof_qadr, paths, o.leaves};
  int rc;
  if ((rc = cert_check(cc, refuse)) != MIR_OK) return rc;
  if (form != CERT_SCENE) {
    const CertRelCall rc2{form == CERT_CARRY, sq, cq, grasp, o.grasp_used, o.seg_self_lower, o.seg_self_upper, o.row_self_lower, o.row_self_upper};
    if ((rc = certrel_check(rc2, refuse)) != MIR_OK) return rc;
  }
  const bool self = sq != nullptr, carry = cq != nullptr;
  const PlanCall c = plan_call(who, h, pq, sq, self, cq, carry, probes, probe_link, dof_qadr, env_idx, n_rows, qpos_start, grasp, o.grasp_used, stream);
  CertArgs a;
  memset(&a, 0, sizeof a);
  long long R = 0;
  if ((rc = plan_front(c, false, a.p, R)) != MIR_OK) return rc;
  if ((rc = cert_check_size(q, R, pq->n_dofs, refuse)) != MIR_OK) return rc;
  const size_t fixed = self ? CERT_FIXED_LDS<true, true> : CERT_FIXED_LDS<false, true>;
  if (form != CERT_SCENE && (rc = certrel_check_lds((long long)fixed, a.p.N, a.p.NS, self, refuse)) != MIR_OK) return rc;
  if (R == 0 || (!o.seg_lower && !o.seg_upper && !o.seg_self_lower && !o.seg_self_upper && !o.seg_status && !o.row_lower && !o.row_upper &&
                 !o.row_self_lower && !o.row_self_upper && !o.row_status && !o.row_first && !o.grasp_used && !o.leaves && !o.stats))
    return MIR_OK;
  a.K = q->num_points; a.max_depth = q->max_depth; a.max_eval = q->max_evaluations; a.max_leaves = o.leaves ? q->max_leaves : 0;
  a.bracket = (q->flags & MIR_CERT_BRACKET) ? 1 : 0;
  a.tol = q->tol; a.guard = q->guard;
  a.paths = paths;
  a.seg_lower = o.seg_lower; a.seg_upper = o.seg_upper; a.seg_self_lower = o.seg_self_lower; a.seg_self_upper = o.seg_self_upper;
  a.seg_status = o.seg_status;
  a.row_lower = o.row_lower; a.row_upper = o.row_upper; a.row_self_lower = o.row_self_lower; a.row_self_upper = o.row_self_upper;
  a.row_status = o.row_status; a.row_first = o.row_first;
  a.leaves = o.leaves; a.stats = o.stats;
  if (self) {
    int32_t parent[MIR_MAX_BODY] = {0}, depth[MIR_MAX_BODY] = {0};
    for (int b = 1; b < h->nbody; b++) {
      parent[b] = (int32_t)(a.p.r.body[b] & 0xff);
      depth[b] = (int32_t)((a.p.r.body[b] >> 10) & 31);
    }
    certrel_lca_table(h->nbody, MIR_MAX_BODY, parent, depth, carry ? a.p.carry_body : -1, carry ? a.p.carry_link : -1, a.lca);
  }
  // (carry in the place of self and back: the four instantiations are then emitted in the order this file always had them, <true, true>,
  // <true, false>, <false, true>, <false, false>, and the code object keeps its bytes)
  const auto kernel = pick_self_carry(carry, self, [](auto C, auto S) { return mir_cert_kernel<decltype(S)::value, decltype(C)::value>; });
  // (the speed bounds of certrel_lds_bytes; the sphere list, its last term, is what plan_launch adds)
  return plan_launch(c, kernel, R, a, a.p, self || carry ? (size_t)certrel_lds_bytes(0, a.p.N, a.p.NS, false) : 0);
}

}  // namespace

extern "C" int mir_cert_query_sizeof(void) { return (int)sizeof(MirCertQuery); }

extern "C" int mir_certify_path(MirHandle h, const MirCertQuery* q, const MirPlanQuery* pq, const float* probes, const int32_t* probe_link,
                                const int32_t* dof_qadr, const int64_t* env_idx, int32_t n_rows, const float* qpos_start, const float* paths,
                                float* seg_lower, float* seg_upper, int32_t* seg_status, float* row_lower, float* row_upper, int32_t* row_status,
                                int32_t* row_first, int32_t* leaves, int32_t* stats, void* stream) {
  const CertOut o{seg_lower, seg_upper, nullptr, nullptr, seg_status, row_lower, row_upper, nullptr, nullptr, row_status, row_first, nullptr, leaves, stats};
  return cert_entry("mir_certify_path", CERT_SCENE, h, q, pq, nullptr, nullptr, probes, probe_link, dof_qadr, env_idx, n_rows, qpos_start, nullptr,
                    paths, o, stream);
}

extern "C" int mir_certify_path_self(MirHandle h, const MirCertQuery* q, const MirPlanQuery* pq, const MirSelfQuery* sq, const float* probes,
                                     const int32_t* probe_link, const int32_t* dof_qadr, const int64_t* env_idx, int32_t n_rows,
                                     const float* qpos_start, const float* paths, float* seg_lower, float* seg_upper, float* seg_self_lower,
                                     float* seg_self_upper, int32_t* seg_status, float* row_lower, float* row_upper, float* row_self_lower,
                                     float* row_self_upper, int32_t* row_status, int32_t* row_first, int32_t* leaves, int32_t* stats, void* stream) {
  const CertOut o{seg_lower, seg_upper, seg_self_lower, seg_self_upper, seg_status, row_lower, row_upper, row_self_lower, row_self_upper,
                  row_status, row_first, nullptr, leaves, stats};
  return cert_entry("mir_certify_path_self", CERT_SELF, h, q, pq, sq, nullptr, probes, probe_link, dof_qadr, env_idx, n_rows, qpos_start, nullptr,
                    paths, o, stream);
}

extern "C" int mir_certify_path_carry(MirHandle h, const MirCertQuery* q, const MirPlanQuery* pq, const MirSelfQuery* sq, const MirCarryQuery* cq,
                                      const float* probes, const int32_t* probe_link, const int32_t* dof_qadr, const int64_t* env_idx,
                                      int32_t n_rows, const float* qpos_start, const float* grasp, const float* paths, float* seg_lower,
                                      float* seg_upper, float* seg_self_lower, float* seg_self_upper, int32_t* seg_status, float* row_lower,
                                      float* row_upper, float* row_self_lower, float* row_self_upper, int32_t* row_status, int32_t* row_first,
                                      float* grasp_used, int32_t* leaves, int32_t* stats, void* stream) {
  const CertOut o{seg_lower, seg_upper, seg_self_lower, seg_self_upper, seg_status, row_lower, row_upper, row_self_lower, row_self_upper,
                  row_status, row_first, grasp_used, leaves, stats};
  return cert_entry("mir_certify_path_carry", CERT_CARRY, h, q, pq, sq, cq, probes, probe_link, dof_qadr, env_idx, n_rows, qpos_start, grasp, paths, o,
                    stream);
}
