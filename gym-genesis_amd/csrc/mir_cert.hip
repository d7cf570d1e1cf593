// mir_cert.hip — certified swept clearance of joint paths (mir_certify_path); include/mirigid.h and DESIGN.md, "Certified clearance".
//
// What it serves: "is this trajectory I already have clear?", answered for the whole of every segment, not for samples of it.  For a
// list of envs, one launch brackets the continuous minimum clearance of the sphere model against the static scene on every segment of
// each row's joint-space path: the signed distance is 1-Lipschitz in a sphere's centre, a centre moves no faster along a segment than
// v_i = sum_j |dq_j| rho_ij, so one evaluation at the midpoint of an interval bounds the clearance on all of it, and the interval is
// bisected where that bound does not decide.
//
// Mapping: one workgroup of one wave64 per row, as mir_path_clear_kernel, on the row machinery of mir_plan_row.h (PlanRow<false, false>,
// plan_setup), which is unchanged: the start row, every body's pose, the geom records, and the forward kinematics of the bodies below
// a planned dof (PlanRow::fk).  Lane j < D holds dof j of the segment's ends; lane = body for the chain lengths S and the sums A, B, P
// (parents before children, one round per tree depth, through LDS); lane = probe in chunks of 64 for the speed bounds v_i (LDS, one
// float per probe) and for the evaluation.
//   The evaluation is a reduction of its own beside PlanRow::clearance_at_poses: probe_world and dist_probe_min give d_i, and one pass
//   yields u = min_i d_i and min_i (d_i - hw v_i) with the not-finite ballot of the planner.
//   The bisection is stackless: the node (l, k) and its dyadic successor are two scalars (mir_cert_front.h, which also holds the
//   status order, the recurrences and the host checks, and which the CPU tests build with g++).
// Bounds: every loop is bounded by K, the tree depth (<= 16), max_depth (through the successor) or max_evaluations: the evaluation
//   counter is compared before every evaluation, so no input can keep a wave running.
// Stores: plain dword stores by lane 0 (outputs, leaves) or into LDS.  No atomics, no scratch, no cross-wave barrier.
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
#include "mir_sphere_front.h"  // (brings mir_dist_body.h)

#include "mir_self_body.h"

#include "mir_plan_row.h"

#include "mir_cert_front.h"

namespace {

struct CertArgs {
  PlanArgs p;  // the clearance side, as mir_path_clearance fills it
  int K, max_depth, max_eval, max_leaves, bracket;
  float tol, guard;
  const float* paths;
  float *seg_lower, *seg_upper, *row_lower, *row_upper;
  int32_t *seg_status, *row_status, *row_first, *leaves, *stats;
};
static_assert(sizeof(CertArgs) <= 4096, "kernel arguments");

// what the rule keeps in LDS beside the row's: the ends of the segment per dof, the chains per body, the speed bound per probe
struct CertLds {
  float adq[PLAN_MAX_DOF], amax[PLAN_MAX_DOF];
  float S[MIR_MAX_BODY], A[MIR_MAX_BODY], B[MIR_MAX_BODY], P[MIR_MAX_BODY];
  float v[DIST_MAX_PROBES];
};

// one evaluation: u = min_i d_i, m = min_i (d_i - hw v_i); nf: a probe centre is not finite
struct CertEval {
  float u, m;
  bool nf;
};

__global__ __launch_bounds__(64) void mir_cert_kernel(CertArgs a) {
  __shared__ PlanLds L;
  __shared__ CertLds C;
  const int lane = threadIdx.x, row = blockIdx.x, D = a.p.D, N = a.p.N, K = a.K;
  PlanRow<false, false> r{a.p, L, lane, 0, 0, false, nullptr, SELF_LIST};
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
        const float reach = hw * C.v[probe];  // (a power of two times v: exact)
        u = fminf(u, dist);
        m = fminf(m, dist - reach);
      }
    }
    return CertEval{wave_min(u), wave_min(m), nan != 0ull};
  };

  const float* const path = a.paths + (size_t)row * K * D;
  int32_t* const leaves = a.leaves ? a.leaves + (size_t)row * a.max_leaves * 3 : nullptr;
  const float margin = a.p.margin;
  const bool bracket = a.bracket != 0;
  int evals = 0, n_leaves = 0, deepest = 0, finished = 0, first = -1, rstatus = MIR_CERT_CLEAR;
  bool spent = false;
  float rlower = INFINITY, rupper = INFINITY;
  float av = isd ? path[lane] : 0.0f;
  for (int s = 0; s + 1 < K; s++) {
    const float bv = isd ? path[(size_t)(s + 1) * D + lane] : 0.0f;
    const float dq = bv - av;
    float lower = INFINITY, upper = INFINITY;
    bool nf = r.bad, budget = false, depth_hit = false, done = false;
    if (a.p.ignore) {
      lower = upper = a.p.max_distance;
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
      }
      for (int i = lane; i < N; i += 64) {
        const V3 c = ld3(a.p.r.probes + (size_t)i * 4);
        const int lk = a.p.r.link[i];
        C.v[i] = cert_speed(C.S[lk], sqrtf(c.x * c.x + c.y * c.y + c.z * c.z), C.A[lk], C.B[lk], C.P[lk]);
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
        if (!bracket && w.u < margin) {  // a witness
          lower = fminf(lower, cert_lo(w.u, a.guard));
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
        upper = fminf(upper, w.u);
        if (!bracket && w.u < margin) {  // a witness
          lower = fminf(lower, lo);
          break;
        }
        bool leaf = cert_leaf(lo, upper, margin, a.tol, bracket);
        if (l >= a.max_depth && !leaf) {
          depth_hit = true;
          leaf = true;
        }
        if (leaf) {
          lower = fminf(lower, lo);
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
    if (nf || budget) lower = -INFINITY;
    const int status = cert_status(nf, budget, depth_hit, lower, upper, margin);
    if (lane == 0) {
      const size_t o = (size_t)row * (K - 1) + s;
      if (a.seg_lower) a.seg_lower[o] = lower;
      if (a.seg_upper) a.seg_upper[o] = upper;
      if (a.seg_status) a.seg_status[o] = status;
    }
    rlower = fminf(rlower, lower);
    rupper = fminf(rupper, upper);
    if (status > rstatus) rstatus = status;
    if (first < 0 && status != MIR_CERT_CLEAR) first = s;
    av = bv;
  }
  if (lane == 0) {
    if (a.row_lower) a.row_lower[row] = rlower;
    if (a.row_upper) a.row_upper[row] = rupper;
    if (a.row_status) a.row_status[row] = rstatus;
    if (a.row_first) a.row_first[row] = first;
    if (a.stats) {
      int32_t* const st = a.stats + (size_t)row * 4;
      st[0] = evals; st[1] = n_leaves; st[2] = deepest; st[3] = finished;
    }
  }
}

}  // namespace

extern "C" int mir_cert_query_sizeof(void) { return (int)sizeof(MirCertQuery); }

extern "C" int mir_certify_path(MirHandle h, const MirCertQuery* q, const MirPlanQuery* pq, const float* probes, const int32_t* probe_link,
                                const int32_t* dof_qadr, const int64_t* env_idx, int32_t n_rows, const float* qpos_start, const float* paths,
                                float* seg_lower, float* seg_upper, int32_t* seg_status, float* row_lower, float* row_upper, int32_t* row_status,
                                int32_t* row_first, int32_t* leaves, int32_t* stats, void* stream) {
  const char* const who = "mir_certify_path";
  const auto refuse = [&](int code, const char* what) { return query_error(code, who, what); };
  const CertCall cc{h != nullptr, q, pq, probes, dof_qadr, paths, leaves};
  int rc;
  if ((rc = cert_check(cc, refuse)) != MIR_OK) return rc;
  PlanCall c{};
  c.who = who; c.h = h; c.q = pq; c.stream = stream;
  c.probes = probes; c.probe_link = probe_link; c.dof_qadr = dof_qadr; c.env_idx = env_idx; c.n_rows = n_rows; c.qpos_start = qpos_start;
  CertArgs a;
  memset(&a, 0, sizeof a);
  long long R = 0;
  if ((rc = plan_front(c, false, a.p, R)) != MIR_OK) return rc;
  if ((rc = cert_check_size(q, R, pq->n_dofs, refuse)) != MIR_OK) return rc;
  if (R == 0 || (!seg_lower && !seg_upper && !seg_status && !row_lower && !row_upper && !row_status && !row_first && !leaves && !stats)) return MIR_OK;
  a.K = q->num_points; a.max_depth = q->max_depth; a.max_eval = q->max_evaluations; a.max_leaves = leaves ? q->max_leaves : 0;
  a.bracket = (q->flags & MIR_CERT_BRACKET) ? 1 : 0;
  a.tol = q->tol; a.guard = q->guard;
  a.paths = paths;
  a.seg_lower = seg_lower; a.seg_upper = seg_upper; a.seg_status = seg_status;
  a.row_lower = row_lower; a.row_upper = row_upper; a.row_status = row_status; a.row_first = row_first;
  a.leaves = leaves; a.stats = stats;
  DeviceGuard guard(h->device);  // (the table's allocation, too)
  if ((rc = fill_dist_tab(h, who, a.p.t)) != MIR_OK) return rc;
  return launch_rows<64>(h, mir_cert_kernel, R, stream, a);
}
