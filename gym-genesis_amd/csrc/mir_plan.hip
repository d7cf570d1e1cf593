// mir_plan.hip — batched collision-checked motion planning (mir_plan_path) and the swept clearance of a given trajectory
// (mir_path_clearance); include/mirigid.h, DESIGN.md "Motion planning".
//
// What it serves: for a list of envs, one launch takes each row's arm from a start configuration to a goal configuration through
// configurations whose sphere model (probe spheres that ride on links, as in mir_signed_distance) keeps `margin` from every geom that is
// not skipped: RRT-Connect in the space of the D planned dofs, shortcut smoothing, resampling to W waypoints.  The second entry point
// streams a caller's trajectory through the same configuration check and reports the lowest clearance per segment.
//
// Mapping: one workgroup of one wave64 per row, as mir_dist.hip.  WSYNC() only; nothing travels from lane to lane through global memory.
//   The row's env, the forward kinematics, the probe centres, the sphere-list entries, the wave reductions and the host's row checks and
//   argument filling are the front end shared with mir_dist.hip and mir_self.hip: mir_sphere_front.h.
//   Row set-up.  The row's full start configuration (nq floats) goes to LDS; forward kinematics with lane = body (sphere_poses_fk); the
//   geom records are built ONCE (dist_build_records): the host guarantees that every geom that is tested rides on a body without a
//   planned dof above it.
//   clear(q).  Lane j < D writes planned dof j into the LDS row; the bodies below a planned dof (bit 15 of their word) are recomputed,
//   every other body keeps its pose; the probes in chunks of 64 through dist_probe_min; the wave minimum of (distance - radius).
//   A configuration is a float per lane: lane j holds dof j, lanes >= D hold 0.
//   Trees.  Two trees in dynamic LDS: coordinates [tree][dof][node] (lanes stride over nodes: conflict free) and a 16-bit parent.
// Bounds: every loop is bounded by max_iterations, max_nodes, the 4096 samples of an edge (PLAN_MAX_SUB: n_sub is clamped), the
//   MIR_PLAN_MAX_POLY nodes of a polyline, smooth_passes, num_waypoints or (mir_path_clearance) the K points of the caller's path.  No
//   input can keep a wave running: a configuration or a geom pose that is not finite counts as blocked, a nearest-node index is
//   clamped to the tree.
// Stores: plain dword stores by lanes 0 .. D-1 (or lane 0).  No atomics, no scratch, no cross-wave barrier.
//
// Self-collision (mir_plan_path_self, mir_path_clearance_self): both kernels are templates on SELF; the instantiation without it is the
//   code of mir_plan_path / mir_path_clearance.  With it, clearance_at_poses() also stores every probe's world centre and radius to a
//   sphere list in dynamic LDS (behind the trees), the E extra probes behind the first N included; self_clearance() walks it: lane =
//   probe i in chunks of 64, a loop over j through the list (self_probe_min of mir_self_body.h: a chunk of the list per lane, sphere j
//   to all lanes by v_readlane), the pair filter as one bit of link_mask[link_i], one wave reduction.  s(i, j) is symmetric, so chunk
//   c of the i's meets the j's from chunk c on.  Bounded by N + E; the mask travels in the kernel arguments.
//
// Carried object (mir_plan_path_carry, mir_path_clearance_carry): a further template parameter, CARRY; the four instantiations without
//   it are the code of the four entry points above.  With it, plan_setup() takes the row's grasp transform (the carried body's pose in
//   the attach link's frame: from the start row's forward kinematics, or the caller's row) into seven registers (the same value in every lane), and the
//   partial fk() ends with one more step: lane 0 overwrites the carried body's pose in LDS by link o grasp.  The probes that ride on
//   the carried body then follow the hand through clearance_at_poses() and self_clearance() unchanged.  A grasp that is not finite or
//   has a zero quaternion sets `bad` (and blocks the self test): every clearance of the row is -INFINITY.
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

namespace {

constexpr int PLAN_MAX_DOF = 16;
constexpr int PLAN_MAX_SUB = 4096;  // samples of one edge
constexpr int PLAN_NO_PARENT = 0xffff;

struct PlanArgs {
  SphereRowArgs r;  // (r.qpos_o: the start rows; body words with bit 15: a planned dof on the body's path to the world)
  DistTabPtrs t;
  const float* qpos;  // the scene's state (rows of qst floats, addressed like the public layout)
  int qst, N, D;
  int NS;  // N + E: the probes of the self test (the first N are those of the scene test)
  int W, max_nodes, max_iter, smooth, ignore, K;
  uint32_t seed;
  float resolution, step, margin, max_distance;
  float self_margin, self_max;
  unsigned long long skip;
  const float* goal;  // mir_plan_path: (R, D); mir_path_clearance: paths (R, K, D)
  float* path;
  int32_t* status;
  float* poly;
  int32_t *n_poly, *stats;
  float *seg_min, *row_min;
  float *seg_self_min, *row_self_min;
  int32_t* first_blocked;
  float lo[PLAN_MAX_DOF], hi[PLAN_MAX_DOF];
  int32_t qadr[PLAN_MAX_DOF];
  uint32_t link_mask[MIR_MAX_BODY];  // SELF: bit b of word a: the spheres on body a are tested against those on body b
  // CARRY: the carried body, the link it follows, the grasp rows (R, 7) (nullable: from the start row), the grasp each row used (nullable)
  int carry_body, carry_link;
  const float* grasp;
  float* grasp_used;
};
static_assert(sizeof(PlanArgs) <= 4096, "kernel arguments");

// the fixed part of the LDS (the trees follow in dynamic LDS)
struct PlanLds {
  float xp[MIR_MAX_BODY][4], xq[MIR_MAX_BODY][4];
  float rec[MIR_MAX_GEOM * DIST_REC];
  float qrow[MIR_MAX_Q];
  float qs[PLAN_MAX_DOF];
  float poly[MIR_PLAN_MAX_POLY][PLAN_MAX_DOF];
  float cum[MIR_PLAN_MAX_POLY];
};

// ---- random numbers: u(env, c, j) in [0, 1), keyed by the env index
__device__ __forceinline__ uint32_t plan_mix(uint32_t x) {
  x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
  return x;
}
__device__ __forceinline__ float plan_u(uint32_t seed, uint32_t env, uint32_t c, uint32_t j) {
  const uint32_t x = plan_mix(plan_mix(plan_mix(seed ^ env) ^ c) ^ j);
  return (float)(x >> 8) * 5.9604644775390625e-8f;  // 2^-24
}

// x / y with one refinement of the quotient (x >= 0, y > 0): within an ulp of the exact quotient whatever the division flags of the build
__device__ __forceinline__ float div_refined(float x, float y) {
  const float r = 1.0f / y;
  const float t = x * r;
  return fmaf(fmaf(-t, y, x), r, t);
}

// what a row carries through its launch (wave-uniform but for `lane`)
enum { SELF_LIST = 0, SELF_IGNORED = 1, SELF_BLOCKED = 2 };  // what the last clearance() left for self_clearance()
template <bool SELF, bool CARRY>
struct PlanRow {
  static constexpr bool carry = CARRY;
  const PlanArgs& a;
  PlanLds& L;
  int lane, count, checked;
  bool bad;  // a geom record is not finite (a free body's pose in the row is not): every clearance is -INFINITY
  float* sph;  // SELF: the sphere list, (centre, radius) x NS in dynamic LDS
  int self_state;
  V3 gp;  // CARRY: the grasp transform, the carried body in the attach link's frame (wave-uniform)
  Q4 gq;

  // forward kinematics, lane = body: every body (all) or the bodies below a planned dof
  __device__ __forceinline__ void fk(bool all) {
    sphere_poses_fk(a.r, L.qrow, all, lane, L.xp, L.xq);
    if constexpr (CARRY)
      if (!all) {  // the carried body follows its link: link o grasp (its qpos entry is never read again, never written)
        if (lane == 0) {
          const V3 lp = ld3(L.xp[a.carry_link]);
          const Q4 lq = ld4(L.xq[a.carry_link]);
          st3(L.xp[a.carry_body], lp + qrot(lq, gp));
          st4(L.xq[a.carry_body], qmul(lq, gq));
        }
        WSYNC();
      }
  }

  // the lowest (signed distance - radius) over the probes at the poses in LDS, max_distance when nothing is that near.  A probe centre
  // that is not finite (a NaN or an infinity in the configuration reaches it through the forward kinematics) gives -INFINITY, blocked:
  // left to the comparisons of dist_probe_min such a probe would lose against every geom and count as a miss, which is clear.
  __device__ __forceinline__ float clearance_at_poses() {
    float mn = INFINITY;
    unsigned long long nan = 0ull;
    for (int base = 0; base < a.N; base += 64) {
      const bool valid = base + lane < a.N;
      const int probe = valid ? base + lane : a.N - 1;
      const ProbeWorld p = probe_world(a.r, probe, L.xp, L.xq);
      const DistBest w = dist_probe_min(L.rec, count, a.t.planes, a.t.tris, p.c, p.radius, a.max_distance);
      const bool hit = w.bestk >= 0 && w.best <= a.max_distance;
      const float dist = hit ? w.best : a.max_distance;
      nan |= probe_nonfinite(valid, p.c);
      if (valid) mn = fminf(mn, dist);
      if constexpr (SELF)
        if (valid) sphere_store(sph, probe, p.c, &p.radius);
    }
    if constexpr (SELF) {
      const unsigned long long nan_x = sphere_list_fill(a.r, a.N, a.NS, lane, L.xp, L.xq, sph);  // the extra probes: no scene test
      self_state = (nan | nan_x) != 0ull || (CARRY && bad) ? SELF_BLOCKED : SELF_LIST;
    }
    mn = wave_min(mn);
    return nan != 0ull || bad ? -INFINITY : mn;
  }

  // the self clearance of the configuration the last clearance() evaluated: the lowest s(i, j) over the enabled pairs of the sphere
  // list, capped at self_max; -INFINITY when a probe centre (or the configuration) is not finite
  __device__ __forceinline__ float self_clearance() {
    if (self_state == SELF_IGNORED) return a.self_max;
    if (self_state == SELF_BLOCKED) return -INFINITY;
    WSYNC();  // (the list is written)
    float mn = a.self_max;
    for (int base = 0; base < a.NS; base += 64) {
      const bool valid = base + lane < a.NS;
      const int i = valid ? base + lane : a.NS - 1;
      const SelfBest w = self_probe_min<false>(sph, a.r.link, a.NS, base, i, valid ? a.link_mask[a.r.link[i]] : 0u, lane);
      mn = fminf(mn, w.best);
    }
    mn = wave_min(mn);
    WSYNC();  // (before the next configuration overwrites the list)
    return mn;
  }

  // clear(q): the clearance of configuration q (lane j: planned dof j)
  __device__ __forceinline__ float clearance(float q) {
    if (a.ignore) {
      self_state = SELF_IGNORED;
      return a.max_distance;
    }
    if (__ballot(lane < a.D && nonfinite(q)) != 0ull) {  // (not a configuration: blocked, and kept out of the row)
      checked++;
      self_state = SELF_BLOCKED;
      return -INFINITY;
    }
    if (lane < a.D) L.qrow[a.qadr[lane]] = q;
    WSYNC();
    fk(false);
    checked++;
    return clearance_at_poses();
  }

  // samples of the edge a -> b: n_sub = max(1, ceil(max_j |b_j - a_j| / resolution)), at most PLAN_MAX_SUB
  __device__ __forceinline__ int n_sub(float diff) const {
    const float m = wave_max(lane < a.D ? fabsf(diff) : 0.0f);
    return __builtin_amdgcn_readfirstlane((int)fminf(fmaxf(ceilf(div_refined(m, a.resolution)), 1.0f), (float)PLAN_MAX_SUB));
  }
  __device__ __forceinline__ static float sample(float av, float bv, float diff, int i, int n) {
    return i == n ? bv : av + div_refined((float)i, (float)n) * diff;  // (the last sample is b's bits)
  }

  // clear(q): the scene test, then (SELF, and only when the scene test holds) the self test
  __device__ __forceinline__ bool clear(float q) {
    if (!(clearance(q) >= a.margin)) return false;
    if constexpr (SELF)
      if (!(self_clearance() >= a.self_margin)) return false;
    return true;
  }

  // edge(a, b): the samples i = 1 .. n_sub in order; the first blocked one ends the check
  __device__ __forceinline__ bool edge(float av, float bv) {
    const float diff = bv - av;
    const int n = n_sub(diff);
    for (int i = 1; i <= n; i++)
      if (!clear(sample(av, bv, diff, i, n))) return false;
    return true;
  }

  // sum_j v_j^2 over the planned dofs, j ascending, the same value in every lane
  __device__ __forceinline__ float norm2(float v) {
    if (lane < a.D) L.qs[lane] = v;
    WSYNC();
    float acc = 0.0f;
    for (int j = 0; j < a.D; j++) {
      const float e = L.qs[j];
      acc = acc + e * e;
    }
    WSYNC();
    return acc;
  }
};

// ---- row set-up shared by the two kernels: the start row, every body's pose, the geom records
template <class Row>
__device__ __forceinline__ void plan_setup(Row& r, int row, int env) {
  const PlanArgs& a = r.a;
  const float* const src = a.r.qpos_o ? a.r.qpos_o + (size_t)row * a.r.nq : a.qpos + (size_t)env * a.qst;
  for (int i = r.lane; i < a.r.nq; i += 64) r.L.qrow[i] = src[i];
  WSYNC();
  r.fk(true);
  r.count = a.ignore ? 0 : __builtin_amdgcn_readfirstlane(dist_build_records(a.t.tab, a.skip, r.lane, r.L.xp, r.L.xq, r.L.rec));
  bool badrec = false;
  if (r.lane < r.count)
    for (int k = 5; k <= 16; k++) badrec = badrec || nonfinite(r.L.rec[r.lane * DIST_REC + k]);  // the geom's centre and axes
  r.bad = __ballot(badrec) != 0ull;
  if constexpr (Row::carry) {  // the grasp transform of the row, the same value in every lane (seven vector registers: the scalar file is full)
    V3 p;
    Q4 q;
    bool zero = false;
    if (a.grasp) {
      const float* const g = a.grasp + (size_t)row * 7;
      const Q4 raw = ld4(g + 3);
      p = ld3(g);
      zero = raw.w * raw.w + raw.x * raw.x + raw.y * raw.y + raw.z * raw.z < 1e-30f;  // (what qnormalize turns into the identity)
      q = qnormalize(raw);
    } else {
      const V3 lp = ld3(r.L.xp[a.carry_link]);
      const Q4 lc = qconj(ld4(r.L.xq[a.carry_link]));
      p = qrot(lc, ld3(r.L.xp[a.carry_body]) - lp);
      q = qmul(lc, ld4(r.L.xq[a.carry_body]));
    }
    r.gp = p;
    r.gq = q;
    const bool nf = nonfinite(r.gp.x) || nonfinite(r.gp.y) || nonfinite(r.gp.z) || nonfinite(r.gq.w) || nonfinite(r.gq.x) || nonfinite(r.gq.y) ||
                    nonfinite(r.gq.z);
    r.bad = r.bad || __ballot(nf || zero) != 0ull;
    if (a.grasp_used && r.lane == 0) {
      float* const o = a.grasp_used + (size_t)row * 7;
      st3(o, r.gp);
      st4(o + 3, r.gq);
    }
  }
}

extern __shared__ float plan_dyn[];

template <bool SELF, bool CARRY>
__global__ __launch_bounds__(64) void mir_plan_kernel(PlanArgs a) {
  __shared__ PlanLds L;
  const int lane = threadIdx.x, row = blockIdx.x, D = a.D, MN = a.max_nodes;
  const int env = sphere_row_env(a.r, row);
  float* const tree = plan_dyn;                                                        // [2][D][MN]
  uint16_t* const parent = reinterpret_cast<uint16_t*>(plan_dyn + (size_t)2 * D * MN);  // [2][MN]
  PlanRow<SELF, CARRY> r{a, L, lane, 0, 0, false, plan_dyn + (size_t)(2 * D + 1) * MN, SELF_LIST};  // (2 MN 16-bit parents are MN floats)
  plan_setup(r, row, env);
  const bool isd = lane < D;
  const int dj = isd ? lane : 0;
  const float lo = a.lo[dj], hi = a.hi[dj];
  const float sv = isd ? L.qrow[a.qadr[dj]] : 0.0f;
  const float gv = isd ? a.goal[(size_t)row * D + dj] : 0.0f;
  WSYNC();

  auto node = [&](int t, int n) { return isd ? tree[((size_t)t * D + dj) * MN + n] : 0.0f; };
  auto add = [&](int t, int n, float v, int par) {
    if (isd) tree[((size_t)t * D + dj) * MN + n] = v;
    if (lane == 0) parent[t * MN + n] = (uint16_t)par;
    WSYNC();
  };
  // nearest node of tree t (cnt nodes) to q: squared L2 distance over the planned dofs, j ascending; the lower index wins a tie
  auto nearest = [&](int t, int cnt, float q, float& d2) {
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
  };

  int status = MIR_PLAN_OK, iterations = 0, na = 1, nb = 1, npoly = 1;
  const bool outside = isd && !(gv >= lo && gv <= hi);
  if (__ballot(outside) != 0ull) status = MIR_PLAN_GOAL_OUT_OF_LIMITS;
  else if (!(r.clearance(sv) >= a.margin)) status = MIR_PLAN_START_IN_COLLISION;
  else if (SELF && !(r.self_clearance() >= a.self_margin)) status = MIR_PLAN_START_IN_SELF_COLLISION;
  else if (!(r.clearance(gv) >= a.margin)) status = MIR_PLAN_GOAL_IN_COLLISION;
  else if (SELF && !(r.self_clearance() >= a.self_margin)) status = MIR_PLAN_GOAL_IN_SELF_COLLISION;
  else if (r.edge(sv, gv)) {
    if (isd) { L.poly[0][lane] = sv; L.poly[1][lane] = gv; }
    npoly = 2;
  } else {
    add(0, 0, sv, PLAN_NO_PARENT);
    add(1, 0, gv, PLAN_NO_PARENT);
    status = MIR_PLAN_ITERATION_LIMIT;
    for (int it = 0; it < a.max_iter; it++) {
      iterations = it + 1;
      const int t = it & 1, o = t ^ 1;
      int ct = t ? nb : na, co = t ? na : nb;
      const float qr = isd ? lo + plan_u(a.seed, (uint32_t)env, (uint32_t)it, (uint32_t)dj) * (hi - lo) : 0.0f;
      float d2;
      const int near = nearest(t, ct, qr, d2);
      const float nv = node(t, near);
      const float qn = nv + fminf(1.0f, a.step / sqrtf(d2)) * (qr - nv);
      if (!r.edge(nv, qn)) continue;
      if (ct >= MN) { status = MIR_PLAN_NODE_LIMIT; break; }
      add(t, ct, qn, near);
      const int inew = ct++;
      // connect: from the other tree's nearest node towards q_new, at most `step` at a time
      int ci = nearest(o, co, qn, d2);
      float cv = node(o, ci);
      bool met = false, full = false;
      for (int k = 0; k < MN; k++) {  // (every pass adds a node or leaves)
        const float diff = qn - cv;
        const float d = sqrtf(r.norm2(diff));
        const bool last = d <= a.step;
        const float tv = last ? qn : cv + (a.step / d) * diff;
        if (!r.edge(cv, tv)) break;
        if (co >= MN) { full = true; break; }
        add(o, co, tv, ci);
        ci = co++;
        cv = tv;
        if (last) { met = true; break; }
      }
      na = t ? co : ct;
      nb = t ? ct : co;
      if (full) { status = MIR_PLAN_NODE_LIMIT; break; }
      if (!met) continue;
      // extract: the parents of both trees into one polyline, start first
      const int ia = t ? ci : inew, ib = t ? inew : ci;
      int la = 0, lb = 0;
      for (int n = ia; n != PLAN_NO_PARENT && la <= MN; n = __builtin_amdgcn_readfirstlane((int)parent[n])) la++;
      for (int n = ib; n != PLAN_NO_PARENT && lb <= MN; n = __builtin_amdgcn_readfirstlane((int)parent[MN + n])) lb++;
      if (la + lb - 1 > MIR_PLAN_MAX_POLY) { status = MIR_PLAN_PATH_TOO_LONG; break; }
      int n = ia;
      for (int p = la - 1; p >= 0; p--) {
        if (isd) L.poly[p][lane] = node(0, n);
        n = __builtin_amdgcn_readfirstlane((int)parent[n]);
      }
      n = __builtin_amdgcn_readfirstlane((int)parent[MN + ib]);  // (the meeting node is in both trees: once)
      for (int p = la; p < la + lb - 1; p++) {
        if (isd) L.poly[p][lane] = node(1, n);
        n = __builtin_amdgcn_readfirstlane((int)parent[MN + n]);
      }
      npoly = la + lb - 1;
      status = MIR_PLAN_OK;
      break;
    }
  }
  if (status != MIR_PLAN_OK) {  // the arm stays put: the start W times, a polyline of one node
    if (isd) L.poly[0][lane] = sv;
    npoly = 1;
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
}

// the swept check on its own: every sample of the edge rule on every segment of the caller's path, no early exit
template <bool SELF, bool CARRY>
__global__ __launch_bounds__(64) void mir_path_clear_kernel(PlanArgs a) {
  __shared__ PlanLds L;
  const int lane = threadIdx.x, row = blockIdx.x, D = a.D;
  PlanRow<SELF, CARRY> r{a, L, lane, 0, 0, false, plan_dyn, SELF_LIST};
  plan_setup(r, row, sphere_row_env(a.r, row));
  const bool isd = lane < D;
  const float* const p = a.goal + (size_t)row * a.K * D;
  float rmin = INFINITY, rself = INFINITY;
  int first = -1;
  float av = isd ? p[lane] : 0.0f;
  for (int k = 0; k + 1 < a.K; k++) {
    const float bv = isd ? p[(size_t)(k + 1) * D + lane] : 0.0f;
    float smin = k == 0 ? r.clearance(av) : INFINITY;  // (a segment's first point counts only for segment 0)
    float sself = INFINITY;
    if constexpr (SELF)
      if (k == 0) sself = r.self_clearance();
    const float diff = bv - av;
    const int n = r.n_sub(diff);
    for (int i = 1; i <= n; i++) {
      smin = fminf(smin, r.clearance(PlanRow<SELF, CARRY>::sample(av, bv, diff, i, n)));
      if constexpr (SELF) sself = fminf(sself, r.self_clearance());
    }
    if (a.seg_min && lane == 0) a.seg_min[(size_t)row * (a.K - 1) + k] = smin;
    rmin = fminf(rmin, smin);
    bool blocked = smin < a.margin;
    if constexpr (SELF) {
      if (a.seg_self_min && lane == 0) a.seg_self_min[(size_t)row * (a.K - 1) + k] = sself;
      rself = fminf(rself, sself);
      blocked = blocked || sself < a.self_margin;
    }
    if (first < 0 && blocked) first = k;
    av = bv;
  }
  if (lane == 0) {
    if (a.row_min) a.row_min[row] = rmin;
    if constexpr (SELF)
      if (a.row_self_min) a.row_self_min[row] = rself;
    if (a.first_blocked) a.first_blocked[row] = first;
  }
}

// ---- host.  A call as its entry point hands it over, by name
struct PlanCall {
  const char* who;
  MirHandle h;
  const MirPlanQuery* q;
  const MirSelfQuery* sq;   // read where `self` is set: the two *_self entry points always (a null sq is their refusal), the two
  bool self;                // *_carry where sq is not null (a null sq is "no self test")
  const MirCarryQuery* cq;  // read where `carry` is set: the two *_carry entry points
  bool carry;
  const float *probes, *qpos_start, *grasp;  // (grasp, grasp_used: carry only, nullable)
  const int32_t *probe_link, *dof_qadr;
  const int64_t* env_idx;
  int32_t n_rows;
  float* grasp_used;
  void* stream;
};

// what the two kinds of entry point share.  Fills `a` but for the outputs and the table; every refusal launches nothing.  The self
// query is checked here, the carry query too (behind the refusals of the entry point it extends).
int plan_front(const PlanCall& c, bool planner, PlanArgs& a, long long& R) {
  const MirHandle h = c.h;
  const MirPlanQuery* const q = c.q;
  const char* const who = c.who;
  const bool self = c.self, carry = c.carry;
  int rc;
  if (!h || !q || !c.probes || !c.dof_qadr || (carry && !c.cq)) return query_error(MIR_E_INVALID, who, "null argument");
  if (self && (rc = self_query_check(h, c.sq, who)) != MIR_OK) return rc;
  if (q->struct_size != (int32_t)sizeof(MirPlanQuery)) return query_error(MIR_E_INVALID, who, "struct_size is not sizeof(MirPlanQuery)");
  if (q->n_probes < 1) return query_error(MIR_E_INVALID, who, "n_probes < 1");
  if (q->n_dofs < 1 || q->n_dofs > PLAN_MAX_DOF) return query_error(MIR_E_INVALID, who, "n_dofs outside 1 .. 16");
  if (!std::isfinite(q->resolution) || !(q->resolution > 0.0f)) return query_error(MIR_E_INVALID, who, "resolution must be finite and > 0");
  if (!std::isfinite(q->margin) || !(q->margin >= 0.0f)) return query_error(MIR_E_INVALID, who, "margin must be finite and >= 0");
  if (!std::isfinite(q->max_distance) || !(q->max_distance > q->margin)) return query_error(MIR_E_INVALID, who, "max_distance must be finite and > margin");
  if (q->flags & ~(uint32_t)MIR_PLAN_IGNORE_COLLISION) return query_error(MIR_E_INVALID, who, "unknown flag bit");
  if (h->ngeom < 64 && (q->skip_geoms >> h->ngeom)) return query_error(MIR_E_INVALID, who, "skip_geoms names a geom at or above ngeom");
  if (planner) {
    if (q->num_waypoints < 2) return query_error(MIR_E_INVALID, who, "num_waypoints < 2");
    if (q->max_nodes < 2) return query_error(MIR_E_INVALID, who, "max_nodes < 2");
    if (q->max_iterations < 0 || q->smooth_passes < 0) return query_error(MIR_E_INVALID, who, "negative max_iterations or smooth_passes");
    if (!std::isfinite(q->step) || !(q->step > 0.0f)) return query_error(MIR_E_INVALID, who, "step must be finite and > 0");
  }
  if ((rc = check_rows(h, c.env_idx, c.n_rows, who, R)) != MIR_OK) return rc;
  const int N = q->n_probes, D = q->n_dofs;
  const long long NS = (long long)N + (self ? c.sq->n_extra : 0);
  if ((rc = check_probe_count(NS, R, false, who)) != MIR_OK) return rc;
  memset(&a, 0, sizeof a);
  const auto refuse = [&](int code, const char* what) { return query_error(code, who, what); };
  if ((rc = pack_probe_links(c.probe_link, (int)NS, h->nbody, a.r.link, refuse)) != MIR_OK) return rc;
  const ModelView mv(h);
  // the planned dofs: the scalar joint behind each qpos address, its limits
  bool planned[MIR_MAX_BODY] = {false};
  for (int j = 0; j < D; j++) {
    int body = -1;
    for (int b = 1; b < h->nbody; b++) {
      const int jt = mv.jtype(b);
      if ((jt == MIR_JNT_REVOLUTE || jt == MIR_JNT_PRISMATIC) && mv.qadr(b) == c.dof_qadr[j]) body = b;
    }
    if (body < 0) return query_error(MIR_E_INVALID, who, "dof_qadr is not the qpos address of a revolute or prismatic joint");
    if (planned[body]) return query_error(MIR_E_INVALID, who, "dof_qadr names a joint twice");
    planned[body] = true;
    double lo, hi;
    int limited;
    mv.limits(body, lo, hi, limited);
    if (!limited || !(hi > lo)) return query_error(MIR_E_INVALID, who, "a planned dof has no limits");
    if ((hi - lo) / (double)q->resolution > (double)PLAN_MAX_SUB) return query_error(MIR_E_INVALID, who, "a planned dof's range exceeds 4096 x resolution");
    a.lo[j] = (float)lo; a.hi[j] = (float)hi; a.qadr[j] = c.dof_qadr[j];
  }
  if ((rc = build_body_words(mv, h->nbody, true, planned, a.r.body, a.r.depth_max, refuse)) != MIR_OK) return rc;
  a.ignore = (q->flags & MIR_PLAN_IGNORE_COLLISION) ? 1 : 0;
  if (!a.ignore)
    for (int g = 0; g < h->ngeom; g++) {
      const int b = h->kernel == 16 ? h->hm.g_body[g] : h->hm64.g_body[g];
      if (!((q->skip_geoms >> g) & 1ull) && b >= 0 && b < h->nbody && ((a.r.body[b] >> 15) & 1u))
        return query_error(MIR_E_INVALID, who, "a geom that is not skipped rides on a planned joint (a moving obstacle is out of scope: skip it)");
    }
  if (carry) {
    if (c.cq->struct_size != (int32_t)sizeof(MirCarryQuery)) return query_error(MIR_E_INVALID, who, "struct_size is not sizeof(MirCarryQuery)");
    if (c.cq->flags) return query_error(MIR_E_INVALID, who, "unknown flag bit in MirCarryQuery");
    const int cb = c.cq->body, cl = c.cq->link;
    if (cb < 1 || cb >= h->nbody || mv.jtype(cb) != MIR_JNT_FREE) return query_error(MIR_E_INVALID, who, "the carried body is not a free-joint body");
    for (int b = 1; b < h->nbody; b++)
      if (mv.parent(b) == cb) return query_error(MIR_E_INVALID, who, "the carried body has a child body");
    if (cl < 0 || cl >= h->nbody) return query_error(MIR_E_INVALID, who, "the attach link is outside 0 .. nbody - 1");
    if (cl == cb) return query_error(MIR_E_INVALID, who, "the attach link is the carried body");
    if (!a.ignore)
      for (int g = 0; g < h->ngeom; g++) {
        const int b = h->kernel == 16 ? h->hm.g_body[g] : h->hm64.g_body[g];
        if (b == cb && !((q->skip_geoms >> g) & 1ull))
          return query_error(MIR_E_INVALID, who, "a geom of the carried body is not skipped (it rides on the planned joints: skip it)");
      }
    a.carry_body = cb; a.carry_link = cl;
  }
  if (planner) {
    const size_t lds = sizeof(PlanLds) + (size_t)2 * (size_t)q->max_nodes * (4 * (size_t)D + 2) + (self ? 16 * (size_t)NS : 0);
    if (q->max_nodes > 0xfffe || lds > 65536)
      return query_error(MIR_E_CAPACITY, who, self ? "the two trees and the sphere list do not fit 64 KB of LDS (max_nodes x n_dofs, n_probes + n_extra)"
                                                    : "the two trees do not fit 64 KB of LDS (max_nodes x n_dofs)");
  }
  a.NS = (int)NS;
  if (self) {
    a.self_margin = c.sq->self_margin; a.self_max = c.sq->max_distance;
    memcpy(a.link_mask, c.sq->link_mask, sizeof a.link_mask);
  }
  fill_sphere_rows(mv, c.env_idx, R, c.qpos_start, c.probes, a.r);
  a.qpos = h->qpos; a.qst = h->pt.qst; a.N = N; a.D = D;
  a.resolution = q->resolution; a.margin = q->margin; a.max_distance = q->max_distance; a.skip = q->skip_geoms;
  a.grasp = c.grasp; a.grasp_used = c.grasp_used;
  return MIR_OK;
}

// the instantiation of either kernel that serves a call
using PlanKernel = void (*)(PlanArgs);
PlanKernel plan_kernel(bool self, bool carry) {
  if (carry) return self ? mir_plan_kernel<true, true> : mir_plan_kernel<false, true>;
  return self ? mir_plan_kernel<true, false> : mir_plan_kernel<false, false>;
}
PlanKernel path_clear_kernel(bool self, bool carry) {
  if (carry) return self ? mir_path_clear_kernel<true, true> : mir_path_clear_kernel<false, true>;
  return self ? mir_path_clear_kernel<true, false> : mir_path_clear_kernel<false, false>;
}

int plan_entry(const PlanCall& c, const float* qpos_goal, float* path, int32_t* status, float* poly, int32_t* n_poly, int32_t* stats) {
  if (!qpos_goal || !path || !status) return query_error(MIR_E_INVALID, c.who, "null argument");
  PlanArgs a;
  long long R = 0;
  int rc = plan_front(c, true, a, R);
  if (rc != MIR_OK || R == 0) return rc;
  a.W = c.q->num_waypoints; a.max_nodes = c.q->max_nodes; a.max_iter = c.q->max_iterations; a.smooth = c.q->smooth_passes; a.seed = c.q->seed;
  a.step = c.q->step; a.goal = qpos_goal; a.path = path; a.status = status; a.poly = poly; a.n_poly = n_poly; a.stats = stats;
  const size_t trees = (size_t)2 * (size_t)a.max_nodes * (4 * (size_t)a.D + 2);
  DeviceGuard guard(c.h->device);  // (the table's allocation, too)
  if ((rc = fill_dist_tab(c.h, c.who, a.t)) != MIR_OK) return rc;
  return launch_rows<64>(c.h, plan_kernel(c.self, c.carry), R, c.stream, a, trees + (c.self ? 16 * (size_t)a.NS : 0));
}

int path_clear_entry(const PlanCall& c, const float* paths, int32_t K, float* seg_min, float* seg_self_min, float* row_min, float* row_self_min,
                     int32_t* row_first_blocked) {
  if (!paths) return query_error(MIR_E_INVALID, c.who, "null argument");
  if (K < 2) return query_error(MIR_E_INVALID, c.who, "K < 2");
  if (!c.self && (seg_self_min || row_self_min)) return query_error(MIR_E_INVALID, c.who, "seg_self_min / row_self_min without a MirSelfQuery");
  PlanArgs a;
  long long R = 0;
  int rc = plan_front(c, false, a, R);
  if (rc != MIR_OK || R == 0 || (!seg_min && !seg_self_min && !row_min && !row_self_min && !row_first_blocked && !c.grasp_used)) return rc;
  a.K = K; a.goal = paths; a.seg_min = seg_min; a.row_min = row_min; a.first_blocked = row_first_blocked;
  a.seg_self_min = seg_self_min; a.row_self_min = row_self_min;
  DeviceGuard guard(c.h->device);  // (the table's allocation, too)
  if ((rc = fill_dist_tab(c.h, c.who, a.t)) != MIR_OK) return rc;
  return launch_rows<64>(c.h, path_clear_kernel(c.self, c.carry), R, c.stream, a, c.self ? 16 * (size_t)a.NS : 0);
}

}  // namespace

extern "C" int mir_plan_query_sizeof(void) { return (int)sizeof(MirPlanQuery); }
extern "C" int mir_self_query_sizeof(void) { return (int)sizeof(MirSelfQuery); }

extern "C" int mir_plan_path(MirHandle h, const MirPlanQuery* q, const float* probes, const int32_t* probe_link, const int32_t* dof_qadr,
                             const int64_t* env_idx, int32_t n_rows, const float* qpos_start, const float* qpos_goal, float* path,
                             int32_t* status, float* poly, int32_t* n_poly, int32_t* stats, void* stream) {
  PlanCall c{};
  c.who = "mir_plan_path"; c.h = h; c.q = q; c.stream = stream;
  c.probes = probes; c.probe_link = probe_link; c.dof_qadr = dof_qadr; c.env_idx = env_idx; c.n_rows = n_rows; c.qpos_start = qpos_start;
  return plan_entry(c, qpos_goal, path, status, poly, n_poly, stats);
}

extern "C" int mir_plan_path_self(MirHandle h, const MirPlanQuery* q, const MirSelfQuery* sq, const float* probes, const int32_t* probe_link,
                                  const int32_t* dof_qadr, const int64_t* env_idx, int32_t n_rows, const float* qpos_start, const float* qpos_goal,
                                  float* path, int32_t* status, float* poly, int32_t* n_poly, int32_t* stats, void* stream) {
  PlanCall c{};
  c.who = "mir_plan_path_self"; c.h = h; c.q = q; c.sq = sq; c.self = true; c.stream = stream;
  c.probes = probes; c.probe_link = probe_link; c.dof_qadr = dof_qadr; c.env_idx = env_idx; c.n_rows = n_rows; c.qpos_start = qpos_start;
  return plan_entry(c, qpos_goal, path, status, poly, n_poly, stats);
}

extern "C" int mir_path_clearance(MirHandle h, const MirPlanQuery* q, const float* probes, const int32_t* probe_link, const int32_t* dof_qadr,
                                  const int64_t* env_idx, int32_t n_rows, const float* qpos_start, const float* paths, int32_t K,
                                  float* seg_min, float* row_min, int32_t* row_first_blocked, void* stream) {
  PlanCall c{};
  c.who = "mir_path_clearance"; c.h = h; c.q = q; c.stream = stream;
  c.probes = probes; c.probe_link = probe_link; c.dof_qadr = dof_qadr; c.env_idx = env_idx; c.n_rows = n_rows; c.qpos_start = qpos_start;
  return path_clear_entry(c, paths, K, seg_min, /*seg_self_min*/ nullptr, row_min, /*row_self_min*/ nullptr, row_first_blocked);
}

extern "C" int mir_path_clearance_self(MirHandle h, const MirPlanQuery* q, const MirSelfQuery* sq, const float* probes, const int32_t* probe_link,
                                       const int32_t* dof_qadr, const int64_t* env_idx, int32_t n_rows, const float* qpos_start,
                                       const float* paths, int32_t K, float* seg_min, float* seg_self_min, float* row_min, float* row_self_min,
                                       int32_t* row_first_blocked, void* stream) {
  PlanCall c{};
  c.who = "mir_path_clearance_self"; c.h = h; c.q = q; c.sq = sq; c.self = true; c.stream = stream;
  c.probes = probes; c.probe_link = probe_link; c.dof_qadr = dof_qadr; c.env_idx = env_idx; c.n_rows = n_rows; c.qpos_start = qpos_start;
  return path_clear_entry(c, paths, K, seg_min, seg_self_min, row_min, row_self_min, row_first_blocked);
}

extern "C" int mir_carry_query_sizeof(void) { return (int)sizeof(MirCarryQuery); }

extern "C" int mir_plan_path_carry(MirHandle h, const MirPlanQuery* q, const MirSelfQuery* sq, const MirCarryQuery* cq, const float* probes,
                                   const int32_t* probe_link, const int32_t* dof_qadr, const int64_t* env_idx, int32_t n_rows, const float* qpos_start,
                                   const float* grasp, const float* qpos_goal, float* path, int32_t* status, float* poly, int32_t* n_poly,
                                   int32_t* stats, float* grasp_used, void* stream) {
  PlanCall c{};
  c.who = "mir_plan_path_carry"; c.h = h; c.q = q; c.sq = sq; c.self = sq != nullptr; c.cq = cq; c.carry = true; c.stream = stream;
  c.grasp = grasp; c.grasp_used = grasp_used;
  c.probes = probes; c.probe_link = probe_link; c.dof_qadr = dof_qadr; c.env_idx = env_idx; c.n_rows = n_rows; c.qpos_start = qpos_start;
  return plan_entry(c, qpos_goal, path, status, poly, n_poly, stats);
}

extern "C" int mir_path_clearance_carry(MirHandle h, const MirPlanQuery* q, const MirSelfQuery* sq, const MirCarryQuery* cq, const float* probes,
                                        const int32_t* probe_link, const int32_t* dof_qadr, const int64_t* env_idx, int32_t n_rows,
                                        const float* qpos_start, const float* grasp, const float* paths, int32_t K, float* seg_min, float* seg_self_min,
                                        float* row_min, float* row_self_min, int32_t* row_first_blocked, float* grasp_used, void* stream) {
  PlanCall c{};
  c.who = "mir_path_clearance_carry"; c.h = h; c.q = q; c.sq = sq; c.self = sq != nullptr; c.cq = cq; c.carry = true; c.stream = stream;
  c.grasp = grasp; c.grasp_used = grasp_used;
  c.probes = probes; c.probe_link = probe_link; c.dof_qadr = dof_qadr; c.env_idx = env_idx; c.n_rows = n_rows; c.qpos_start = qpos_start;
  return path_clear_entry(c, paths, K, seg_min, seg_self_min, row_min, row_self_min, row_first_blocked);
}
