// mir_plan_row.h — the row machinery of the planner, shared by mir_plan.hip (mir_plan_path, mir_path_clearance and their _self / _carry
// forms), mir_cart.hip, mir_blend.hip, mir_opt.hip and mir_cert.hip: the kernel arguments and the fixed LDS of a row, the refined division,
// PlanRow<SELF, CARRY> with clear(q) and edge(a, b), the row set-up, and on the host what every entry point shares: the call description
// and its filling (PlanCall, plan_call), the checks and the argument filling (plan_front), the choice of the instantiation
// (pick_self_carry) and the launch (plan_launch).  mir_plan.hip's header comment says what each part does.  Needs mir_dev.h with G = 16,
// mir_query.h, mir_sphere_front.h and mir_self_body.h in front of it.  Inside no namespace.
#pragma once

#include <type_traits>

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

// random numbers of the planner: u(env, c, j) in [0, 1), keyed by the env index (mir_plan.hip, mir_goal.hip)
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
constexpr size_t SELF_SPHERE_BYTES = 16;  // an entry of the sphere list of the self test: (centre, radius)
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

// the call of an entry point from the arguments every one of them receives (grasp, grasp_used: null but for the carry forms)
PlanCall plan_call(const char* who, MirHandle h, const MirPlanQuery* pq, const MirSelfQuery* sq, bool self, const MirCarryQuery* cq, bool carry,
                   const float* probes, const int32_t* probe_link, const int32_t* dof_qadr, const int64_t* env_idx, int32_t n_rows,
                   const float* qpos_start, const float* grasp, float* grasp_used, void* stream) {
  PlanCall c{};
  c.who = who; c.h = h; c.q = pq; c.sq = sq; c.self = self; c.cq = cq; c.carry = carry; c.stream = stream;
  c.grasp = grasp; c.grasp_used = grasp_used;
  c.probes = probes; c.probe_link = probe_link; c.dof_qadr = dof_qadr; c.env_idx = env_idx; c.n_rows = n_rows; c.qpos_start = qpos_start;
  return c;
}

// the <SELF, CARRY> instantiation that serves a call: `kernel` names the template,
//   [](auto S, auto C) { return mir_plan_kernel<decltype(S)::value, decltype(C)::value>; }
template <class Kernel>
auto pick_self_carry(bool self, bool carry, Kernel kernel) {
  using T = std::true_type;
  using F = std::false_type;
  if (carry) return self ? kernel(T{}, T{}) : kernel(F{}, T{});
  return self ? kernel(T{}, F{}) : kernel(F{}, F{});
}

// the launch every entry point ends with: the distance table into `p` (the PlanArgs inside `a`), one wave64 per row, the caller's
// dynamic LDS with the sphere list of the self test behind it
template <class Args>
int plan_launch(const PlanCall& c, void (*kernel)(Args), long long R, Args& a, PlanArgs& p, size_t lds) {
  DeviceGuard guard(c.h->device);  // (the table's allocation, too)
  const int rc = fill_dist_tab(c.h, c.who, p.t);
  if (rc != MIR_OK) return rc;
  return launch_rows<64>(c.h, kernel, R, c.stream, a, lds + (c.self ? SELF_SPHERE_BYTES * (size_t)p.NS : 0));
}

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
    const size_t lds = sizeof(PlanLds) + (size_t)2 * (size_t)q->max_nodes * (4 * (size_t)D + 2) + (self ? SELF_SPHERE_BYTES * (size_t)NS : 0);
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

}  // namespace
