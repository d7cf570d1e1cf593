// mir_sphere_front.h — the front end the three sphere-model kernels share (mir_dist.hip: mir_signed_distance; mir_self.hip:
// mir_self_distance; mir_plan.hip: mir_plan_path, mir_path_clearance and their _self / _carry forms).  One wave64 serves one row.
//   host:   the probe links as a byte each and the body words of the forward kinematics (plain C++ on a model view given as a template
//           parameter: tests/sphere_front_host.cpp builds them with g++ and a fake model); the row checks, the rows part of the kernel
//           arguments with its filler (SphereRowArgs), the pointers into the geometry table;
//   device: the env of a row, the body poses in LDS from the pose cache or by forward kinematics from a qpos row, the world centre of
//           a probe with its not-finite ballot, the sphere list, the wave reductions.
// All but the first two need mir_dev.h with G = 16 and mir_query.h in front, and bring mir_dist_body.h.  Inside no namespace.
// What differs between the entry points, all of it here (texts, codes and their order are part of the interface):
//   mir_signed_distance  refuses rows x probes >= 2^31, and a path longer than 16 bodies only with qpos rows (else no forward kinematics
//                        runs); builds the geometry table BEFORE it returns for zero rows or no output; no not-finite ballot in its
//                        kernel: a probe centre that is not finite loses every comparison and comes out as a miss;
//   mir_self_distance    the same two refusals; its MirSelfQuery BEFORE n_probes; returns for zero rows or no output before the device
//                        is touched; a centre that is not finite makes the whole row -INFINITY;
//   the six of mir_plan  the MirSelfQuery before the MirPlanQuery; no rows x probes refusal; a path longer than 16 bodies always (the
//                        start row goes through the forward kinematics); the planned dofs are checked between the probe links and
//                        the body words; zero rows return MIR_OK before the table is built.
#pragma once
#include <stdint.h>
#include "mirigid.h"

namespace {

// ---- host: probe_link (n host integers, nullable: every probe stands in the world and `link` stays as it is) as one byte per probe.
// Here and below a refusal is `refuse(code, text)`: the caller's, which names the entry point.
template <class Refuse>
static int pack_probe_links(const int32_t* probe_link, int n, int nbody, uint8_t* link, Refuse refuse) {
  if (probe_link)
    for (int i = 0; i < n; i++) {
      if (probe_link[i] < 0 || probe_link[i] >= nbody) return refuse(MIR_E_INVALID, "probe_link outside 0 .. nbody - 1");
      link[i] = (uint8_t)probe_link[i];
    }
  return MIR_OK;
}

// ---- host: the body words of the depth-ordered forward kinematics, body[b] = parent | jtype << 8 | depth << 10 | moves << 15.
// depth: the bodies above b that its pose is composed with (a free body's pose is its qpos pose: depth 0 wherever it hangs).  moves:
// a body of `planned` (MIR_MAX_BODY flags, nullable: none) lies on b's path to the world, b included.  `fk`: the kernel will run the
// forward kinematics, whose rounds allow 16 bodies on a path.  View: parent(b), jtype(b) of a model whose parents precede their
// children.  body[0] is left as it is (zero).
template <class View, class Refuse>
static int build_body_words(const View& mv, int nbody, bool fk, const bool* planned, uint32_t* body, int& depth_max, Refuse refuse) {
  depth_max = 0;
  for (int b = 1; b < nbody; b++) {
    const int par = mv.parent(b), jt = mv.jtype(b);
    const bool chained = par > 0 && jt != MIR_JNT_FREE;
    const int depth = chained ? (int)((body[par] >> 10) & 31) + 1 : 0;
    if (fk && depth >= 16) return refuse(MIR_E_CAPACITY, "path longer than 16 bodies");
    const bool moves = planned && (planned[b] || (chained && ((body[par] >> 15) & 1u)));
    body[b] = (uint32_t)par | (uint32_t)jt << 8 | (uint32_t)depth << 10 | (uint32_t)(moves ? 1 : 0) << 15;
    if (depth > depth_max) depth_max = depth;
  }
  return MIR_OK;
}

}  // namespace

#ifdef __HIPCC__
#include "mir_dist_body.h"

namespace {

// ---- the rows of a call as the three kernels read them: the first member of their arguments
struct SphereRowArgs {
  const long long* env_idx;  // row k is env env_idx[k] (null: env k)
  const float* qpos_o;       // (R, nq) rows in the public layout evaluated in place of the envs' state, nullable
  const float* probes;       // (probes, 4): centre in the link's frame, radius
  int B, n_rows, nbody, nq, depth_max;
  JointPtrs m;
  uint32_t body[MIR_MAX_BODY];    // build_body_words
  uint8_t link[DIST_MAX_PROBES];  // pack_probe_links; all zero when every probe stands in the world
};

// ---- host: the row checks, each entry point in its own order (above)
static int check_rows(MirHandle h, const int64_t* env_idx, int32_t n_rows, const char* who, long long& R) {
  if (h->pending) return query_error(MIR_E_INVALID, who, "a step is pending (mir_step_end first)");
  if (env_idx && n_rows < 0) return query_error(MIR_E_INVALID, who, "negative n_rows");
  R = env_idx ? n_rows : h->B;
  return MIR_OK;
}
static int check_probe_count(long long n, long long R, bool per_probe_outputs, const char* who) {
  if (n > DIST_MAX_PROBES) return query_error(MIR_E_CAPACITY, who, "more than 1024 probes in one call");
  if (per_probe_outputs && R * n > 0x7fffffffLL) return query_error(MIR_E_CAPACITY, who, "rows x probes reaches 2^31");
  return MIR_OK;
}
// what pack_probe_links and build_body_words leave of r
static void fill_sphere_rows(const ModelView& mv, const int64_t* env_idx, long long R, const float* qpos_rows, const float* probes, SphereRowArgs& r) {
  r.env_idx = reinterpret_cast<const long long*>(env_idx); r.qpos_o = qpos_rows; r.probes = probes;
  r.B = mv.h->B; r.n_rows = (int)R; r.nbody = mv.h->nbody; r.nq = mv.h->nq; r.m = mv.joint_pointers();
}

// ---- host: the geometry table of the handle (built by the first call that needs it) as the kernels address it
struct DistTabPtrs { const DistTab* tab; const float *planes, *tris; };
static int fill_dist_tab(MirHandle h, const char* who, DistTabPtrs& t) {
  const int rc = mir_dist_table(h, who);
  if (rc != MIR_OK) return rc;
  const char* const tab = static_cast<const char*>(h->dist_tab);
  t.tab = reinterpret_cast<const DistTab*>(tab);
  t.planes = reinterpret_cast<const float*>(tab + sizeof(DistTab));
  t.tris = t.planes + 4 * (size_t)h->dist_nplane;
  return MIR_OK;
}

// ---- device: the env of a row (an index outside the batch is clamped, as in mir_link_kinematics)
__device__ __forceinline__ int sphere_row_env(const SphereRowArgs& r, int row) {
  const int env = r.env_idx ? (int)r.env_idx[row] : row;
  return env < 0 ? 0 : (env >= r.B ? r.B - 1 : env);
}

// ---- device: the body poses into LDS, lane = body, from the pose cache (rows of 2 x pst float4: positions, then quaternions)
__device__ __forceinline__ void sphere_poses_cached(const float* poses, int pst, int env, int nbody, int lane, float (*xp)[4], float (*xq)[4]) {
  const bool isb = lane < nbody;
  const int b = isb ? lane : 0;
  const float* const pe = poses + (size_t)env * 2 * pst * 4;
  V3 P = v3(0, 0, 0);
  Q4 Qx = Q4{1, 0, 0, 0};
  if (b > 0) {
    P = ld3(pe + b * 4);
    Qx = ld4(pe + (pst + b) * 4);
  }
  if (isb) {
    st3(xp[b], P);
    st4(xq[b], Qx);
  }
  WSYNC();
}

// ---- device: ... or by forward kinematics from the qpos row `qrow` (global or LDS): every lane computes the local transform of its
// body (joint_local) and the world poses are composed parent before child, one round per tree depth (a free body's pose is its qpos
// pose, as in the oracle's fk).  `all`: every body takes part; else the bodies whose word has bit 15 set, the others keep their pose.
__device__ __forceinline__ void sphere_poses_fk(const SphereRowArgs& r, const float* qrow, bool all, int lane, float (*xp)[4], float (*xq)[4]) {
  const bool isb = lane < r.nbody;
  const int b = isb ? lane : 0;
  const uint32_t bw = r.body[b];
  const int par = bw & 0xff, jt = (bw >> 8) & 3, depth = (bw >> 10) & 31;
  const bool mine = isb && (all || ((bw >> 15) & 1u));
  const JointLocal jl = joint_local(mine && b > 0, b, jt, qrow, r.m);
  V3 P = jl.P;
  Q4 Qx = jl.Qx;
  for (int lvl = 0; lvl <= r.depth_max; lvl++) {
    if (mine && depth == lvl) {
      if (lvl > 0) {
        const V3 pp = ld3(xp[par]);
        const Q4 pq = ld4(xq[par]);
        P = pp + qrot(pq, P);
        Qx = qmul(pq, Qx);
      }
      st3(xp[b], P);
      st4(xq[b], Qx);
    }
    WSYNC();
  }
}

// ---- device: probe i at the body poses in LDS: its centre in the world and its radius; the lanes whose centre is not finite; the
// entry of the sphere list (centre, radius: 16 bytes per probe)
struct ProbeWorld { V3 c; float radius; };
__device__ __forceinline__ ProbeWorld probe_world(const SphereRowArgs& r, int i, const float (*xp)[4], const float (*xq)[4]) {
  const float* const pr = r.probes + (size_t)i * 4;
  const float radius = pr[3];
  const int lk = r.link[i];
  return {ld3(xp[lk]) + qrot(ld4(xq[lk]), ld3(pr)), radius};
}
__device__ __forceinline__ unsigned long long probe_nonfinite(bool valid, V3 c) {
  return __ballot(valid && (nonfinite(c.x) || nonfinite(c.y) || nonfinite(c.z)));
}
__device__ __forceinline__ void sphere_store(float* sph, int i, V3 c, const float* radius) {
  st3(sph + 4 * i, c);
  sph[4 * i + 3] = *radius;
}
// the entries of probes i0 .. n - 1, lane = probe in chunks of 64 -> the lanes whose centre is not finite.  The radius is read behind
// the store of the centre (sphere_store takes its address): read in front of it, the planner with self model and carried object is 1.5 % slower.
__device__ __forceinline__ unsigned long long sphere_list_fill(const SphereRowArgs& r, int i0, int n, int lane, const float (*xp)[4], const float (*xq)[4],
                                                                float* sph) {
  unsigned long long nan = 0ull;
  for (int base = i0; base < n; base += 64) {
    const bool valid = base + lane < n;
    const int probe = valid ? base + lane : n - 1;
    const ProbeWorld p = probe_world(r, probe, xp, xq);
    nan |= probe_nonfinite(valid, p.c);
    if (valid) sphere_store(sph, probe, p.c, r.probes + (size_t)probe * 4 + 3);
  }
  return nan;
}

// ---- device: wave reductions (every lane takes part and holds the result)
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fminf(v, __shfl_xor(v, off));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
  return v;
}
// the lowest v with its index i, the lower index keeping a tie; `ride` travels with the winner (self's pair partner)
struct ArgMin { float v; int i, ride; };
__device__ __forceinline__ ArgMin wave_argmin(float v, int i, int ride = 0) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float ov = __shfl_xor(v, off);
    const int oi = __shfl_xor(i, off), oride = __shfl_xor(ride, off);
    if (ov < v || (ov == v && oi < i)) { v = ov; i = oi; ride = oride; }
  }
  return {v, i, ride};
}

}  // namespace
#endif  // __HIPCC__
