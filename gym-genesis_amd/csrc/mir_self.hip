// mir_self.hip — batched self-distance queries of a sphere model (mir_self_distance, include/mirigid.h; DESIGN.md "Self-collision").
//
// What it serves: for a list of envs, the lowest signed distance from every probe sphere of an entity's model to the spheres on the
// links it is tested against (MirSelfQuery.link_mask), and the row's lowest pair: EntityView.get_self_clearance / in_self_collision.
// It reads the pose cache (or, with candidate qpos rows, the compiled model alone) and writes only its outputs.
//
// Mapping: one workgroup of one wave64 per row, as mir_dist.hip.
//   Poses.  Lane = body: the pose cache, or the forward kinematics of mir_dist_kernel from the qpos row (the same arithmetic).
//   List.   Lane = probe in chunks of 64: world centre and radius to an LDS list of 16 bytes per probe (N + E <= 1024: 16 KB).
//   Pairs.  Lane = probe i in chunks of 64, a loop over j through the list (self_probe_min of mir_self_body.h: a chunk of the list per
//   lane, sphere j to all lanes by v_readlane; the pair filter is one bit of link_mask[link_i]).
// Stores: plain dword stores; a per-lane running minimum over the chunks, then one wave reduction.  No atomics, no scratch, no
//   cross-wave barrier; WSYNC() only.  Every loop is bounded by N + E or the tree depth.
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

#include "mir_dist_body.h"

#include "mir_self_body.h"

namespace {

struct SelfArgs {
  const float* poses;  // pose cache (qpos_o == NULL)
  int pst, B, n_rows, NS, nbody, nq, depth_max;
  float max_distance;
  const float* probes;
  const long long* env_idx;
  const float* qpos_o;  // (R, nq) public layout, nullable
  JointPtrs m;
  float *distance, *row_min;
  int32_t *other, *row_pair;
  uint32_t body[MIR_MAX_BODY];  // parent | jtype << 8 | depth << 10
  uint32_t link_mask[MIR_MAX_BODY];
  uint8_t link[DIST_MAX_PROBES];
};
static_assert(sizeof(SelfArgs) <= 4096, "kernel arguments");

__global__ __launch_bounds__(64) void mir_self_kernel(SelfArgs a) {
  __shared__ float xp[MIR_MAX_BODY][4], xq[MIR_MAX_BODY][4];
  __shared__ float sph[DIST_MAX_PROBES * 4];
  const int lane = threadIdx.x;
  const int row = blockIdx.x;
  int env = a.env_idx ? (int)a.env_idx[row] : row;
  env = env < 0 ? 0 : (env >= a.B ? a.B - 1 : env);  // (an index outside the batch is clamped, as in mir_link_kinematics)

  // ---- body poses, lane = body (the two routes of mir_dist_kernel)
  {
    const bool isb = lane < a.nbody;
    const int b = isb ? lane : 0;
    if (!a.qpos_o) {
      const float* const pe = a.poses + (size_t)env * 2 * a.pst * 4;
      V3 P = v3(0, 0, 0);
      Q4 Qx = Q4{1, 0, 0, 0};
      if (b > 0) {
        P = ld3(pe + b * 4);
        Qx = ld4(pe + (a.pst + b) * 4);
      }
      if (isb) {
        st3(xp[b], P);
        st4(xq[b], Qx);
      }
      WSYNC();
    } else {
      const uint32_t bw = a.body[b];
      const int par = bw & 0xff, jt = (bw >> 8) & 3, depth = (bw >> 10) & 31;
      const JointLocal jl = joint_local(isb && b > 0, b, jt, a.qpos_o + (size_t)row * a.nq, a.m);
      V3 P = jl.P;
      Q4 Qx = jl.Qx;
      for (int lvl = 0; lvl <= a.depth_max; lvl++) {
        if (isb && depth == lvl) {
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
  }

  // ---- the sphere list
  unsigned long long nan = 0ull;
  for (int base = 0; base < a.NS; base += 64) {
    const bool valid = base + lane < a.NS;
    const int probe = valid ? base + lane : a.NS - 1;
    const float* const pr = a.probes + (size_t)probe * 4;
    const int lk = a.link[probe];
    const V3 pw = ld3(xp[lk]) + qrot(ld4(xq[lk]), ld3(pr));
    nan |= __ballot(valid && (nonfinite(pw.x) || nonfinite(pw.y) || nonfinite(pw.z)));
    if (valid) {
      st3(sph + 4 * probe, pw);
      sph[4 * probe + 3] = pr[3];
    }
  }
  const bool blocked = nan != 0ull;  // a centre that is not finite: the whole row is -INFINITY, as a configuration of the planner
  WSYNC();

  // ---- pairs
  float run_min = INFINITY;
  int run_i = 0x7fffffff, run_j = -1;
  for (int base = 0; base < a.NS; base += 64) {
    const bool valid = base + lane < a.NS;
    const int i = valid ? base + lane : a.NS - 1;
    const SelfBest w = self_probe_min<true>(sph, a.link, a.NS, 0, i, a.link_mask[a.link[i]], lane);
    const bool hit = !blocked && w.j >= 0 && w.best <= a.max_distance;
    const float dist = blocked ? -INFINITY : (hit ? w.best : a.max_distance);
    const int oj = hit ? w.j : -1;
    if (valid) {
      const size_t cell = (size_t)row * a.NS + i;
      if (a.distance) a.distance[cell] = dist;
      if (a.other) a.other[cell] = oj;
      if (hit && dist < run_min) { run_min = dist; run_i = i; run_j = oj; }  // (chunks ascend: the lower i keeps a tie)
    }
  }
  if (a.row_min || a.row_pair) {  // (uniform over the launch)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const float om = __shfl_xor(run_min, off);
      const int oi = __shfl_xor(run_i, off), oj = __shfl_xor(run_j, off);
      if (om < run_min || (om == run_min && oi < run_i)) { run_min = om; run_i = oi; run_j = oj; }
    }
    if (lane == 0) {
      const bool any = run_j >= 0;
      if (a.row_min) a.row_min[row] = blocked ? -INFINITY : (any ? run_min : a.max_distance);
      if (a.row_pair) {
        a.row_pair[(size_t)row * 2] = any ? run_i : -1;
        a.row_pair[(size_t)row * 2 + 1] = any ? run_j : -1;
      }
    }
  }
}

}  // namespace

extern "C" int mir_self_distance(MirHandle h, const MirSelfQuery* sq, int32_t n_probes, const float* probes, const int32_t* probe_link,
                                 const int64_t* env_idx, int32_t n_rows, const float* qpos, float* distance, int32_t* other, float* row_min,
                                 int32_t* row_pair, void* stream) {
  static const char who[] = "mir_self_distance";
  if (!h || !probes) return query_error(MIR_E_INVALID, who, "null argument");
  int rc = self_query_check(h, sq, who);
  if (rc != MIR_OK) return rc;
  if (n_probes < 1) return query_error(MIR_E_INVALID, who, "n_probes < 1");
  if (h->pending) return query_error(MIR_E_INVALID, who, "a step is pending (mir_step_end first)");
  if (env_idx && n_rows < 0) return query_error(MIR_E_INVALID, who, "negative n_rows");
  const long long R = env_idx ? n_rows : h->B, NS = (long long)n_probes + sq->n_extra;
  if (NS > DIST_MAX_PROBES) return query_error(MIR_E_CAPACITY, who, "more than 1024 probes in one call");
  if (R * NS > 0x7fffffffLL) return query_error(MIR_E_CAPACITY, who, "rows x probes reaches 2^31");
  SelfArgs a;
  memset(&a, 0, sizeof a);
  if (probe_link)
    for (int i = 0; i < (int)NS; i++) {
      if (probe_link[i] < 0 || probe_link[i] >= h->nbody) return query_error(MIR_E_INVALID, who, "probe_link outside 0 .. nbody - 1");
      a.link[i] = (uint8_t)probe_link[i];
    }
  const ModelView mv(h);
  int depth_max = 0;
  for (int b = 1; b < h->nbody; b++) {  // (body order: a parent comes before its children)
    const int par = mv.parent(b), jt = mv.jtype(b);
    const int depth = par > 0 && jt != MIR_JNT_FREE ? (int)((a.body[par] >> 10) & 31) + 1 : 0;
    if (qpos && depth >= G) return query_error(MIR_E_CAPACITY, who, "path longer than 16 bodies");
    a.body[b] = (uint32_t)par | (uint32_t)jt << 8 | (uint32_t)depth << 10;
    if (depth > depth_max) depth_max = depth;
  }
  if (R == 0 || (!distance && !other && !row_min && !row_pair)) return MIR_OK;  // (nothing asked for)
  DeviceGuard guard(h->device);  // (the pose refresh, too)
  // link poses: the rasteriser's pose cache, refreshed when the state has moved since it was written; not touched with qpos rows
  if (!qpos && !h->poses_current && (rc = mir_refresh_poses(h, stream)) != MIR_OK) return rc;
  a.poses = h->poses; a.pst = h->pt.pst; a.B = h->B; a.n_rows = (int)R; a.NS = (int)NS; a.nbody = h->nbody; a.nq = h->nq; a.depth_max = depth_max;
  a.max_distance = sq->max_distance;
  memcpy(a.link_mask, sq->link_mask, sizeof a.link_mask);
  a.probes = probes; a.env_idx = reinterpret_cast<const long long*>(env_idx); a.qpos_o = qpos;
  a.m = mv.joint_pointers();
  a.distance = distance; a.other = other; a.row_min = row_min; a.row_pair = row_pair;
  return launch_rows<64>(h, mir_self_kernel, R, stream, a);
}
