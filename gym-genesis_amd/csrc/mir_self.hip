// mir_self.hip — batched self-distance queries of a sphere model (mir_self_distance, include/mirigid.h; DESIGN.md "Self-collision").
//
// What it serves: for a list of envs, the lowest signed distance from every probe sphere of an entity's model to the spheres on the
// links it is tested against (MirSelfQuery.link_mask), and the row's lowest pair: EntityView.get_self_clearance / in_self_collision.
// It reads the pose cache (or, with candidate qpos rows, the compiled model alone) and writes only its outputs.
//
// Mapping: one workgroup of one wave64 per row, as mir_dist.hip.  Poses, list, the row's env, the wave reduction and the host's row
//   checks and argument filling are the front end shared with mir_dist.hip and mir_plan.hip: mir_sphere_front.h.
//   Poses.  Lane = body: the pose cache, or the forward kinematics from the qpos row.
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
#include "mir_sphere_front.h"  // (brings mir_dist_body.h)

#include "mir_self_body.h"

namespace {

struct SelfArgs {
  SphereRowArgs r;
  const float* poses;  // pose cache (r.qpos_o == NULL)
  int pst, NS;
  float max_distance;
  float *distance, *row_min;
  int32_t *other, *row_pair;
  uint32_t link_mask[MIR_MAX_BODY];
};
static_assert(sizeof(SelfArgs) <= 4096, "kernel arguments");

__global__ __launch_bounds__(64) void mir_self_kernel(SelfArgs a) {
  __shared__ float xp[MIR_MAX_BODY][4], xq[MIR_MAX_BODY][4];
  __shared__ float sph[DIST_MAX_PROBES * 4];
  const int lane = threadIdx.x, row = blockIdx.x;

  // ---- body poses, lane = body
  if (!a.r.qpos_o) sphere_poses_cached(a.poses, a.pst, sphere_row_env(a.r, row), a.r.nbody, lane, xp, xq);
  else sphere_poses_fk(a.r, a.r.qpos_o + (size_t)row * a.r.nq, true, lane, xp, xq);

  // ---- the sphere list.  A centre that is not finite: the whole row is -INFINITY, as a configuration of the planner
  const bool blocked = sphere_list_fill(a.r, 0, a.NS, lane, xp, xq, sph) != 0ull;
  WSYNC();

  // ---- pairs
  float run_min = INFINITY;
  int run_i = 0x7fffffff, run_j = -1;
  for (int base = 0; base < a.NS; base += 64) {
    const bool valid = base + lane < a.NS;
    const int i = valid ? base + lane : a.NS - 1;
    const SelfBest w = self_probe_min<true>(sph, a.r.link, a.NS, 0, i, a.link_mask[a.r.link[i]], lane);
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
    const ArgMin m = wave_argmin(run_min, run_i, run_j);
    if (lane == 0) {
      const bool any = m.ride >= 0;
      if (a.row_min) a.row_min[row] = blocked ? -INFINITY : (any ? m.v : a.max_distance);
      if (a.row_pair) {
        a.row_pair[(size_t)row * 2] = any ? m.i : -1;
        a.row_pair[(size_t)row * 2 + 1] = any ? m.ride : -1;
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
  long long R, NS = (long long)n_probes + sq->n_extra;
  if ((rc = check_rows(h, env_idx, n_rows, who, R)) != MIR_OK) return rc;
  if ((rc = check_probe_count(NS, R, true, who)) != MIR_OK) return rc;
  SelfArgs a;
  memset(&a, 0, sizeof a);
  const ModelView mv(h);
  const auto refuse = [&](int code, const char* what) { return query_error(code, who, what); };
  if ((rc = pack_probe_links(probe_link, (int)NS, h->nbody, a.r.link, refuse)) != MIR_OK) return rc;
  if ((rc = build_body_words(mv, h->nbody, qpos != nullptr, nullptr, a.r.body, a.r.depth_max, refuse)) != MIR_OK) return rc;
  if (R == 0 || (!distance && !other && !row_min && !row_pair)) return MIR_OK;  // (nothing asked for)
  DeviceGuard guard(h->device);  // (the pose refresh, too)
  // link poses: the rasteriser's pose cache, refreshed when the state has moved since it was written; not touched with qpos rows
  if (!qpos && !h->poses_current && (rc = mir_refresh_poses(h, stream)) != MIR_OK) return rc;
  fill_sphere_rows(mv, env_idx, R, qpos, probes, a.r);
  a.poses = h->poses; a.pst = h->pt.pst; a.NS = (int)NS; a.max_distance = sq->max_distance;
  memcpy(a.link_mask, sq->link_mask, sizeof a.link_mask);
  a.distance = distance; a.other = other; a.row_min = row_min; a.row_pair = row_pair;
  return launch_rows<64>(h, mir_self_kernel, R, stream, a);
}
