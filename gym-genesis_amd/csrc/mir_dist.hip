// mir_dist.hip — batched signed-distance queries (mir_signed_distance, include/mirigid.h; DESIGN.md "signed distance and clearance").
//
// What it serves: the signed distance, closest surface point and outward gradient from N probe spheres -- points with a radius that
// ride on links or stand in the world -- to the nearest geom of the scene, for a list of envs, in one launch of a kernel of its own:
// proximity sensors, clearance rewards, and the clearance of an arm's sphere model at candidate configurations (EntityView.get_clearance).
// It reads the pose cache (or, with candidate qpos rows, the compiled model alone) and a geometry table of its own and writes only its
// outputs.
//
// Mapping: one workgroup of one wave64 per row.
//   Poses.  Lane = body.  Without qpos the body poses are copied from the pose cache to LDS (sphere_poses_cached), with qpos they are
//   composed from the row (sphere_poses_fk).  Those, the row's env, the probe centres and the wave reduction are the front end that
//   this kernel shares with mir_self.hip and mir_plan.hip: mir_sphere_front.h, like the host's row checks and argument filling.
//   Geoms.  Lane = geom (ngeom <= 40): the geom's world frame (the arithmetic of mir_ray_kernel's prologue); the geoms whose skip bit
//   is clear are compacted in geom order by a ballot into an LDS list of 24-float records.
//   Probes.  Chunks of 64, lane = probe.  A lane reads its link's pose from LDS and walks the list: the record address and the geom
//   type are wave-uniform (LDS broadcast reads), the hull planes and triangles are read at wave-uniform global addresses.  Every
//   distance is a closed form; a hull outside is the minimum over its triangle fans (closed-form point - triangle), skipped for the
//   whole wave when no lane's bounding-sphere bound can beat what it holds.
// Stores: plain dword stores (rows are short: <= 1024 probes).  row_min / row_argmin: a per-lane running minimum over the chunks, then
//   one wave reduction.  No atomics, no scratch, no cross-wave barrier.  Whole waves reach every ballot and shuffle: lanes beyond N are
//   clamped to the last probe and their stores predicated.
// probe_link is a HOST array: it is checked on the host and travels in the kernel arguments, one byte per probe (hence N <= 1024).
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "mir_model.h"
#include "mir_model64.h"
#include "mir_scene.h"

#define G 16
#include "mir_dev.h"

#include "mir_query.h"
#include "mir_sphere_front.h"  // (brings mir_dist_body.h)

#include "mir_hullfan.h"

namespace {

struct DistArgs {
  SphereRowArgs r;
  DistTabPtrs t;
  const float* poses;  // pose cache (r.qpos_o == NULL)
  int pst, N;
  float max_distance;
  unsigned long long skip;
  float *distance, *closest, *normal, *row_min;
  int32_t *geom, *row_argmin;
};
static_assert(sizeof(DistArgs) <= 4096, "kernel arguments");

__global__ __launch_bounds__(64) void mir_dist_kernel(DistArgs a) {
  __shared__ float xp[MIR_MAX_BODY][4], xq[MIR_MAX_BODY][4];
  __shared__ float rec[MIR_MAX_GEOM * DIST_REC];
  const int lane = threadIdx.x, row = blockIdx.x;

  // ---- body poses, lane = body
  if (!a.r.qpos_o) sphere_poses_cached(a.poses, a.pst, sphere_row_env(a.r, row), a.r.nbody, lane, xp, xq);
  else sphere_poses_fk(a.r, a.r.qpos_o + (size_t)row * a.r.nq, true, lane, xp, xq);

  // ---- geom records, lane = geom (mir_dist_body.h)
  const int count = __builtin_amdgcn_readfirstlane(dist_build_records(a.t.tab, a.skip, lane, xp, xq, rec));

  // ---- probes, 64 at a time
  float run_min = INFINITY;
  int run_arg = 0;
  for (int base = 0; base < a.N; base += 64) {
    const bool valid = base + lane < a.N;
    const int probe = valid ? base + lane : a.N - 1;
    const ProbeWorld p = probe_world(a.r, probe, xp, xq);
    const DistBest w = dist_probe_min(rec, count, a.t.planes, a.t.tris, p.c, p.radius, a.max_distance);
    const V3 bc = w.bc, bn = w.bn;  // closest point and normal of the best geom, in its frame
    const bool hit = w.bestk >= 0 && w.best <= a.max_distance;
    const float dist = hit ? w.best : a.max_distance;
    const size_t cell = (size_t)row * a.N + probe;
    const float* const rb = rec + (hit ? w.bestk : 0) * DIST_REC;
    if (valid) {
      if (a.distance) a.distance[cell] = dist;
      if (a.geom) a.geom[cell] = hit ? __float_as_int(rb[1]) : -1;
      if (a.closest) {
        V3 o = p.c;
        if (hit) o = v3(rb[5] + rb[8] * bc.x + rb[9] * bc.y + rb[10] * bc.z, rb[6] + rb[11] * bc.x + rb[12] * bc.y + rb[13] * bc.z,
                        rb[7] + rb[14] * bc.x + rb[15] * bc.y + rb[16] * bc.z);
        st3(a.closest + cell * 3, o);
      }
      if (a.normal) {
        V3 o = v3(0, 0, 0);
        if (hit) o = v3(rb[8] * bn.x + rb[9] * bn.y + rb[10] * bn.z, rb[11] * bn.x + rb[12] * bn.y + rb[13] * bn.z, rb[14] * bn.x + rb[15] * bn.y + rb[16] * bn.z);
        st3(a.normal + cell * 3, o);
      }
      if (dist < run_min) { run_min = dist; run_arg = probe; }  // (chunks ascend: the lower index keeps a tie)
    }
  }
  if (a.row_min || a.row_argmin) {  // (uniform over the launch)
    const ArgMin m = wave_argmin(run_min, run_arg);
    if (lane == 0) {
      if (a.row_min) a.row_min[row] = m.v;
      if (a.row_argmin) a.row_argmin[row] = m.i;
    }
  }
}

// ---- the geometry table, once per handle: geoms as the compiled model holds them (float32), hull faces by mir_hullfan.h
int build_tab(MirScene* h, const char* who) {
  DistTab tab;
  memset(&tab, 0, sizeof tab);
  HullFan fan;
  const bool k16 = h->kernel == 16;
  tab.ngeom = h->ngeom;
  for (int g = 0; g < h->ngeom; g++) {
    DistGeom& r = tab.g[g];
    r.type = k16 ? h->hm.g_type[g] : h->hm64.g_type[g];
    r.body = k16 ? h->hm.g_body[g] : h->hm64.g_body[g];
    for (int k = 0; k < 3; k++) {
      r.size[k] = k16 ? h->hm.g_size[g][k] : h->hm64.g_size[g][k];
      r.pos[k] = k16 ? h->hm.g_pos[g][k] : h->hm64.g_pos[g][k];
    }
    for (int k = 0; k < 4; k++) r.quat[k] = k16 ? h->hm.g_quat[g][k] : h->hm64.g_quat[g][k];
    if (r.body < 0 || r.body >= h->nbody) return query_error(MIR_E_INVALID, who, "a geom's body lies outside the scene");
    double rad = 0.0;
    if (r.type == MIR_GEOM_HULL) {
      const int v0 = (int)r.size[0], nv = (int)r.size[1];
      const int pool = k16 ? K16_MAX_VERT : MIR_MAX_VERT;
      if (v0 < 0 || nv < 0 || nv > MIR_MAX_HULL_VERT || v0 + nv > pool) return query_error(MIR_E_INVALID, who, "a hull's vertices lie outside the pool");
      double v[MIR_MAX_HULL_VERT][3];
      for (int i = 0; i < nv; i++) {
        for (int k = 0; k < 3; k++) v[i][k] = k16 ? h->hm.hverts[v0 + i][k] : h->hm64.hverts[v0 + i][k];
        rad = std::fmax(rad, std::sqrt(v[i][0] * v[i][0] + v[i][1] * v[i][1] + v[i][2] * v[i][2]));
      }
      r.p0 = (int)(fan.planes.size() / 4);
      r.t0 = (int)(fan.tris.size() / 12);
      if (!hull_fan_build(v, nv, fan)) return query_error(MIR_E_INVALID, who, "a hull geom has no volume (its vertices lie in one plane)");
      r.np = (int)(fan.planes.size() / 4) - r.p0;
      r.nt = (int)(fan.tris.size() / 12) - r.t0;
    }
    r.rad = (float)(rad * (1.0 + 1e-4));  // (a bound for the cull only, with room for float32 rounding)
  }
  tab.nplane = (int)(fan.planes.size() / 4);
  tab.ntri = (int)(fan.tris.size() / 12);
  const size_t bytes = sizeof(DistTab) + (fan.planes.size() + fan.tris.size() + 4) * sizeof(float);
  char* dev = nullptr;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&dev), bytes);
  if (e == hipSuccess) e = hipMemcpy(dev, &tab, sizeof tab, hipMemcpyHostToDevice);
  if (e == hipSuccess && !fan.planes.empty()) e = hipMemcpy(dev + sizeof tab, fan.planes.data(), fan.planes.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess && !fan.tris.empty())
    e = hipMemcpy(dev + sizeof tab + fan.planes.size() * sizeof(float), fan.tris.data(), fan.tris.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    if (dev) (void)hipFree(dev);
    return mir_set_error(MIR_E_HIP, hipGetErrorString(e));
  }
  h->dist_tab = dev;
  h->dist_nplane = tab.nplane;
  return MIR_OK;
}

}  // namespace

// the table of the handle for the entry points that read it (this file and mir_plan.hip); the verdict on a hull without volume is kept
int mir_dist_table(MirScene* h, const char* who) {
  int rc = MIR_OK;
  if (h->dist_state == 0) h->dist_state = (rc = build_tab(h, who)) == MIR_OK ? 1 : (rc == MIR_E_INVALID ? -1 : 0);
  else if (h->dist_state < 0) rc = query_error(MIR_E_INVALID, who, "a hull geom has no volume (its vertices lie in one plane)");
  return rc;
}

extern "C" int mir_dist_query_sizeof(void) { return (int)sizeof(MirDistQuery); }

extern "C" int mir_signed_distance(MirHandle h, const MirDistQuery* q, const float* probes, const int32_t* probe_link, const int64_t* env_idx,
                                   int32_t n_rows, const float* qpos, float* distance, int32_t* geom, float* closest, float* normal,
                                   float* row_min, int32_t* row_argmin, void* stream) {
  static const char who[] = "mir_signed_distance";
  if (!h || !q || !probes) return query_error(MIR_E_INVALID, who, "null argument");
  if (q->struct_size != (int32_t)sizeof(MirDistQuery)) return query_error(MIR_E_INVALID, who, "struct_size is not sizeof(MirDistQuery)");
  if (q->n_probes < 1) return query_error(MIR_E_INVALID, who, "n_probes < 1");
  if (!std::isfinite(q->max_distance) || !(q->max_distance > 0.0f)) return query_error(MIR_E_INVALID, who, "max_distance must be finite and > 0");
  if (q->flags) return query_error(MIR_E_INVALID, who, "unknown flag bit");
  if (h->ngeom < 64 && (q->skip_geoms >> h->ngeom)) return query_error(MIR_E_INVALID, who, "skip_geoms names a geom at or above ngeom");
  int rc;
  long long R, N = q->n_probes;
  if ((rc = check_rows(h, env_idx, n_rows, who, R)) != MIR_OK) return rc;
  if ((rc = check_probe_count(N, R, true, who)) != MIR_OK) return rc;
  DistArgs a;
  memset(&a, 0, sizeof a);
  const ModelView mv(h);
  const auto refuse = [&](int code, const char* what) { return query_error(code, who, what); };
  if ((rc = pack_probe_links(probe_link, (int)N, h->nbody, a.r.link, refuse)) != MIR_OK) return rc;
  if ((rc = build_body_words(mv, h->nbody, qpos != nullptr, nullptr, a.r.body, a.r.depth_max, refuse)) != MIR_OK) return rc;
  DeviceGuard guard(h->device);  // (the table's allocation and the pose refresh, too)
  if ((rc = fill_dist_tab(h, who, a.t)) != MIR_OK) return rc;
  if (R == 0 || (!distance && !geom && !closest && !normal && !row_min && !row_argmin)) return MIR_OK;  // (nothing asked for)
  // link poses: the rasteriser's pose cache, refreshed when the state has moved since it was written; not touched with qpos rows
  if (!qpos && !h->poses_current && (rc = mir_refresh_poses(h, stream)) != MIR_OK) return rc;
  fill_sphere_rows(mv, env_idx, R, qpos, probes, a.r);
  a.poses = h->poses; a.pst = h->pt.pst; a.N = (int)N; a.max_distance = q->max_distance; a.skip = q->skip_geoms;
  a.distance = distance; a.closest = closest; a.normal = normal; a.row_min = row_min; a.geom = geom; a.row_argmin = row_argmin;
  return launch_rows<64>(h, mir_dist_kernel, R, stream, a);
}
