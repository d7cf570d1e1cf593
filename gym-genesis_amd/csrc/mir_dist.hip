// mir_dist.hip — batched signed-distance queries (mir_signed_distance, include/mirigid.h; DESIGN.md "signed distance and clearance").
//
// What it serves: the signed distance, closest surface point and outward gradient from N probe spheres -- points with a radius that
// ride on links or stand in the world -- to the nearest geom of the scene, for a list of envs, in one launch of a kernel of its own:
// proximity sensors, clearance rewards, and the clearance of an arm's sphere model at candidate configurations (EntityView.get_clearance).
// It reads the pose cache (or, with candidate qpos rows, the compiled model alone) and a geometry table of its own and writes only its
// outputs.
//
// Mapping: one workgroup of one wave64 per row.
//   Poses.  Lane = body.  Without qpos the body poses are copied from the pose cache to LDS.  With qpos every lane computes the local
//   transform of its body from the row (joint_local of mir_query.h) and the world poses are composed parent before child, one round
//   per tree depth, in LDS (a free body's pose is its qpos pose, as in the oracle's fk).
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

#include "mir_hullfan.h"

#include "mir_dist_body.h"

namespace {

struct DistArgs {
  const DistTab* tab;
  const float *planes, *tris;
  const float* poses;  // pose cache (qpos_o == NULL)
  int pst, B, n_rows, N, nbody, nq, depth_max;
  float max_distance;
  unsigned long long skip;
  const float* probes;
  const long long* env_idx;
  const float* qpos_o;  // (R, nq) public layout, nullable
  JointPtrs m;
  float *distance, *closest, *normal, *row_min;
  int32_t *geom, *row_argmin;
  uint32_t body[MIR_MAX_BODY];     // parent | jtype << 8 | depth << 10 (depth: bodies above it that its pose is composed with)
  uint8_t link[DIST_MAX_PROBES];   // all zero when every probe stands in the world
};
static_assert(sizeof(DistArgs) <= 4096, "kernel arguments");

__global__ __launch_bounds__(64) void mir_dist_kernel(DistArgs a) {
  __shared__ float xp[MIR_MAX_BODY][4], xq[MIR_MAX_BODY][4];
  __shared__ float rec[MIR_MAX_GEOM * DIST_REC];
  const int lane = threadIdx.x;
  const int row = blockIdx.x;
  int env = a.env_idx ? (int)a.env_idx[row] : row;
  env = env < 0 ? 0 : (env >= a.B ? a.B - 1 : env);  // (an index outside the batch is clamped, as in mir_link_kinematics)

  // ---- body poses, lane = body
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

  // ---- geom records, lane = geom (mir_dist_body.h)
  int count = dist_build_records(a.tab, a.skip, lane, xp, xq, rec);
  count = __builtin_amdgcn_readfirstlane(count);

  // ---- probes, 64 at a time
  float run_min = INFINITY;
  int run_arg = 0;
  for (int base = 0; base < a.N; base += 64) {
    const bool valid = base + lane < a.N;
    const int probe = valid ? base + lane : a.N - 1;
    const float* const pr = a.probes + (size_t)probe * 4;
    const float radius = pr[3];
    const int lk = a.link[probe];
    const V3 pw = ld3(xp[lk]) + qrot(ld4(xq[lk]), ld3(pr));  // probe centre, world
    const DistBest w = dist_probe_min(rec, count, a.planes, a.tris, pw, radius, a.max_distance);
    const float best = w.best;
    const int bestk = w.bestk;
    const V3 bc = w.bc, bn = w.bn;  // closest point and normal of the best geom, in its frame
    const bool hit = bestk >= 0 && best <= a.max_distance;
    const float dist = hit ? best : a.max_distance;
    const size_t cell = (size_t)row * a.N + probe;
    const float* const rb = rec + (hit ? bestk : 0) * DIST_REC;
    if (valid) {
      if (a.distance) a.distance[cell] = dist;
      if (a.geom) a.geom[cell] = hit ? __float_as_int(rb[1]) : -1;
      if (a.closest) {
        V3 o = pw;
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
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const float om = __shfl_xor(run_min, off);
      const int oa = __shfl_xor(run_arg, off);
      if (om < run_min || (om == run_min && oa < run_arg)) { run_min = om; run_arg = oa; }
    }
    if (lane == 0) {
      if (a.row_min) a.row_min[row] = run_min;
      if (a.row_argmin) a.row_argmin[row] = run_arg;
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
  if (h->pending) return query_error(MIR_E_INVALID, who, "a step is pending (mir_step_end first)");
  if (env_idx && n_rows < 0) return query_error(MIR_E_INVALID, who, "negative n_rows");
  const long long R = env_idx ? n_rows : h->B, N = q->n_probes;
  if (N > DIST_MAX_PROBES) return query_error(MIR_E_CAPACITY, who, "more than 1024 probes in one call");
  if (R * N > 0x7fffffffLL) return query_error(MIR_E_CAPACITY, who, "rows x probes reaches 2^31");
  DistArgs a;
  memset(&a, 0, sizeof a);
  if (probe_link)
    for (int i = 0; i < (int)N; i++) {
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
  DeviceGuard guard(h->device);  // (the table's allocation and the pose refresh, too)
  int rc = MIR_OK;
  do {
    if ((rc = mir_dist_table(h, who)) != MIR_OK) break;
    if (R == 0 || (!distance && !geom && !closest && !normal && !row_min && !row_argmin)) break;  // (nothing asked for)
    // link poses: the rasteriser's pose cache, refreshed when the state has moved since it was written; not touched with qpos rows
    if (!qpos && !h->poses_current && (rc = mir_refresh_poses(h, stream)) != MIR_OK) break;
    const char* const tab = static_cast<const char*>(h->dist_tab);
    a.tab = reinterpret_cast<const DistTab*>(tab);
    a.planes = reinterpret_cast<const float*>(tab + sizeof(DistTab));
    a.tris = a.planes + 4 * (size_t)h->dist_nplane;
    a.poses = h->poses; a.pst = h->pt.pst; a.B = h->B; a.n_rows = (int)R; a.N = (int)N; a.nbody = h->nbody; a.nq = h->nq; a.depth_max = depth_max;
    a.max_distance = q->max_distance; a.skip = q->skip_geoms;
    a.probes = probes; a.env_idx = reinterpret_cast<const long long*>(env_idx); a.qpos_o = qpos;
    a.m = mv.joint_pointers();
    a.distance = distance; a.closest = closest; a.normal = normal; a.row_min = row_min; a.geom = geom; a.row_argmin = row_argmin;
    rc = launch_rows<64>(h, mir_dist_kernel, R, stream, a);
  } while (0);
  return rc;
}
