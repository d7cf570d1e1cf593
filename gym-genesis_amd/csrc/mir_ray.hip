// mir_ray.hip — batched ray-cast range sensing (mir_raycast, include/mirigid.h; DESIGN.md sensor-3).
//
// What it serves: scene.add_sensor(gs.sensors.Lidar / Raycaster / DepthCamera) + sensor.read() of Genesis -- the Euclidean range to the
// nearest surface along each ray of a pattern that rides on a link (or stands in the world), for a list of envs, in one launch of a
// kernel of its own.  It reads the pose cache (what the rasteriser reads) and a geometry table of its own and writes only its outputs.
//
// Mapping: workgroup = 256 rays of one row (1-D grid, rows x ceil(N / 256) workgroups), one lane owns one ray.
//   Prologue, wave 0, lane = geom (ngeom <= 40): the geom's world frame from the pose cache (the arithmetic at the top of
//   k_render_setup), the sensor origin in the geom's frame and M = R_g^T R_s, which takes a sensor-frame direction into the geom's frame.
//   A geom that is skipped, that contains the origin, or whose bounding sphere starts beyond max_range is dropped; the others are
//   compacted in geom order by a ballot into an LDS list of 32-float records.
//   Per ray: every lane walks the list.  The record address is wave-uniform (LDS broadcast reads, no bank conflicts) and so is the geom
//   type: nine FMAs for the direction, one closed-form intersection.  A hull is clipped against its face planes (geom frame, computed
//   once per handle on the host), read at a wave-uniform global address.
// Stores: distance and geom one dword per lane.  points / normal are 12 B per ray: the workgroup's 768 floats are staged in LDS at the
//   same 16-byte phase as their global address and leave as 16-byte stores; only the (at most two) chunks that straddle the ends of the
//   workgroup's span take 4-byte stores.  No atomics, no scratch.  Whole waves reach every ballot and barrier: lanes beyond N are clamped
//   to the last ray and their stores predicated.
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

namespace {

constexpr int RAY_TPB = 256;
constexpr int RAY_REC = 32;  // floats per LDS record

// per-handle geometry table (device): the geoms as the spec has them -- hulls as hulls -- and the face planes of every hull
struct RayGeom {
  int32_t type, body, p0, np;  // p0, np: the hull's planes in RayTab::planes
  float size[3], rad;          // rad: radius of the bounding sphere about the geom frame's origin
  float pos[3], quat[4];
};
struct RayTab {
  int32_t ngeom, nplane, _pad[2];
  RayGeom g[MIR_MAX_GEOM];
  // float4 planes[nplane] follow: unit outward normal, offset (n . x <= d inside), geom frame
};

struct RayArgs {
  const RayTab* tab;
  const float* planes;
  const float* poses;
  int pst, B, n_rows, N, nblk;
  int link;
  float pos_off[3], quat_off[4];
  float min_range, max_range;
  unsigned flags;
  unsigned long long skip;
  const float* dirs;
  const long long* env_idx;
  float *distance, *points, *normal;
  int32_t* geom;
};

// the workgroup's 3 x n floats, staged in `st` from float `pad` on (pad = the 16-byte phase of `out`), to global memory
__device__ __forceinline__ void store_span(float* out, const float* st, int pad, int nf, int tid) {
  float* const base = out - pad;  // 16-byte aligned
  const int c = tid;              // (pad + nf + 3) / 4 <= 193 chunks: one pass
  const int lo = 4 * c, hi = lo + 4;
  if (lo >= pad + nf || hi <= pad) return;
  if (lo >= pad && hi <= pad + nf) {
    reinterpret_cast<f4*>(base)[c] = *reinterpret_cast<const f4*>(st + lo);
  } else {
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (lo + k >= pad && lo + k < pad + nf) base[lo + k] = st[lo + k];
  }
}

__global__ __launch_bounds__(RAY_TPB) void mir_ray_kernel(RayArgs a) {
  __shared__ f4 rec4[MIR_MAX_GEOM * RAY_REC / 4];
  __shared__ f4 stage4[(3 * RAY_TPB + 4) / 4];
  __shared__ float hdr[16];  // [0] list length, [1..3] sensor origin (world), [4..12] R_s row-major
  float* const rec = reinterpret_cast<float*>(rec4);
  float* const stage = reinterpret_cast<float*>(stage4);
  const int tid = threadIdx.x;
  const int row = blockIdx.x / a.nblk, blk = blockIdx.x - row * a.nblk;
  int env = a.env_idx ? (int)a.env_idx[row] : row;
  env = env < 0 ? 0 : (env >= a.B ? a.B - 1 : env);  // (an index outside the batch is clamped, as in mir_link_kinematics)
  const bool world_out = (a.flags & MIR_RAY_POINTS_WORLD) != 0;

  if (tid < 64) {  // ---- prologue: wave 0, lane = geom
    const RayTab* __restrict__ t = a.tab;
    const int ng = t->ngeom;
    const bool isg = tid < ng;
    const int g = isg ? tid : 0;
    const float* const pe = a.poses + (size_t)env * 2 * a.pst * 4;
    // sensor frame in the world: o_s = o_link + R_link pos_offset, q_s = q_link (x) quat_offset
    V3 ol = v3(0, 0, 0);
    Q4 ql = Q4{1, 0, 0, 0};
    if (a.link > 0) {
      ol = ld3(pe + a.link * 4);
      ql = ld4(pe + (a.pst + a.link) * 4);
    }
    const V3 os = ol + qrot(ql, v3(a.pos_off[0], a.pos_off[1], a.pos_off[2]));
    const M3 Rs = q2m(qnormalize(qmul(ql, Q4{a.quat_off[0], a.quat_off[1], a.quat_off[2], a.quat_off[3]})));
    // geom frame in the world: c = xpos + R(xquat) g_pos, q = xquat (x) g_quat
    const int b = t->g[g].body;
    const V3 xp = ld3(pe + b * 4);
    const Q4 xq = ld4(pe + (a.pst + b) * 4);
    const V3 c = xp + qrot(xq, ld3(t->g[g].pos));
    const M3 Rg = q2m(qnormalize(qmul(xq, ld4(t->g[g].quat))));
    const V3 ax0 = mcol(Rg, 0), ax1 = mcol(Rg, 1), ax2 = mcol(Rg, 2);  // world axes of the geom
    const V3 rel = os - c;
    const V3 o = v3(dot(ax0, rel), dot(ax1, rel), dot(ax2, rel));
    const V3 s0 = mcol(Rs, 0), s1 = mcol(Rs, 1), s2 = mcol(Rs, 2);
    const int type = t->g[g].type;
    const float sx = t->g[g].size[0], sy = t->g[g].size[1], sz = t->g[g].size[2];
    const int p0 = t->g[g].p0, np = t->g[g].np;
    bool inside = false, far = false;
    if (type == MIR_GEOM_PLANE) {
      far = fabsf(o.z) > a.max_range;
    } else {
      far = sqrtf(dot(rel, rel)) - t->g[g].rad > a.max_range;
      if (type == MIR_GEOM_BOX) {
        inside = fabsf(o.x) <= sx && fabsf(o.y) <= sy && fabsf(o.z) <= sz;
      } else if (type == MIR_GEOM_HULL) {
        inside = true;
        for (int p = 0; p < np; p++) {
          const float* pl = a.planes + 4 * (p0 + p);
          if (pl[0] * o.x + pl[1] * o.y + pl[2] * o.z - pl[3] > 0.0f) inside = false;
        }
      } else {  // sphere = capsule with hl = 0
        const float hl = type == MIR_GEOM_CAPSULE ? sy : 0.0f;
        const float dz = o.z - fminf(fmaxf(o.z, -hl), hl);
        inside = o.x * o.x + o.y * o.y + dz * dz <= sx * sx;
      }
    }
    const bool keep = isg && !((a.skip >> g) & 1ull) && !inside && !far;
    const unsigned long long m = __ballot(keep);
    if (keep) {
      const int slot = __popcll(m & ((1ull << tid) - 1ull));
      float* r = rec + slot * RAY_REC;
      const float hl = type == MIR_GEOM_CAPSULE ? sy : 0.0f;
      r[0] = __int_as_float(type); r[1] = __int_as_float(g); r[2] = sx; r[3] = type == MIR_GEOM_BOX ? sy : hl;
      r[4] = sz; r[5] = o.x; r[6] = o.y; r[7] = o.z;
      // M: d_g = M d_s, row i = (ax_i . s_0, ax_i . s_1, ax_i . s_2)
      r[8] = dot(ax0, s0); r[9] = dot(ax0, s1); r[10] = dot(ax0, s2);
      r[11] = dot(ax1, s0); r[12] = dot(ax1, s1); r[13] = dot(ax1, s2);
      r[14] = dot(ax2, s0); r[15] = dot(ax2, s1); r[16] = dot(ax2, s2);
      // the axes a geom-frame normal is written in: the world's, or the sensor's (M^T)
      r[17] = world_out ? ax0.x : r[8];  r[18] = world_out ? ax0.y : r[9];  r[19] = world_out ? ax0.z : r[10];
      r[20] = world_out ? ax1.x : r[11]; r[21] = world_out ? ax1.y : r[12]; r[22] = world_out ? ax1.z : r[13];
      r[23] = world_out ? ax2.x : r[14]; r[24] = world_out ? ax2.y : r[15]; r[25] = world_out ? ax2.z : r[16];
      r[26] = __int_as_float(p0); r[27] = __int_as_float(np);
    }
    if (tid == 0) {
      hdr[0] = __int_as_float(__popcll(m));
      hdr[1] = os.x; hdr[2] = os.y; hdr[3] = os.z;
      hdr[4] = Rs.r0.x; hdr[5] = Rs.r0.y; hdr[6] = Rs.r0.z;
      hdr[7] = Rs.r1.x; hdr[8] = Rs.r1.y; hdr[9] = Rs.r1.z;
      hdr[10] = Rs.r2.x; hdr[11] = Rs.r2.y; hdr[12] = Rs.r2.z;
    }
  }
  __syncthreads();

  // ---- my ray
  const int n_here = a.N - blk * RAY_TPB < RAY_TPB ? a.N - blk * RAY_TPB : RAY_TPB;
  const bool valid = tid < n_here;
  const int ray = blk * RAY_TPB + (valid ? tid : n_here - 1);
  const V3 draw = ld3(a.dirs + (size_t)ray * 3);
  const float len2 = dot(draw, draw);
  const bool zero = !(len2 > 0.0f);
  const V3 d = zero ? v3(0, 0, 0) : (1.0f / sqrtf(len2)) * draw;
  const int count = __builtin_amdgcn_readfirstlane(__float_as_int(hdr[0]));
  float best = INFINITY;
  int bestk = -1;
  V3 bn = v3(0, 0, 0);  // normal of the best hit, geom frame
  for (int k = 0; k < count; k++) {
    const float* r = rec + k * RAY_REC;
    const int type = __builtin_amdgcn_readfirstlane(__float_as_int(r[0]));
    const V3 o = v3(r[5], r[6], r[7]);
    const V3 dg = v3(r[8] * d.x + r[9] * d.y + r[10] * d.z, r[11] * d.x + r[12] * d.y + r[13] * d.z, r[14] * d.x + r[15] * d.y + r[16] * d.z);
    float t = INFINITY;
    V3 n = v3(0, 0, 0);
    if (type == MIR_GEOM_PLANE) {  // z = 0 of the geom frame, two-sided
      const float tp = -o.z / dg.z;
      if (dg.z != 0.0f && tp > 0.0f) t = tp;
      n = v3(0, 0, o.z >= 0.0f ? 1.0f : -1.0f);
    } else if (type == MIR_GEOM_BOX) {  // slabs (the origin is outside)
      const float h[3] = {r[2], r[3], r[4]}, oo[3] = {o.x, o.y, o.z}, dd[3] = {dg.x, dg.y, dg.z};
      float tn = -INFINITY, tf = INFINITY;
      int kn = 0;
#pragma unroll
      for (int i = 0; i < 3; i++) {
        const float inv = 1.0f / dd[i];
        const float t1 = (-h[i] - oo[i]) * inv, t2 = (h[i] - oo[i]) * inv;
        float lo = fminf(t1, t2), hi = fmaxf(t1, t2);
        if (dd[i] == 0.0f) {  // parallel to the slab: inside it or never
          const bool out = fabsf(oo[i]) > h[i];
          lo = out ? INFINITY : -INFINITY;
          hi = out ? -INFINITY : INFINITY;
        }
        if (lo > tn) { tn = lo; kn = i; }
        tf = fminf(tf, hi);
      }
      if (tn <= tf && tn > 0.0f) t = tn;
      const float sg = (kn == 0 ? dg.x : (kn == 1 ? dg.y : dg.z)) > 0.0f ? -1.0f : 1.0f;
      n = v3(kn == 0 ? sg : 0.0f, kn == 1 ? sg : 0.0f, kn == 2 ? sg : 0.0f);
    } else if (type == MIR_GEOM_HULL) {  // half-space clipping against the face planes
      const int p0 = __builtin_amdgcn_readfirstlane(__float_as_int(r[26])), np = __builtin_amdgcn_readfirstlane(__float_as_int(r[27]));
      float tn = -INFINITY, tf = INFINITY;
      for (int p = 0; p < np; p++) {
        const float* pl = a.planes + 4 * (p0 + p);
        const float px = pl[0], py = pl[1], pz = pl[2], pd = pl[3];
        const float den = px * dg.x + py * dg.y + pz * dg.z;
        const float dist = px * o.x + py * o.y + pz * o.z - pd;
        const float tp = -dist / den;
        if (den < 0.0f) {
          if (tp > tn) { tn = tp; n = v3(px, py, pz); }
        } else if (den > 0.0f) {
          tf = fminf(tf, tp);
        } else if (dist > 0.0f) {
          tn = INFINITY;
        }
      }
      if (tn <= tf && tn > 0.0f) t = tn;
    } else {  // capsule about |z| <= hl (sphere: hl = 0): the two end spheres and the lateral surface
      const float rad = r[2], hl = r[3], r2 = rad * rad;
#pragma unroll
      for (int e = 0; e < 2; e++) {
        if (e == 1 && hl == 0.0f) break;
        const V3 oc = v3(o.x, o.y, o.z + (e == 0 ? -hl : hl));
        const float bb = dot(oc, dg);
        const V3 cr = cross(oc, dg);
        const float disc = r2 - dot(cr, cr);
        const float ts = -bb - sqrtf(fmaxf(disc, 0.0f));
        if (disc >= 0.0f && bb < 0.0f && ts < t) t = ts;
      }
      const float c2 = dg.x * dg.x + dg.y * dg.y, ac = o.x * o.x + o.y * o.y - r2;
      if (ac > 0.0f && hl > 0.0f && c2 > 0.0f) {
        const float bb = o.x * dg.x + o.y * dg.y, cz = o.x * dg.y - o.y * dg.x;
        const float disc = r2 * c2 - cz * cz;
        const float tl = (-bb - sqrtf(fmaxf(disc, 0.0f))) / c2;
        if (disc >= 0.0f && bb < 0.0f && fabsf(o.z + tl * dg.z) <= hl && tl < t) t = tl;
      }
      if (t < INFINITY) {
        const V3 p = o + t * dg;
        const float inv = 1.0f / rad;
        n = inv * v3(p.x, p.y, p.z - fminf(fmaxf(p.z, -hl), hl));
      }
      if (!(t > 0.0f)) t = INFINITY;
    }
    if (!zero && t < best) { best = t; bestk = k; bn = n; }  // (strict: a tie stays with the lower geom index)
  }
  const bool hit = bestk >= 0 && best <= a.max_range;
  const float dist = fminf(fmaxf(hit ? best : a.max_range, a.min_range), a.max_range);
  const size_t cell = (size_t)row * a.N + ray;
  if (valid) {
    if (a.distance) a.distance[cell] = dist;
    if (a.geom) a.geom[cell] = hit ? __float_as_int(rec[(bestk < 0 ? 0 : bestk) * RAY_REC + 1]) : -1;
  }
  const size_t span0 = ((size_t)row * a.N + (size_t)blk * RAY_TPB) * 3;
  const int nf = 3 * n_here;
  if (a.points) {  // (uniform over the launch)
    V3 p = dist * d;
    if (world_out) {
      p = v3(hdr[1] + hdr[4] * p.x + hdr[5] * p.y + hdr[6] * p.z, hdr[2] + hdr[7] * p.x + hdr[8] * p.y + hdr[9] * p.z,
             hdr[3] + hdr[10] * p.x + hdr[11] * p.y + hdr[12] * p.z);
    }
    float* const out = a.points + span0;
    const int pad = (int)(((uintptr_t)out >> 2) & 3);
    if (valid) { stage[pad + 3 * tid] = p.x; stage[pad + 3 * tid + 1] = p.y; stage[pad + 3 * tid + 2] = p.z; }
    __syncthreads();
    store_span(out, stage, pad, nf, tid);
    __syncthreads();
  }
  if (a.normal) {
    V3 nn = v3(0, 0, 0);
    if (hit) {
      const float* r = rec + bestk * RAY_REC + 17;  // columns = the geom's axes in the output frame
      nn = v3(r[0] * bn.x + r[3] * bn.y + r[6] * bn.z, r[1] * bn.x + r[4] * bn.y + r[7] * bn.z, r[2] * bn.x + r[5] * bn.y + r[8] * bn.z);
    }
    float* const out = a.normal + span0;
    const int pad = (int)(((uintptr_t)out >> 2) & 3);
    if (valid) { stage[pad + 3 * tid] = nn.x; stage[pad + 3 * tid + 1] = nn.y; stage[pad + 3 * tid + 2] = nn.z; }
    __syncthreads();
    store_span(out, stage, pad, nf, tid);
  }
}

// ---- the geometry table, once per handle: geoms as the compiled model holds them (float32), hull face planes by brute force over
// vertex triples (<= 32 vertices, <= 60 faces: a triple is a face when every vertex lies on one side of its plane)
int build_tab(MirScene* h) {
  RayTab tab;
  memset(&tab, 0, sizeof tab);
  std::vector<float> planes;
  const bool k16 = h->kernel == 16;
  tab.ngeom = h->ngeom;
  for (int g = 0; g < h->ngeom; g++) {
    RayGeom& r = tab.g[g];
    r.type = k16 ? h->hm.g_type[g] : h->hm64.g_type[g];
    r.body = k16 ? h->hm.g_body[g] : h->hm64.g_body[g];
    for (int k = 0; k < 3; k++) {
      r.size[k] = k16 ? h->hm.g_size[g][k] : h->hm64.g_size[g][k];
      r.pos[k] = k16 ? h->hm.g_pos[g][k] : h->hm64.g_pos[g][k];
    }
    for (int k = 0; k < 4; k++) r.quat[k] = k16 ? h->hm.g_quat[g][k] : h->hm64.g_quat[g][k];
    double rad = 0.0;
    if (r.type == MIR_GEOM_BOX) rad = std::sqrt((double)r.size[0] * r.size[0] + (double)r.size[1] * r.size[1] + (double)r.size[2] * r.size[2]);
    else if (r.type == MIR_GEOM_SPHERE) rad = r.size[0];
    else if (r.type == MIR_GEOM_CAPSULE) rad = (double)r.size[0] + r.size[1];
    else if (r.type == MIR_GEOM_HULL) {
      const int v0 = (int)r.size[0], nv = (int)r.size[1];
      const int pool = k16 ? K16_MAX_VERT : MIR_MAX_VERT;
      if (v0 < 0 || nv < 0 || nv > MIR_MAX_HULL_VERT || v0 + nv > pool) return mir_set_error(MIR_E_INVALID, "mir_raycast: a hull's vertices lie outside the pool");
      double v[MIR_MAX_HULL_VERT][3], scale = 0.0;
      for (int i = 0; i < nv; i++)
        for (int k = 0; k < 3; k++) {
          v[i][k] = k16 ? h->hm.hverts[v0 + i][k] : h->hm64.hverts[v0 + i][k];
          scale = std::fmax(scale, std::fabs(v[i][k]));
        }
      for (int i = 0; i < nv; i++) rad = std::fmax(rad, std::sqrt(v[i][0] * v[i][0] + v[i][1] * v[i][1] + v[i][2] * v[i][2]));
      const double tol = 1e-6 * scale;
      r.p0 = (int)(planes.size() / 4);
      bool volume = false;
      for (int i = 0; i < nv; i++)
        for (int j = i + 1; j < nv; j++)
          for (int k = j + 1; k < nv; k++) {
            const double e1[3] = {v[j][0] - v[i][0], v[j][1] - v[i][1], v[j][2] - v[i][2]}, e2[3] = {v[k][0] - v[i][0], v[k][1] - v[i][1], v[k][2] - v[i][2]};
            double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
            const double len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
            if (!(len > 1e-9 * scale * scale)) continue;  // (collinear)
            for (int c = 0; c < 3; c++) n[c] /= len;
            double d = n[0] * v[i][0] + n[1] * v[i][1] + n[2] * v[i][2], smin = 0.0, smax = 0.0;
            for (int m = 0; m < nv; m++) {
              const double s = n[0] * v[m][0] + n[1] * v[m][1] + n[2] * v[m][2] - d;
              smin = std::fmin(smin, s);
              smax = std::fmax(smax, s);
            }
            if (smax > tol && smin < -tol) continue;  // vertices on both sides: no face
            if (smax <= tol && smin >= -tol) continue;  // every vertex in this plane: a flat hull, no volume from this triple
            volume = true;
            if (smax > tol) { for (int c = 0; c < 3; c++) n[c] = -n[c]; d = -d; }
            bool dup = false;  // (another triple of the same face)
            for (size_t p = (size_t)r.p0 * 4; p < planes.size() && !dup; p += 4)
              dup = n[0] * planes[p] + n[1] * planes[p + 1] + n[2] * planes[p + 2] > 1.0 - 1e-9 && std::fabs(d - planes[p + 3]) <= tol;
            if (dup) continue;
            planes.push_back((float)n[0]); planes.push_back((float)n[1]); planes.push_back((float)n[2]); planes.push_back((float)d);
          }
      r.np = (int)(planes.size() / 4) - r.p0;
      if (!volume || r.np < 4) return mir_set_error(MIR_E_INVALID, "mir_raycast: a hull geom has no volume (its vertices lie in one plane)");
    }
    r.rad = (float)(rad * (1.0 + 1e-6));
  }
  tab.nplane = (int)(planes.size() / 4);
  const size_t bytes = sizeof(RayTab) + (planes.size() + 4) * sizeof(float);
  void* dev = nullptr;
  hipError_t e = hipMalloc(&dev, bytes);
  if (e == hipSuccess) e = hipMemcpy(dev, &tab, sizeof tab, hipMemcpyHostToDevice);
  if (e == hipSuccess && !planes.empty()) e = hipMemcpy(static_cast<char*>(dev) + sizeof tab, planes.data(), planes.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    if (dev) (void)hipFree(dev);
    return mir_set_error(MIR_E_HIP, hipGetErrorString(e));
  }
  h->ray_tab = dev;
  return MIR_OK;
}

}  // namespace

static_assert(sizeof(RayTab) % 16 == 0, "the planes behind the table are 16-byte rows");

extern "C" int mir_ray_query_sizeof(void) { return (int)sizeof(MirRayQuery); }

extern "C" int mir_raycast(MirHandle h, const MirRayQuery* q, const float* dirs, const int64_t* env_idx, int32_t n_rows, float* distance,
                           float* points, int32_t* geom, float* normal, void* stream) {
  if (!h || !q || !dirs) return mir_set_error(MIR_E_INVALID, "mir_raycast: null argument");
  if (q->struct_size != (int32_t)sizeof(MirRayQuery)) return mir_set_error(MIR_E_INVALID, "mir_raycast: struct_size is not sizeof(MirRayQuery)");
  if (q->n_rays < 1) return mir_set_error(MIR_E_INVALID, "mir_raycast: n_rays < 1");
  if (q->link_body < 0 || q->link_body >= h->nbody) return mir_set_error(MIR_E_INVALID, "mir_raycast: link out of range");
  if (!std::isfinite(q->min_range) || !std::isfinite(q->max_range) || !(q->min_range >= 0.0f) || !(q->min_range < q->max_range))
    return mir_set_error(MIR_E_INVALID, "mir_raycast: ranges must be finite with 0 <= min_range < max_range");
  if (q->flags & ~MIR_RAY_POINTS_WORLD) return mir_set_error(MIR_E_INVALID, "mir_raycast: unknown flag bit");
  if (h->ngeom < 64 && (q->skip_geoms >> h->ngeom)) return mir_set_error(MIR_E_INVALID, "mir_raycast: skip_geoms names a geom at or above ngeom");
  double qn = 0.0;
  for (int k = 0; k < 4; k++) qn += (double)q->quat_offset[k] * q->quat_offset[k];
  for (int k = 0; k < 3; k++)
    if (!std::isfinite(q->pos_offset[k])) return mir_set_error(MIR_E_INVALID, "mir_raycast: pos_offset is not finite");
  if (!std::isfinite(qn) || !(qn > 1e-24)) return mir_set_error(MIR_E_INVALID, "mir_raycast: quat_offset has no direction");
  if (h->pending) return mir_set_error(MIR_E_INVALID, "mir_raycast: a step is pending (mir_step_end first)");
  if (env_idx && n_rows < 0) return mir_set_error(MIR_E_INVALID, "mir_raycast: negative n_rows");
  const long long R = env_idx ? n_rows : h->B, N = q->n_rays;
  const long long nblk = (N + RAY_TPB - 1) / RAY_TPB;
  if (R * N > 0x7fffffffLL || R * nblk > 0x7fffffffLL) return mir_set_error(MIR_E_CAPACITY, "mir_raycast: rows x rays reaches 2^31");
  DeviceGuard guard(h->device);  // (the table's allocation and the pose refresh, too)
  int rc = MIR_OK;
  do {
    if (h->ray_state == 0) h->ray_state = (rc = build_tab(h)) == MIR_OK ? 1 : (rc == MIR_E_INVALID ? -1 : 0);
    else if (h->ray_state < 0) rc = mir_set_error(MIR_E_INVALID, "mir_raycast: a hull geom has no volume (its vertices lie in one plane)");
    if (rc != MIR_OK) break;
    if (R == 0 || (!distance && !points && !geom && !normal)) break;  // (nothing asked for)
    // link poses: the rasteriser's pose cache, refreshed when the state has moved since it was written
    if (!h->poses_current && (rc = mir_refresh_poses(h, stream)) != MIR_OK) break;
    RayArgs a;
    memset(&a, 0, sizeof a);
    a.tab = static_cast<const RayTab*>(h->ray_tab);
    a.planes = reinterpret_cast<const float*>(static_cast<const char*>(h->ray_tab) + sizeof(RayTab));
    a.poses = h->poses; a.pst = h->pt.pst; a.B = h->B; a.n_rows = (int)R; a.N = (int)N; a.nblk = (int)nblk;
    a.link = q->link_body;
    const float s = (float)(1.0 / std::sqrt(qn));
    for (int k = 0; k < 3; k++) a.pos_off[k] = q->pos_offset[k];
    for (int k = 0; k < 4; k++) a.quat_off[k] = q->quat_offset[k] * s;
    a.min_range = q->min_range; a.max_range = q->max_range; a.flags = q->flags; a.skip = q->skip_geoms;
    a.dirs = dirs; a.env_idx = reinterpret_cast<const long long*>(env_idx);
    a.distance = distance; a.points = points; a.geom = geom; a.normal = normal;
    rc = launch_rows<RAY_TPB>(h, mir_ray_kernel, R * nblk, stream, a);
  } while (0);
  return rc;
}
