// mir_self_body.h — what the self-collision test of the sphere model shares between mir_self.hip (mir_self_distance) and mir_plan.hip
// (mir_plan_path_self, mir_path_clearance_self); include/mirigid.h "self-collision", DESIGN.md "Self-collision".
//   device: the signed distance of two spheres of the world-frame sphere list, and the lowest one of a probe over the list;
//   host:   the checks of a MirSelfQuery.
// The sphere list is (centre xyz, radius) per probe in LDS, written by the wave that reads it (sphere_list_fill / sphere_store of
// mir_sphere_front.h, where the rest of what the two files share lives).  Included after mir_dev.h and mir_query.h.
#pragma once

namespace {

// s(i, j) = |c_i - c_j| - (r_i + r_j): symmetric in i and j bit for bit (the squares and the sum of the radii do not see the order).
// The root is the hardware's v_sqrt_f32 (within an ulp): the library routine wraps it in five more instructions that rescale
// denormals, and two centres closer than 1e-19 m are inside each other by their radii either way.
__device__ __forceinline__ float self_pair(float xi, float yi, float zi, float ri, float xj, float yj, float zj, float rj) {
  const float dx = xi - xj, dy = yi - yj, dz = zi - zj;
  return __builtin_amdgcn_sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx))) - (ri + rj);
}

// the lowest s(i, j) of probe i (this lane's) over the probes j = j0 .. n - 1 whose link is enabled against i's (bit link[j] of `mask`, the
// mask row of i's link), j ascending: the lower j keeps a tie.  j0 is a multiple of 64.  The list is walked in chunks of 64: every
// lane reads one sphere of the chunk and its link, and the inner loop hands sphere j to all lanes with v_readlane (j is wave-uniform),
// so that no memory access stands in it.  The loop is bound by its instruction count (the planner's LDS leaves one wave per SIMD,
// nothing overlaps it): TRACK says whether j is kept (mir_self_distance) or the value alone (the planner, which also starts at its
// own chunk: s is symmetric, so the pairs with j in an earlier chunk have been seen from the other side).  Called by whole waves (every lane is a source of
// the readlane).  -> the value (INFINITY: no pair is enabled) and its j (-1; TRACK only).
struct SelfBest {
  float best;
  int j;
};
__device__ __forceinline__ float lane_bcast(float v, int src) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src)); }
template <bool TRACK>
__device__ __forceinline__ SelfBest self_probe_min(const float* sph, const uint8_t* link, int n, int j0, int i, uint32_t mask, int lane) {
  const float xi = sph[4 * i], yi = sph[4 * i + 1], zi = sph[4 * i + 2], ri = sph[4 * i + 3];
  SelfBest w{INFINITY, -1};
  for (int base = j0; base < n; base += 64) {
    const int mine = base + lane < n ? base + lane : n - 1;
    const float xm = sph[4 * mine], ym = sph[4 * mine + 1], zm = sph[4 * mine + 2], rm = sph[4 * mine + 3];
    const int lm = link[mine];
    const int cnt = n - base < 64 ? n - base : 64;
    for (int k = 0; k < cnt; k++) {
      const float s = self_pair(xi, yi, zi, ri, lane_bcast(xm, k), lane_bcast(ym, k), lane_bcast(zm, k), lane_bcast(rm, k));
      const bool on = (mask >> __builtin_amdgcn_readlane(lm, k)) & 1u;
      if constexpr (TRACK) {
        if (on && s < w.best) {
          w.best = s;
          w.j = base + k;
        }
      } else {
        w.best = fminf(w.best, on ? s : INFINITY);
      }
    }
  }
  return w;
}

// ---- host: the refusals of a MirSelfQuery (none of them launches anything)
static int self_query_check(MirHandle h, const MirSelfQuery* sq, const char* who) {
  if (!sq) return query_error(MIR_E_INVALID, who, "null self query");
  if (sq->struct_size != (int32_t)sizeof(MirSelfQuery)) return query_error(MIR_E_INVALID, who, "struct_size is not sizeof(MirSelfQuery)");
  if (sq->n_extra < 0) return query_error(MIR_E_INVALID, who, "n_extra < 0");
  if (!std::isfinite(sq->self_margin) || !(sq->self_margin >= 0.0f)) return query_error(MIR_E_INVALID, who, "self_margin must be finite and >= 0");
  if (!std::isfinite(sq->max_distance) || !(sq->max_distance > sq->self_margin))
    return query_error(MIR_E_INVALID, who, "the self query's max_distance must be finite and > self_margin");
  if (sq->flags) return query_error(MIR_E_INVALID, who, "unknown flag bit in the self query");
  for (int a = 0; a < MIR_MAX_BODY; a++) {
    const uint32_t m = sq->link_mask[a];
    if ((m >> a) & 1u) return query_error(MIR_E_INVALID, who, "link_mask has a diagonal bit (a link against itself)");
    if (h->nbody < 32 && ((m >> h->nbody) || (a >= h->nbody && m))) return query_error(MIR_E_INVALID, who, "link_mask names a body at or above nbody");
    for (int b = 0; b < MIR_MAX_BODY; b++)
      if (((m >> b) & 1u) != ((sq->link_mask[b] >> a) & 1u)) return query_error(MIR_E_INVALID, who, "link_mask is not symmetric");
  }
  return MIR_OK;
}

}  // namespace
