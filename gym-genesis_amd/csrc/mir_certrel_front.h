// mir_certrel_front.h — the host-side checks of mir_certify_path_self / mir_certify_path_carry and the scalar part of the relative-motion
// rule (mir_cert.hip, the instantiations with SELF or CARRY; include/mirigid.h, "certified clearance: self and carried object"): plain C++, no HIP in it, so that
// tests/certrel_host.cpp builds it with g++ (`make certrel-host`) and tests/test_certrel_cpu.py walks every refusal and compares the
// branch sums, the pair speed bound and the LCA table with the NumPy port without a device.  The kernel calls the same scalar functions
// (CERT_HD makes them device functions under hipcc); certrel_branch() below is the same walk over arrays, for the host.
// It stands on mir_cert_front.h (the bisection, the leaf tests, the chain recurrences).
// Every product stands in a statement of its own, so that no build fuses it with the sum behind it.
// A refusal is `refuse(code, text)`: the caller's, which names the entry point.  The order of the checks and their texts are part of
// the interface.
#pragma once
#include "mir_cert_front.h"

namespace {

constexpr int CERTREL_NONE = 0xff;   // the LCA table: the two bodies share no chain (or one of them is the world)
constexpr int CERTREL_STEPS = 17;    // a chain holds at most 16 bodies: 0 .. 16 of them enter a branch sum

// what the two entry points were handed beyond mir_certify_path's own arguments, as far as these checks read it
struct CertRelCall {
  bool carry_form;  // mir_certify_path_carry (sq and cq nullable, not both); else mir_certify_path_self (sq required, no cq)
  const void *sq, *cq, *grasp, *grasp_used;
  const void *seg_self_lower, *seg_self_upper, *row_self_lower, *row_self_upper;
};

// behind cert_check() and in front of the planner's front end
template <class Refuse>
static int certrel_check(const CertRelCall& c, Refuse refuse) {
  if (!c.carry_form && !c.sq) return refuse(MIR_E_INVALID, "null self query");
  if (c.carry_form && !c.sq && !c.cq) return refuse(MIR_E_INVALID, "neither a MirSelfQuery nor a MirCarryQuery (mir_certify_path judges the scene test alone)");
  if (!c.sq && (c.seg_self_lower || c.seg_self_upper || c.row_self_lower || c.row_self_upper))
    return refuse(MIR_E_INVALID, "seg_self_lower / seg_self_upper / row_self_lower / row_self_upper without a MirSelfQuery");
  if (!c.cq && c.grasp) return refuse(MIR_E_INVALID, "grasp without a MirCarryQuery");
  if (!c.cq && c.grasp_used) return refuse(MIR_E_INVALID, "grasp_used without a MirCarryQuery");
  return MIR_OK;
}

// the LDS of one row: `fixed` bytes whatever the call, 4 per probe of the scene test (v_i), 4 per sphere (cn_i), and with a self query
// 16 per sphere (the sphere list)
static inline long long certrel_lds_bytes(long long fixed, long long n_probes, long long n_spheres, bool self) {
  return fixed + 4 * n_probes + 4 * n_spheres + (self ? 16 * n_spheres : 0);
}
template <class Refuse>
static int certrel_check_lds(long long fixed, long long n_probes, long long n_spheres, bool self, Refuse refuse) {
  if (certrel_lds_bytes(fixed, n_probes, n_spheres, self) > 65536)
    return refuse(MIR_E_CAPACITY, "the speed bounds and the sphere list do not fit 64 KB of LDS (n_probes, n_probes + n_extra)");
  return MIR_OK;
}

// ---- the rule.  One step of the walk a, parent(a), ... towards the LCA: body k with its planned dof (kind: 0 none, 1 revolute, 2
// prismatic; adq = |dq_k|) adds to the three non-negative sums of the branch
CERT_HD float certrel_step_a(float dA, int kind, float adq) { return dA + (kind == 1 ? adq : 0.0f); }
CERT_HD float certrel_step_sb(float dSB, int kind, float adq, float s_link, float s_body) {
  const float w = s_link - s_body;
  const float t = adq * w;
  return dSB + (kind == 1 ? t : 0.0f);
}
CERT_HD float certrel_step_p(float dP, int kind, float adq, float axis_len) {
  const float t = adq * axis_len;
  return dP + (kind == 2 ? t : 0.0f);
}

// rel(i, c) = (cn_i dA + dSB) + dP: how fast sphere i, at distance <= cn_i from its link's origin, moves relative to body c's frame
CERT_HD float certrel_rel(float cn, float dA, float dSB, float dP) {
  const float t = cn * dA;
  const float u = t + dSB;
  return u + dP;
}

// v_ij = (rel(i, c) + rel(j, c)) 1.0001, never below 0: the bound on |d s_ij / dt|
CERT_HD float certrel_speed(float rel_i, float rel_j) {
  const float x = rel_i + rel_j;
  const float v = x * 1.0001f;
  return v > 0.0f ? v : 0.0f;
}

// the bodies that enter rel(., c) for a sphere on a link at chain depth `depth` (-1: the world) when the table says `lca`
CERT_HD int certrel_steps(int depth, int lca) { return lca == CERTREL_NONE ? depth + 1 : depth - lca; }

// cn of a sphere on the carried body: |p_G| + |c_i| (the rotation of the grasp does not enter)
CERT_HD float certrel_cn_carried(float grasp_len, float cn) { return grasp_len + cn; }

// one evaluation's pair value: min(s_ij, self_max) - hw v_ij
CERT_HD float certrel_pair_bound(float s, float self_max, float hw, float v) {
  const float cap = s < self_max ? s : self_max;
  const float reach = hw * v;
  return cap - reach;
}

// the status of a segment with both tests (self: a MirSelfQuery was given); the order of mir_certify_path: without `self` it is
// cert_status().  The one the kernel calls, in every instantiation
CERT_HD int certrel_status(bool not_finite, bool budget, bool depth, float lower, float upper, float margin, bool self, float lower_s, float upper_s,
                           float self_margin) {
  if (not_finite) return MIR_CERT_NOT_FINITE;
  if (budget) return MIR_CERT_BUDGET;
  if (upper < margin || (self && upper_s < self_margin)) return MIR_CERT_BLOCKED;
  if (depth) return MIR_CERT_DEPTH;
  return lower >= margin && (!self || lower_s >= self_margin) ? MIR_CERT_CLEAR : MIR_CERT_UNDECIDED;
}

// ---- host: the LCA table, nbody x nbody bytes (row stride nbody_stride): the chain depth of the lowest common ancestor-or-self of a and
// b, or CERTREL_NONE when they stand in different chains or one of them is the world.  parent[b], depth[b] (bodies above b in its chain:
// 0 starts one) as the body words hold them; a carried body counts as its attach link (carry_body < 0: none).
static inline void certrel_lca_table(int nbody, int stride, const int32_t* parent, const int32_t* depth, int carry_body, int carry_link, uint8_t* out) {
  for (int a = 0; a < nbody; a++)
    for (int b = 0; b < nbody; b++) {
      int x = a == carry_body ? carry_link : a, y = b == carry_body ? carry_link : b;
      int found = CERTREL_NONE;
      if (x > 0 && y > 0) {
        while (depth[x] > depth[y]) x = parent[x];
        while (depth[y] > depth[x]) y = parent[y];
        while (x != y && depth[x] > 0) {
          x = parent[x];
          y = parent[y];
        }
        if (x == y) found = depth[x];
      }
      out[a * stride + b] = (uint8_t)found;
    }
}

#ifndef __HIPCC__
// ---- the branch sums over arrays, for the host: walking from body a upward, out[3 t .. 3 t + 2] = (dA, dSB, dP) over the first t bodies
// of the walk, t = 0 .. depth[a] + 1 (the kernel's table row of a).  kind[b], adq[b], axis_len[b], S[b] as cert_chains() takes and gives them.
static void certrel_branch(int a, const int32_t* parent, const int32_t* depth, const int32_t* kind, const float* adq, const float* axis_len,
                           const float* S, float* out) {
  float dA = 0.0f, dSB = 0.0f, dP = 0.0f;
  out[0] = out[1] = out[2] = 0.0f;
  int k = a;
  for (int t = 0; a > 0 && t <= depth[a]; t++) {
    dA = certrel_step_a(dA, kind[k], adq[k]);
    dSB = certrel_step_sb(dSB, kind[k], adq[k], S[a], S[k]);
    dP = certrel_step_p(dP, kind[k], adq[k], axis_len[k]);
    out[3 * (t + 1)] = dA; out[3 * (t + 1) + 1] = dSB; out[3 * (t + 1) + 2] = dP;
    k = parent[k];
  }
}
#endif

}  // namespace
