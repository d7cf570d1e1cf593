// mir_cert_front.h — the host-side checks of mir_certify_path and the scalar part of its rule (mir_cert.hip; include/mirigid.h,
// "certified clearance"): plain C++, no HIP in it, so that tests/cert_host.cpp builds it with g++ (`make cert-host`) and
// tests/test_cert_cpu.py walks every refusal and compares the dyadic successor, the status order, the chain-length recurrence and the
// speed bound with the NumPy port without a device.  The kernel calls the same scalar functions (CERT_HD makes them device functions
// under hipcc) with a body or a probe per lane; cert_chains() below is the same recurrence over arrays, for the host.
// Every product stands in a statement of its own, so that no build fuses it with the sum behind it.
// A refusal is `refuse(code, text)`: the caller's, which names the entry point.  The order of the checks and their texts are part of
// the interface.
#pragma once
#include <math.h>
#include <stdint.h>

#include "mirigid.h"

#ifdef __HIPCC__
#define CERT_HD __host__ __device__ __forceinline__
#else
#define CERT_HD static inline
#endif

namespace {

// what the entry point was handed, as far as these checks read it (the clearance side is checked by the planner's front end)
struct CertCall {
  bool handle;
  const MirCertQuery* q;
  const void *pq, *probes, *dof_qadr, *paths, *leaves;
};

template <class Refuse>
static int cert_check(const CertCall& c, Refuse refuse) {
  const MirCertQuery* const q = c.q;
  if (!c.handle || !q || !c.pq || !c.probes || !c.dof_qadr || !c.paths) return refuse(MIR_E_INVALID, "null argument");
  if (q->struct_size != (int32_t)sizeof(MirCertQuery)) return refuse(MIR_E_INVALID, "struct_size is not sizeof(MirCertQuery)");
  if (q->num_points < 2) return refuse(MIR_E_INVALID, "num_points < 2");
  if (q->max_depth < 0 || q->max_depth > MIR_CERT_MAX_DEPTH) return refuse(MIR_E_INVALID, "max_depth outside 0 .. 20");
  if (q->max_evaluations < 1) return refuse(MIR_E_INVALID, "max_evaluations < 1");
  if (q->max_leaves < 0) return refuse(MIR_E_INVALID, "max_leaves < 0");
  if (q->max_leaves > 0 && !c.leaves) return refuse(MIR_E_INVALID, "max_leaves > 0 without leaves");
  if (q->flags & ~(uint32_t)MIR_CERT_BRACKET) return refuse(MIR_E_INVALID, "unknown flag bit in MirCertQuery");
  if (!isfinite(q->tol)) return refuse(MIR_E_INVALID, "tol must be finite");
  if (!(isfinite(q->guard) && q->guard >= 0.0f)) return refuse(MIR_E_INVALID, "guard must be finite and >= 0");
  if (!(q->tol > q->guard)) return refuse(MIR_E_INVALID, "tol <= guard (the bracket could never close)");
  return MIR_OK;
}

// R x max(K x D, max_leaves x 3) elements must be addressable by 31 bits (behind the planner's front end, which yields R and D)
template <class Refuse>
static int cert_check_size(const MirCertQuery* q, long long R, int D, Refuse refuse) {
  const long long kd = (long long)q->num_points * D, lv = (long long)q->max_leaves * 3;
  const long long per_row = kd > lv ? kd : lv;
  if (R > 0 && per_row > 0x7fffffffLL / R) return refuse(MIR_E_CAPACITY, "rows x max(num_points x n_dofs, 3 max_leaves) beyond 2^31 - 1");
  return MIR_OK;
}

// ---- the rule.  Node (l, k) covers [k 2^-l, (k + 1) 2^-l]: its midpoint and its half-width, both exact in float32 for l <= 20
CERT_HD float cert_half(int l) { return ldexpf(1.0f, -(l + 1)); }
CERT_HD float cert_mid(int l, int k) { return ldexpf((float)(2 * k + 1), -(l + 1)); }

// the dyadic successor of an accepted leaf (depth first, left child first): true when the segment is tiled
CERT_HD bool cert_next(int* l, int* k) {
  while (*k & 1) {
    *k >>= 1;
    (*l)--;
  }
  if (*l == 0) return true;
  (*k)++;
  return false;
}

// the bound of a node from the wave's reductions: lo = min_i(d_i - hw v_i) - guard
CERT_HD float cert_lo(float min_bound, float guard) { return min_bound - guard; }

// the two leaf tests (step 4)
CERT_HD bool cert_leaf(float lo, float upper, float margin, float tol, bool bracket) {
  const float closed = upper - tol;
  return (!bracket && lo >= margin) || lo >= closed;
}

// the status of a segment (step 7); `budget` and `not_finite` as steps 5 and 6 set them, `depth`: a node at max_depth failed both tests
// (the scene test alone: certrel_status() of mir_certrel_front.h with self == false, which is what the kernel calls)
CERT_HD int cert_status(bool not_finite, bool budget, bool depth, float lower, float upper, float margin) {
  if (not_finite) return MIR_CERT_NOT_FINITE;
  if (budget) return MIR_CERT_BUDGET;
  if (upper < margin) return MIR_CERT_BLOCKED;
  if (depth) return MIR_CERT_DEPTH;
  return lower >= margin ? MIR_CERT_CLEAR : MIR_CERT_UNDECIDED;
}

// the chain-length recurrence (step 1) and the three sums of step 2, parent before child.  `root`: the body starts a chain (its
// parent is the world, or it is a free body).  kind: 0 not planned (or fixed), 1 planned revolute, 2 planned prismatic.
CERT_HD float cert_chain(bool root, float s_parent, float pos_len, float pris) {
  if (root) return 0.0f;
  const float t = s_parent + pos_len;
  return t + pris;
}
CERT_HD float cert_sum_a(bool root, float a_parent, int kind, float adq) { return (root ? 0.0f : a_parent) + (kind == 1 ? adq : 0.0f); }
CERT_HD float cert_sum_b(bool root, float b_parent, int kind, float adq, float s_body) {
  const float w = adq * s_body;
  return (root ? 0.0f : b_parent) + (kind == 1 ? w : 0.0f);
}
CERT_HD float cert_sum_p(bool root, float p_parent, int kind, float adq, float axis_len) {
  const float w = adq * axis_len;
  return (root ? 0.0f : p_parent) + (kind == 2 ? w : 0.0f);
}

// the speed bound of a probe at distance cn from the origin of its link: ((S + cn) A - B + P) 1.0001, never below 0
CERT_HD float cert_speed(float S, float cn, float A, float B, float P) {
  const float r = S + cn;
  const float t = r * A;
  const float w = t - B;
  const float x = w + P;
  const float v = x * 1.0001f;
  return v > 0.0f ? v : 0.0f;
}

#ifndef __HIPCC__
// ---- the recurrences over arrays, for the host: bodies 0 .. n - 1 with parents in front of their children; root[b], kind[b], pos_len[b],
// pris[b], adq[b] (|dq| of the body's planned dof, 0 without), axis_len[b] -> S, A, B, P (n each)
static void cert_chains(int n, const int32_t* parent, const int32_t* root, const int32_t* kind, const float* pos_len, const float* pris,
                        const float* adq, const float* axis_len, float* S, float* A, float* B, float* P) {
  S[0] = A[0] = B[0] = P[0] = 0.0f;
  for (int b = 1; b < n; b++) {
    const int p = parent[b];
    const bool rt = root[b] != 0;
    S[b] = cert_chain(rt, S[p], pos_len[b], pris[b]);
    A[b] = cert_sum_a(rt, A[p], kind[b], adq[b]);
    B[b] = cert_sum_b(rt, B[p], kind[b], adq[b], S[b]);
    P[b] = cert_sum_p(rt, P[p], kind[b], adq[b], axis_len[b]);
  }
}
#endif

}  // namespace
