// C entry points over gym-genesis_amd/csrc/mir_certrel_front.h for tests/test_certrel_cpu.py (built by `make certrel-host`): the host-side
// checks of mir_certify_path_self / mir_certify_path_carry with the call as plain arguments and the refusal's text into `what` (128
// bytes), and the scalar part of the relative-motion rule (the branch sums, rel, the pair speed bound, the pair value of an evaluation,
// the status order, the LCA table) as the kernel calls it.  No HIP anywhere.
#include <string.h>

#include "mir_certrel_front.h"

extern "C" {

// present: bit 0 sq, 1 cq, 2 grasp, 3 grasp_used, 4 seg_self_lower, 5 seg_self_upper, 6 row_self_lower, 7 row_self_upper
int certrel_host_check(int carry_form, unsigned present, char* what) {
  static const char some = 0;
  const auto ptr = [&](int bit) -> const void* { return ((present >> bit) & 1u) ? &some : nullptr; };
  const CertRelCall c{carry_form != 0, ptr(0), ptr(1), ptr(2), ptr(3), ptr(4), ptr(5), ptr(6), ptr(7)};
  what[0] = 0;
  return certrel_check(c, [&](int code, const char* text) {
    strncpy(what, text, 127);
    what[127] = 0;
    return code;
  });
}

long long certrel_host_lds_bytes(long long fixed, long long n_probes, long long n_spheres, int self) {
  return certrel_lds_bytes(fixed, n_probes, n_spheres, self != 0);
}
int certrel_host_check_lds(long long fixed, long long n_probes, long long n_spheres, int self, char* what) {
  what[0] = 0;
  return certrel_check_lds(fixed, n_probes, n_spheres, self != 0, [&](int code, const char* text) {
    strncpy(what, text, 127);
    what[127] = 0;
    return code;
  });
}

float certrel_host_rel(float cn, float dA, float dSB, float dP) { return certrel_rel(cn, dA, dSB, dP); }
float certrel_host_speed(float rel_i, float rel_j) { return certrel_speed(rel_i, rel_j); }
int certrel_host_steps(int depth, int lca) { return certrel_steps(depth, lca); }
float certrel_host_cn_carried(float grasp_len, float cn) { return certrel_cn_carried(grasp_len, cn); }
float certrel_host_pair_bound(float s, float self_max, float hw, float v) { return certrel_pair_bound(s, self_max, hw, v); }
int certrel_host_status(int not_finite, int budget, int depth, float lower, float upper, float margin, int self, float lower_s, float upper_s,
                        float self_margin) {
  return certrel_status(not_finite != 0, budget != 0, depth != 0, lower, upper, margin, self != 0, lower_s, upper_s, self_margin);
}
void certrel_host_lca(int nbody, const int32_t* parent, const int32_t* depth, int carry_body, int carry_link, uint8_t* out) {
  certrel_lca_table(nbody, nbody, parent, depth, carry_body, carry_link, out);
}
// the table row of body a: 3 (depth[a] + 2) floats
void certrel_host_branch(int a, const int32_t* parent, const int32_t* depth, const int32_t* kind, const float* adq, const float* axis_len,
                         const float* S, float* out) {
  certrel_branch(a, parent, depth, kind, adq, axis_len, S, out);
}
// S, A, B, P as the kernel forms them (cert_chains of mir_cert_front.h), for the branch sums' inputs
void certrel_host_chains(int n, const int32_t* parent, const int32_t* root, const int32_t* kind, const float* pos_len, const float* pris,
                         const float* adq, const float* axis_len, float* S, float* A, float* B, float* P) {
  cert_chains(n, parent, root, kind, pos_len, pris, adq, axis_len, S, A, B, P);
}

}  // extern "C"
