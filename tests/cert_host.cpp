// C entry points over gym-genesis_amd/csrc/mir_cert_front.h for tests/test_cert_cpu.py (built by `make cert-host`): the host-side
// checks of mir_certify_path with the call as plain arguments and the refusal's text into `what` (128 bytes), and the scalar part of
// the rule (the dyadic successor, the node's midpoint and half-width, the leaf tests, the status order, the chain-length recurrence and
// the speed bound) as the kernel calls it.  No HIP anywhere.
#include <string.h>

#include "mir_cert_front.h"

extern "C" {

int cert_host_query_sizeof(void) { return (int)sizeof(MirCertQuery); }

// present: bit 0 handle, 1 pq, 2 probes, 3 dof_qadr, 4 paths, 5 leaves
int cert_host_check(const MirCertQuery* q, unsigned present, long long rows, int n_dofs, char* what) {
  static const char some = 0;
  const auto ptr = [&](int bit) -> const void* { return ((present >> bit) & 1u) ? &some : nullptr; };
  const CertCall c{(present & 1u) != 0, q, ptr(1), ptr(2), ptr(3), ptr(4), ptr(5)};
  what[0] = 0;
  const auto refuse = [&](int code, const char* text) {
    strncpy(what, text, 127);
    what[127] = 0;
    return code;
  };
  const int rc = cert_check(c, refuse);
  return rc != MIR_OK ? rc : cert_check_size(q, rows, n_dofs, refuse);
}

float cert_host_half(int l) { return cert_half(l); }
float cert_host_mid(int l, int k) { return cert_mid(l, k); }
int cert_host_next(int* l, int* k) { return cert_next(l, k) ? 1 : 0; }
float cert_host_lo(float min_bound, float guard) { return cert_lo(min_bound, guard); }
int cert_host_leaf(float lo, float upper, float margin, float tol, int bracket) { return cert_leaf(lo, upper, margin, tol, bracket != 0) ? 1 : 0; }
int cert_host_status(int not_finite, int budget, int depth, float lower, float upper, float margin) {
  return cert_status(not_finite != 0, budget != 0, depth != 0, lower, upper, margin);
}
float cert_host_speed(float S, float cn, float A, float B, float P) { return cert_speed(S, cn, A, B, P); }
void cert_host_chains(int n, const int32_t* parent, const int32_t* root, const int32_t* kind, const float* pos_len, const float* pris,
                      const float* adq, const float* axis_len, float* S, float* A, float* B, float* P) {
  cert_chains(n, parent, root, kind, pos_len, pris, adq, axis_len, S, A, B, P);
}

}  // extern "C"
