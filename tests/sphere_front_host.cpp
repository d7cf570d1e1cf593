// C entry points over the host half of gym-genesis_amd/csrc/mir_sphere_front.h for tests/test_sphere_front_cpu.py (built by
// `make sphere-front-host`): pack_probe_links and build_body_words on a model given as plain arrays, no HIP anywhere.
#include <string.h>

#include "mir_sphere_front.h"

namespace {
// the view build_body_words reads, over arrays indexed by body
struct FakeModel {
  const int32_t *par, *jt;
  int parent(int b) const { return par[b]; }
  int jtype(int b) const { return jt[b]; }
};
// a refusal as the kernels' entry points get it: the code, and the text into `what` (128 bytes)
struct Refuse {
  char* what;
  int operator()(int code, const char* text) const {
    strncpy(what, text, 127);
    what[127] = 0;
    return code;
  }
};
}  // namespace

extern "C" {

// body (MIR_MAX_BODY words, zeroed here as the entry points zero their arguments); planned: MIR_MAX_BODY bytes or null
int sphere_front_body_words(int nbody, const int32_t* parent, const int32_t* jtype, int fk, const uint8_t* planned, uint32_t* body, int32_t* depth_max,
                            char* what) {
  bool pl[MIR_MAX_BODY];
  for (int b = 0; b < MIR_MAX_BODY; b++) { pl[b] = planned && planned[b]; body[b] = 0; }
  what[0] = 0;
  int dm = -1;
  const int rc = build_body_words(FakeModel{parent, jtype}, nbody, fk != 0, planned ? pl : nullptr, body, dm, Refuse{what});
  *depth_max = dm;
  return rc;
}

int sphere_front_pack_links(const int32_t* probe_link, int n, int nbody, uint8_t* link, char* what) {
  what[0] = 0;
  return pack_probe_links(probe_link, n, nbody, link, Refuse{what});
}

}  // extern "C"
