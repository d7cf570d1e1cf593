// C entry points over the two scene compilers (gym-genesis_amd/csrc/mir_compile.cpp, mir_compile64.cpp: no HIP in them) for
// tests/test_tree_cases_cpu.py (built by `make compile-host` with plain g++): which model a MirSceneSpec compiles for, no GPU anywhere.
#include <cstdint>
#include <cstring>

#include "mir_model.h"
#include "mir_model64.h"

extern "C" {

// the return code of the compiler of the 16-lane model (which = 16) or of the wave model (which = 64); err (256 bytes): the text of a refusal
int compile_host_rc(const MirSceneSpec* spec, int which, char* err) {
  HostConsts hc;
  err[0] = 0;
  if (which == 16) {
    DevModel* m = new DevModel;
    memset(m, 0, sizeof *m);
    const int rc = mir_compile_model(spec, m, &hc, err);
    delete m;
    return rc;
  }
  DevModel64* m = new DevModel64;
  memset(m, 0, sizeof *m);
  const int rc = mir_compile_model64(spec, m, &hc, err);
  delete m;
  return rc;
}

}  // extern "C"
