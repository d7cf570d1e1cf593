// mir_host.h — what the host code of the step path shares between mir_api.hip (the C ABI, begin / go / end) and mir_exact.hip (the
// launches and waits of exact contacts): error plumbing, the launch arguments and the poller.  The device guard they and the query
// files take is in mir_guard.h.
#pragma once
#include <hip/hip_runtime.h>

#include "mir_guard.h"
#include "mir_scene.h"
#include "mir_step.h"

namespace mir_host {

// (implemented in mir_api.hip; the text goes to mir_last_error)
int set_err(int code, const char* fmt, const char* detail = "");
int hip_fail(hipError_t e, const char* what);
#define HIPCHK(call)                                   \
  do {                                                 \
    hipError_t _e = (call);                            \
    if (_e != hipSuccess) return hip_fail(_e, #call);  \
  } while (0)

using ::DeviceGuard;  // (mir_guard.h)

inline int check(MirHandle h) {
  if (!h) return set_err(MIR_E_INVALID, "null MirHandle");
  return MIR_OK;
}
int check_mask(MirScene* h);  // the sticky word of wrong early bytes (mir_api.hip)

// launch arguments common to both kernels
struct Outs {
  const float* action = nullptr;
  float *agent_pos = nullptr, *env_state = nullptr, *reward = nullptr;
  uint8_t* terminated = nullptr;
  uint8_t* term_host = nullptr;
  uint32_t *done_ticket = nullptr, *done_flag = nullptr;
  uint32_t done_seq = 0, term_tag = 0;
  float *out_M = nullptr, *out_bias = nullptr, *out_qas = nullptr, *out_qacc = nullptr, *out_xpos = nullptr, *out_xquat = nullptr;
  float* rows = nullptr;
  int row_stride = 0, mode = 0, n_steps = 1;
  long act_step = 0, rows_step = 0;
  AutoResetArgs ar = {nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0};
  bool diag = true;
  bool poses = false;  // 16-lane kernel: also write the link poses into h->poses (the rasteriser reads them)
  int kind = STEP_FULL;  // 16-lane kernel: which launch (StepKind, mir_step.h); STEP_FULL = a whole step, narrowed by mir_launch_step
  int exact = 0;       // 16-lane kernel: defer the envs with more candidate points than lanes (StepArgs::exact)
  int over_cap = 0;    // 16-lane kernel, STEP_LIST48 / STEP_HEAVY48 (StepArgs::over_cap)
  const int32_t* env_list = nullptr;  // 16-lane kernel, the kinds of step_reads_env_list: serve the envs env_list[0 .. nlist) (StepArgs::env_list)
  int nlist = 0;
  uint32_t* next_host = nullptr;      // 16-lane kernel, STEP_PRE48 (StepArgs::next_host)
  unsigned long long* prof = nullptr;  // 16-lane kernel only (debug)
  // contact force sensing (mir_contact_forces; StepArgs::cf_*)
  int32_t *cf_ncon = nullptr, *cf_ids = nullptr;
  uint8_t* cf_flags = nullptr;
  float *cf_geom = nullptr, *cf_force = nullptr, *cf_link = nullptr;
};
int launch(MirScene* h, const Outs& o, void* stream);  // (mir_api.hip)

// exact contacts (mir_exact.hip), called by mir_step_begin / mir_step_end / mir_destroy
int split_lists(MirScene* h, int* buf, int* nh_out);
int exact_finish(MirScene* h, int n, uint8_t* terminated_host);
void exact_destroy(MirScene* h);

/* The host's wait for words a launch stores into pinned memory.  `ready` is the caller's: it consumes what has arrived (its cursor
 * stands still at the first item that has not) and says whether everything has.  Between two looks: a pause; every 2^20 polls the stream
 * is asked whether it has died under us (`what` names it in that error), or has finished without delivering -- `timeout_text` -- which
 * is believed only after 2^26 polls (`patient`: the stores of a finished launch may still be on their way) or, for a word the stream
 * itself writes, at once. */
template <class Ready>
static inline int spin_until(MirScene* h, void* stream, const char* what, const char* timeout_text, bool patient, Ready ready) {
  unsigned long polls = 0;
  while (!ready()) {
    __builtin_ia32_pause();
    if ((++polls & 0xfffffu) == 0) {
      DeviceGuard guard(h->device);
      hipError_t e = hipStreamQuery((hipStream_t)stream);
      if (e != hipSuccess && e != hipErrorNotReady) return hip_fail(e, what);
      if (e == hipSuccess && (patient ? polls > 0x4000000u : !ready())) return set_err(MIR_E_HIP, timeout_text);
    }
  }
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  return MIR_OK;
}

}  // namespace mir_host
