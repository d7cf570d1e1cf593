// mir_retime_front.h — the host-side checks of mir_retime_path (mir_retime.hip; include/mirigid.h, "time parameterisation"): plain C++,
// no HIP in it, so that tests/retime_host.cpp builds them with g++ (`make retime-host`) and tests/test_retime_cpu.py walks every
// refusal without a device.  A refusal is `refuse(code, text)`: the caller's, which names the entry point.  The order of the checks
// and their texts are part of the interface.
#pragma once
#include <math.h>
#include <stdint.h>

#include "mirigid.h"

namespace {

constexpr int RETIME_MAX_DOF = 16;
constexpr int RETIME_MAX_ROWS = 64;  // the rows of one interval's LP: a lane each

// what the entry point was handed, as far as the checks read it
struct RetimeCall {
  bool handle, step_open;  // a handle was given; a mir_step_begin is open on it
  const MirRetimeQuery* q;
  int n_rows;
  const void *paths, *ea, *eb, *elo, *ehi;
  const void *x, *t, *duration, *status, *n_samples, *samples, *sample_vel;
};

static bool retime_positive(float v) { return isfinite(v) && v > 0.0f; }

template <class Refuse>
static int retime_check(const RetimeCall& c, Refuse refuse) {
  const MirRetimeQuery* const q = c.q;
  if (!c.handle || !q || !c.paths || !c.x || !c.t || !c.duration || !c.status || !c.n_samples) return refuse(MIR_E_INVALID, "null argument");
  if (q->struct_size != (int32_t)sizeof(MirRetimeQuery)) return refuse(MIR_E_INVALID, "struct_size is not sizeof(MirRetimeQuery)");
  if (q->num_waypoints < 2) return refuse(MIR_E_INVALID, "num_waypoints < 2");
  if (q->n_dofs < 1 || q->n_dofs > RETIME_MAX_DOF) return refuse(MIR_E_INVALID, "n_dofs outside 1 .. 16");
  if (q->n_extra < 0) return refuse(MIR_E_INVALID, "negative n_extra");
  if (q->n_extra > 0 && (!c.ea || !c.eb || !c.elo || !c.ehi)) return refuse(MIR_E_INVALID, "n_extra > 0 with a null extra array");
  if (c.n_rows < 0) return refuse(MIR_E_INVALID, "negative n_rows");
  if (q->num_samples < 0) return refuse(MIR_E_INVALID, "negative num_samples");
  if (q->flags) return refuse(MIR_E_INVALID, "unknown flag bit");
  for (int j = 0; j < q->n_dofs; j++) {
    if (!retime_positive(q->vmax[j])) return refuse(MIR_E_INVALID, "vmax must be finite and > 0");
    if (!retime_positive(q->amax[j])) return refuse(MIR_E_INVALID, "amax must be finite and > 0");
  }
  if (!retime_positive(q->dt)) return refuse(MIR_E_INVALID, "dt must be finite and > 0");
  if (!retime_positive(q->max_path_speed)) return refuse(MIR_E_INVALID, "max_path_speed must be finite and > 0");
  if ((c.samples || c.sample_vel) && q->num_samples < 1) return refuse(MIR_E_INVALID, "samples or sample_vel with num_samples < 1");
  if (c.step_open) return refuse(MIR_E_INVALID, "a step is pending (mir_step_end first)");
  if (2 * ((long long)q->n_dofs + q->n_extra) > RETIME_MAX_ROWS) return refuse(MIR_E_CAPACITY, "2 (n_dofs + n_extra) > 64: a lane holds one row of an interval");
  if (q->num_waypoints > MIR_RETIME_MAX_WAYPOINTS) return refuse(MIR_E_CAPACITY, "num_waypoints > MIR_RETIME_MAX_WAYPOINTS (x and t of a row live in LDS)");
  if ((long long)c.n_rows * q->num_samples * q->n_dofs > 0x7fffffffLL) return refuse(MIR_E_CAPACITY, "rows x num_samples x n_dofs beyond 2^31 - 1");
  return MIR_OK;
}

}  // namespace
