// C entry points over gym-genesis_amd/csrc/mir_route.h for tests/test_route_cpu.py (built by `make route-host`): the routing decisions
// of exact contacts on the CPU, no HIP anywhere.
#include "mir_route.h"

extern "C" {

// n cases in one call.  in: 18 columns of n floats {exact, big_on, split_step, sync_mode, gap_us, big_gap_us, exact_big, bigmode, heavy,
// rt_ok, big_side, big_lists, pre_valid, same_stream, fk_free_leaf, has_pre_big, has_side_stream, has_next_host}, perm_next is 1;
// out: n rows of 8 ints {kind, heavy, bigrot, split, have_pre, rotated, lists, perm}
void route_plan_begin(const float* in, int n, int32_t* out) {
  for (int i = 0; i < n; i++) {
    float r[18];
    for (int j = 0; j < 18; j++) r[j] = in[(size_t)j * n + i];
    ExactCfg c = {};
    ExactPhase ph = {};
    BeginFacts f = {};
    f.exact = (int)r[0]; c.big_on = (int)r[1]; f.split_step = (int)r[2]; f.sync_mode = (int)r[3]; f.gap_us = r[4]; c.big_gap_us = r[5];
    c.exact_big = (int)r[6]; ph.bigmode = (int)r[7]; ph.heavy = (int)r[8]; ph.rt_ok = (int)r[9]; c.big_side = (int)r[10]; c.big_lists = (int)r[11];
    f.pre_valid = r[12] != 0; f.same_stream = r[13] != 0; f.fk_free_leaf = r[14] != 0;
    f.has_pre_big = r[15] != 0; f.has_side_stream = r[16] != 0; f.has_next_host = r[17] != 0;
    ph.perm_next = 1;
    const BeginPlan p = plan_begin(c, ph, f);
    int32_t* o = out + 8 * (size_t)i;
    o[0] = p.kind; o[1] = p.heavy; o[2] = p.bigrot; o[3] = p.split; o[4] = p.have_pre; o[5] = p.rotated; o[6] = p.lists; o[7] = p.perm;
  }
}

// returns 1 for two launches; *kind = the (first) launch's kind
int route_plan_lists(int kind, int nh, int B, int32_t* kind_out) {
  BeginPlan p = {};
  p.kind = kind;
  const bool two = plan_lists(p, nh, B);
  *kind_out = p.kind;
  return two ? 1 : 0;
}

// cfg {exact_big, big_on, heavy_enter, heavy_leave, heavy_sort}; phase in/out {heavy, bigmode, perm_next, rt_ok}; pend {heavy, big};
// stats in/out {steps with overflow, overflow env-steps, most in a step}; out {sort, bit}
void route_close_step(const int32_t* cfg, int32_t* phase, const int32_t* pend, uint64_t* stats, int ndefer, int nover, int32_t* out) {
  ExactCfg c = {};
  c.exact_big = cfg[0]; c.big_on = cfg[1]; c.heavy_enter = cfg[2]; c.heavy_leave = cfg[3]; c.heavy_sort = cfg[4];
  ExactPhase ph = {};
  ph.heavy = phase[0]; ph.bigmode = phase[1]; ph.perm_next = phase[2]; ph.rt_ok = phase[3];
  ExactPend pe = {};
  pe.heavy = pend[0]; pe.big = pend[1];
  ExactStats st = {};
  st.ovf_steps = stats[0]; st.ovf_envs = stats[1]; st.ovf_max = stats[2];
  const CloseResult r = close_step(c, ph, pe, st, ndefer, nover);
  phase[0] = ph.heavy; phase[1] = ph.bigmode; phase[2] = ph.perm_next; phase[3] = ph.rt_ok;
  stats[0] = st.ovf_steps; stats[1] = st.ovf_envs; stats[2] = st.ovf_max;
  out[0] = r.sort; out[1] = (int32_t)r.bit;
}

int route_partition_by_bit(const uint32_t* words, int word_stride, const int32_t* perm_in, int B, uint32_t bit, int32_t* out) {
  return (int)partition_by_bit(words, (size_t)word_stride, perm_in, (size_t)B, bit, out);
}

}  // extern "C"
