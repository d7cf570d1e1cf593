// mir_route.h — which launches a step of a scene with EXACT CONTACTS gets, as plain functions of plain data: no HIP,
// no handle, nothing is launched or waited for here.  mir_step_begin asks plan_begin, mir_step_end asks close_step (mir_api.hip);
// tests/test_route_cpu.py compiles this header with g++ and checks the rules on the CPU.
//
// The routes.  A launch of the 16-lane kernel holds 16 contact points per env; with exact contacts on it DEFERS an env above that (bit 7
// of the env's terminated byte) and the step is completed for those envs behind the bytes:
//   light step     one launch (rotated / second half / whole step, as without exact contacts); mir_step_end hands the deferred envs to the
//                  LIST launch of the three-contacts-per-lane instantiation (48 points), and what that one cannot hold either to the
//                  wave-per-env kernel (exact_finish, mir_exact.hip);
//   heavy step     the WHOLE batch in one launch of the three-contacts-per-lane instantiation (STEP_HEAVY48): nothing deferred but the envs
//                  beyond 48 points, no scratch rows.  mir_step_end enters the phase when a step deferred at least heavy_enter envs and
//                  leaves it when fewer than heavy_leave were above 16 points (bit 6 of the bytes of such a launch);
//   two launches   (an OVERFLOW RUN: from the step after one that deferred an env until a step with no env above 16 points) where the
//                  caller leaves room between two steps: the step's second half for the whole batch with three contacts per lane
//                  (STEP_POST48), then the first half of the next step (STEP_PRE48) on the side stream, beside the caller's work;
//   two lists      the second half of such a step once the first-half launch before it has said which envs are above 16 points NOW:
//                  those on STEP_POST48 on the step's stream, the others on STEP_ROTATED_LIST on the side stream.
// Every route computes the same bits; they differ in GPU time and in the time to the terminated bytes.
#pragma once
#include <stddef.h>
#include <stdint.h>

// the launches plan_begin chooses from, numbered like StepKind (mir_step.h, which needs HIP; mir_api.hip asserts that they agree)
enum RouteKind : int { RK_FULL = 2, RK_POST = 4, RK_ROTATED = 5, RK_HEAVY48 = 7, RK_POST48 = 9, RK_ROTATED_LIST = 11 };

// set once by mir_set_exact_contacts, from the scene and the environment
struct ExactCfg {
  int exact_big;                 // the deferred envs take the list instantiation of the 16-lane kernel; 0: the wave-per-env kernel (MIR_EXACT_WAVE=1, or no split closing FK)
  int big_on;                    // MIR_EXACT_BIG: two-launch steps 0 never, 1 when the caller leaves room between two steps (default), 2 always
  int big_lists;                 // MIR_EXACT_BIG_LISTS=0: their second half never as two lists
  int big_side;                  // MIR_EXACT_BIG_SIDE=0 (a test switch): their first-half launch on the step's stream, not the side stream
  int heavy_enter, heavy_leave;  // MIR_EXACT_HEAVY, in envs; enter <= 0: never heavy
  int heavy_sort;                // MIR_EXACT_HEAVY_SORT=0: never permute the envs
  double big_gap_us;             // MIR_EXACT_BIG_GAP: what the caller must spend between two steps for "leaves room"
};

// decided by mir_step_end (close_step) for the next mir_step_begin; rt_* by mir_step_begin for the next one
struct ExactPhase {
  int heavy;           // the coming step is a heavy step
  int bigmode;         // an overflow run is on: the coming step may take the two launches
  int perm_next;       // which of the two permutation buffers the coming heavy / two-launch step serves the envs through (-1: in order)
  int rt_ok, rt_perm;  // the first-half launch of the step before wrote its "above 16 points" words, serving the envs through buffer rt_perm (-1: in order)
  uint32_t rt_tag;     // ... tagged with this
  double t_end_us;     // wall clock of the last mir_step_end's return (0: none yet)
};

// what the pending step was launched as (mir_step_begin), for the mir_step_end that closes it
struct ExactPend {
  int heavy, big;       // a heavy step / a two-launch step
  int perm;             // the permutation buffer its launches served the envs through (-1: in order)
  int rotated;          // ONE rotated launch (else a launch followed by the first half of the next step for all envs)
  const float* action;  // its arguments: the launches for the deferred envs take the same
  void* out[4];
};

struct ExactStats {
  unsigned long long steps, ovf_steps, ovf_envs, ovf_max;  // steps closed / with envs above 16 points / such env-steps / most in one step
  unsigned long long big_envs, wave_envs;                  // env-steps handed to the list launch (those it handed on included) / stepped by the wave-per-env kernel
  unsigned long long heavy_steps, big_steps;               // heavy steps / two-launch steps
};

// what mir_step_begin knows about the handle and the call when it asks
struct BeginFacts {
  int exact;       // 0 off, 1 on, 2 every env is deferred (the twin of the tests)
  int sync_mode, split_step;
  bool pre_valid, same_stream;  // the first half of this step is in the scratch rows / was launched on this call's stream
  bool fk_free_leaf;            // the scene has the split closing forward kinematics
  bool has_pre_big, has_side_stream, has_next_host;
  double gap_us;   // since the last mir_step_end returned; negative: there was none
};

struct BeginPlan {
  int kind;  // RouteKind of the step's launch (of the first of two lists)
  bool heavy, bigrot;  // a heavy step / a two-launch step
  bool split;          // the first half of the NEXT step goes out with this one (inside a rotated launch, or as a launch of its own)
  bool have_pre, rotated;
  bool lists;          // the second half may go out as two lists: wait for the words of the first-half launch before, then plan_lists
  int perm;            // permutation buffer the launches serve the envs through (-1: in order; with `lists`: the one the split fills)
};

static inline BeginPlan plan_begin(const ExactCfg& c, const ExactPhase& ph, const BeginFacts& f) {
  BeginPlan p;
  const bool big48 = f.exact && c.exact_big && f.sync_mode == 3;
  // two launches: the rows of the first half must be there, and the caller must leave the next first-half launch room to hide (the policy
  // and its IK in the reference's expert loop: ~90 us; a loop that does nothing between two steps: 2 - 5 us)
  p.bigrot = big48 && f.exact == 1 && ph.bigmode && f.has_pre_big && f.has_side_stream && f.split_step && f.pre_valid && f.same_stream &&
             f.fk_free_leaf && (c.big_on == 2 || (f.gap_us >= 0.0 && f.gap_us >= c.big_gap_us));
  p.heavy = big48 && ph.heavy && !p.bigrot;
  p.split = f.split_step && f.sync_mode != 2 && !p.heavy;
  p.have_pre = p.split && f.pre_valid && f.same_stream;
  // (one rotated launch -- this step's second half, then the next step's first half -- where the closing FK can be shared between the
  //  waves; otherwise two launches)
  p.rotated = p.have_pre && f.fk_free_leaf && f.split_step != 2 && !p.bigrot;
  p.kind = p.heavy ? RK_HEAVY48 : p.bigrot ? RK_POST48 : p.rotated ? RK_ROTATED : p.have_pre ? RK_POST : RK_FULL;
  p.lists = p.bigrot && ph.rt_ok && c.big_side && f.has_next_host && c.big_lists;
  // (in the order mir_step_end left: the envs above 16 points first -- workgroups of like cost, the long ones early)
  p.perm = (p.heavy || p.bigrot) ? ph.perm_next : -1;
  return p;
}

// nh of the B envs are above 16 points (padded to whole workgroups).  True: two launches, perm[0 .. nh) as p.kind on the step's stream
// and perm[nh .. B) as RK_ROTATED_LIST on the side stream; false: one launch of p.kind (adjusted here) over the whole permutation.
static inline bool plan_lists(BeginPlan& p, int nh, int B) {
  if (nh > 0 && nh < B) return true;
  p.kind = nh == 0 ? RK_ROTATED_LIST : RK_POST48;
  return false;
}

struct CloseResult {
  bool sort;     // fill a permutation buffer for the next launch: the envs with `bit` set in their byte first
  uint32_t bit;  // 0x40 "above 16 points" (bytes of a heavy or two-launch step), 0x80 "deferred" (a light one)
};

// The pending step's bytes are in: ndefer envs were deferred (bit 7), nover had bit 6.  Counts the step and decides the next one's phase.
static inline CloseResult close_step(const ExactCfg& c, ExactPhase& ph, const ExactPend& pend, ExactStats& st, int ndefer, int nover) {
  // a heavy or two-launch step reports its envs above 16 points in bit 6; a light one defers exactly those
  const bool big = pend.heavy || pend.big;
  const unsigned long long cnt = (unsigned long long)(big ? nover : ndefer), nd = (unsigned long long)ndefer;
  st.ovf_envs += cnt;
  if (cnt) st.ovf_steps++;
  if (cnt > st.ovf_max) st.ovf_max = cnt;
  if (nd > st.ovf_max) st.ovf_max = nd;  // (the envs a heavy or two-launch step deferred count towards the maximum whatever their bit 6 says)
  if (!c.exact_big) return {false, 0u};
  // an overflow run starts behind the first step that deferred an env and ends with the first of its steps in which no env is above 16 points
  if (c.big_on) {
    if (!ph.bigmode && ndefer > 0) ph.bigmode = 1;
    else if (pend.big && nover == 0 && ndefer == 0) ph.bigmode = 0;
  }
  // The cost model behind the default thresholds: a light step with a deferred list costs launch + list launch, a heavy
  // one two rounds of the bigger kernel.
  const int n = pend.heavy ? nover : ndefer;
  if (!ph.heavy && c.heavy_enter > 0 && n >= c.heavy_enter) ph.heavy = 1;
  else if (ph.heavy && n < c.heavy_leave) ph.heavy = 0;
  // A workgroup serves four consecutive entries and lasts as long as its slowest env: with 70 % of the envs at 20 - 38 points and the
  // rest at 4 - 12, unsorted 99 % of the workgroups hold a slow env; sorted, 30 % of them are done in half the time, and the expensive
  // ones are dispatched first.  (rt_ok: the next step of the run takes its order from the first-half launch's words, plan_lists.)
  ph.perm_next = -1;
  return {(ph.heavy || ph.bigmode) && c.heavy_sort && !(pend.big && ph.rt_ok && !ph.heavy), big ? 0x40u : 0x80u};
}

// One word = the bytes of the four envs 4 g .. 4 g + 3 of the launch order (env perm_in[i], or i): those with `bit` set in their byte
// go to out[nh++], the others to out[--lo].
static inline void partition_word(uint32_t v, size_t g, const int32_t* perm_in, size_t B, uint32_t bit, int32_t* out, size_t& nh, size_t& lo) {
  for (size_t k = 0; k < 4 && 4 * g + k < B; k++) {
    const int32_t e = perm_in ? perm_in[4 * g + k] : (int32_t)(4 * g + k);
    if (v >> (8 * k) & bit) out[nh++] = e; else out[--lo] = e;
  }
}

// The order of the next launch: the envs with `bit` set from the front in scan order, the others packed from the back.  Returns how many
// are in front.  words[g * word_stride] is word g.
static inline size_t partition_by_bit(const volatile uint32_t* words, size_t word_stride, const int32_t* perm_in, size_t B, uint32_t bit, int32_t* out) {
  size_t nh = 0, lo = B;
  for (size_t g = 0; 4 * g < B; g++) partition_word(words[g * word_stride], g, perm_in, B, bit, out, nh, lo);
  return nh;
}
