// mir_step.h — the kinds (instantiations) of the fused step kernel with their properties, and its launch arguments (shared by
// mir_step.hip and mir_api.hip)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mir_model.h"

// ---------------------------------------------------------------------------------------------
// FEAT (second template argument of mir_step_kernel, StepArgs::features): what the scene needs compiled in.
// FEAT_CONVEX = the scene has sphere / capsule geoms: the closed-form plane cases and the lane-private GJK / MPR narrowphase
// (mir_convex.h) are compiled in.  FEAT_SAP = the candidate pairs come from a sweep-and-prune over the geoms' world AABBs instead
// of the static pair list (scenes whose static list would exceed K16_MAX_PAIR, e.g. with self-collision enabled).  Scenes of planes
// and boxes with a short static list run the instantiation without either, whose register allocation and schedule are therefore
// untouched by that code.  FEAT_SPEC = the headline scene: its sizes and options (SpecPick, mir_spec_pick.h) are literals instead
// of model reads.
enum : int { FEAT_PLAIN = 0 /* planes and boxes, static pair list */, FEAT_CONVEX = 1, FEAT_SAP = 2, FEAT_SPEC = 4 };

// The KINDS of step launch = the first template argument (VARIANT) of mir_step_kernel<VARIANT, FEAT, CPL>; the numbers are part of
// the kernels' demangled names, which bench.py and tools/ look for in traces (8 was measured and dropped, see STEP_POST48).  One step
// body (mir_step_body.inc) serves all of them; built with -ffp-contract=on so that they agree bit for bit.  The host names the
// launch it wants by the same word (StepArgs::kind).  CPL = contacts per lane: 1, or 3 where lane c owns contacts c, c + 16, c + 32
// (capacity 48 = MIR_MAX_CONTACT, what the wave-per-env kernel holds).  DESIGN.md section 5 has the table.
enum StepKind : int {
  // one full step per launch without the rollout / autoreset / per-stage-output options (the headline launch): the step loop
  // disappears at compile time, and with it the block of scalar-register spills that the loop structure forces in front of it
  // (every launch-invariant value is otherwise saved before the loop and restored inside it).  Two waves, no AGPRs.
  STEP_SINGLE = 0,
  // the step loop for K-step rollouts (no per-stage / debug outputs and no separate observation buffers: only packed rows), which
  // keeps 11 pointers out of the scalar registers
  STEP_LOOP = 1,
  // everything (per-stage outputs, pose refresh, profiling stamps).  What the host asks for when it wants a whole step:
  // mir_launch_step takes STEP_SINGLE or STEP_LOOP instead where the arguments use nothing that those leave out.
  STEP_FULL = 2,
  // STEP_PRE / STEP_POST = the two halves of a single step for GenesisEnv.step, through a scratch row in HBM: PRE is the
  // action-independent half -- everything the two waves do up to the contact Jacobians (poses, dynamics, collision, contact arrays,
  // Jacobians) -- whose results go to the `pre` buffer instead of staying in LDS; POST picks them up and runs the rest on one wave
  // (all-rows-active Hessian included).  The host launches PRE for the NEXT step right behind the current step, so that it runs
  // while the host is between two env.step() calls.  (POST has no collision code in it: one instantiation serves every scene.)
  STEP_PRE = 3,
  STEP_POST = 4,
  // both halves in one launch, ROTATED: first the action-dependent half of THIS step (from the pre buffer), then the
  // action-independent half of the NEXT one (into the pre buffer).  The host sees `terminated` after the first half; the second
  // runs while it is between two env.step() calls, without a second launch, a second prologue or a second forward kinematics
  // (the closing FK of this step is the opening FK of the next).  Needs the split closing FK (fk_free_leaf scenes).
  STEP_ROTATED = 5,
  // (CPL = 3) the LIST instantiation for EXACT CONTACTS: the envs of StepArgs::env_list -- the ones a launch of the mir_step_begin
  // path deferred because their narrowphase found more candidate points than lanes -- take the WHOLE step here (the fused launch's
  // pass: two waves, dynamics beside collision detection) with three contacts per lane (Genesis keeps every point of its candidate
  // pairs: gym_genesis/tasks/franka/cube_pick.py:46 of the reference), store state, targets, observations and their terminated
  // bytes (byte k of StepArgs::term_host for list entry k), and then run the action-independent half of the NEXT step like the
  // rotated launch's second pass, into the env's scratch row: one launch instead of the wave-per-env kernel on the list followed
  // by STEP_PRE on the list, four envs per workgroup instead of one.  80 KB of LDS per workgroup, two workgroups per CU, one wave
  // per SIMD with the whole register file.  An env with more than 48 points or more than 16 candidate pairs is deferred AGAIN
  // (bit 7 of its byte; nothing stored): the wave-per-env kernel (64 candidates) stays the fallback for those.
  STEP_LIST48 = 6,
  // (CPL = 3) the same first pass ALONE, for the whole batch (no list, the regular terminated words): what mir_step_begin launches
  // INSTEAD of the one-contact-per-lane kernel while most envs would be deferred anyway (the HEAVY phase: the reference's expert
  // holds 70 % of its envs above 16 points through its two grasp stages): one launch per step instead of a launch that computes
  // garbage for the deferred majority followed by the list launch for them.  Bit 6 of a byte: the env had more points than
  // StepArgs::over_cap (what the host decides on when to go back).
  STEP_HEAVY48 = 7,
  // STEP_POST48 / STEP_PRE48 (CPL = 3) = the two halves of a step with three contacts per lane, as TWO launches: what mir_step_begin
  // launches for the whole batch while some env is above 16 points (an OVERFLOW RUN).  POST48 = the second half of this step from
  // the scratch rows -- an env with 17 .. 48 contacts has its row in StepArgs::pre_big, written by the launch before -- up to the
  // outputs and the terminated bytes (the rotated launch's first pass, then it returns); PRE48 = the first half of the next step
  // with the 48-point capacity (STEP_PRE with three contacts per lane).  The bytes of EVERY env leave after a solver pass -- two
  // rounds of short workgroups -- instead of after two rounds of whole steps (the heavy phase) or a fused pass of the list
  // instantiation behind the main launch's bytes; the first halves run while the host is between two env.step calls.  (8 = both in
  // one rotated launch: measured, no better than the heavy phase -- the second round's bytes wait for the first round's first
  // halves -- and not instantiated.)
  STEP_POST48 = 9,
  STEP_PRE48 = 10,
  // (CPL = 1) the rotated launch's first pass alone for a LIST of envs: the second half of the step for the envs of an overflow run
  // that are at most at 16 points -- one round of 40 KB workgroups beside STEP_POST48's list of the others
  STEP_ROTATED_LIST = 11,
  // STEP_XR16 / STEP_XR48 = the device-resident rollout that keeps every contact point (mir_rollout_exact; StepArgs::xr_*).  XR16
  // (CPL = 1) is STEP_LOOP -- the same one-wave step loop, the same arithmetic -- with DEFERRAL: at the first step whose candidate
  // points exceed the one-contact-per-lane capacity an env stores its state of that step's start and hands itself off to a device
  // list; from there on the launch stores nothing for it (its lanes compute on, unread).  XR48 (CPL = 3) is a step loop of passes
  // of STEP_HEAVY48's whole step, each env of that list from its own start step, with the step's packed row and the episode loop
  // of STEP_LOOP inside (mir_step_kernel); an env beyond its capacity goes on a second list for the wave-per-env kernel.
  // STEP_LOOP itself is untouched by either.
  STEP_XR16 = 12,
  STEP_XR48 = 13,
  // (CPL = 3) CONTACT FORCE SENSING (mir_contact_forces): STEP_HEAVY48's first pass for the whole batch -- 48 points, 16 candidate pairs,
  // two waves -- FORWARD ONLY: it stops behind the Newton solve, where every lane still holds the four pyramid-row forces of its
  // contacts, forms the world force of each contact, stores the contact list and reduces the net force per link over the env's row
  // (StepArgs::cf_*).  No integration, no state / target / warm-start / observation / terminated / host-byte stores, no diagnostics:
  // a read is invisible to the steps around it.  An env beyond the capacity is not deferred but FLAGGED (bit 0 of its flag byte: the
  // forces are those of the thinned manifold).  No launch of env.step(), of the rollouts or of bench.py takes this kind.
  STEP_SENSE48 = 14,
};

// ---- the table: what each kind is.  Everything that depends on the kind -- launch bounds, occupancy hint, block size and CPL of
// the launch, the body's compile-time switches, the host's bookkeeping -- asks here.
// contacts per lane
constexpr int step_cpl(int k) { return (k == STEP_LIST48 || k == STEP_HEAVY48 || k == STEP_POST48 || k == STEP_PRE48 || k == STEP_XR48 || k == STEP_SENSE48) ? 3 : 1; }
// three contacts per lane: the whole step in one pass (two waves, as STEP_SINGLE) ...
constexpr bool step_big(int k) { return step_cpl(k) > 1; }
// ... then the outputs, then the action-independent half of the next step
constexpr bool step_fused_next_pre(int k) { return k == STEP_LIST48; }
// the kinds that run only in contact-rich steps (an env above 16 points in the batch): their arithmetic is dominated by the contact
// rows, where packed fp32 pairs pay (STEP_POST48 57.5 us packed / 60.8 us not, STEP_HEAVY48 93.9 / 97.2, STEP_ROTATED_LIST 49.8 / 51.0 on
// the reference's expert and the scripted grasp), so they are compiled with the SLP vectoriser on; every other kind without it
// (STEP_ROTATED on the headline 21.1 / 20.8 us).  Build flags only: the bits are the same either way.
constexpr bool step_packed(int k) { return step_big(k) || k == STEP_ROTATED_LIST; }
// two passes of the body's loop: the second half of this step, then the first half of the next one ...
constexpr bool step_rotated(int k) { return k == STEP_ROTATED || k == STEP_POST48 || k == STEP_ROTATED_LIST; }
// ... of which only the first is taken
constexpr bool step_first_pass_only(int k) { return k == STEP_POST48 || k == STEP_ROTATED_LIST; }
// the action-independent half alone (into `pre`); the action-dependent half alone on one wave (from `pre`)
constexpr bool step_pre_only(int k) { return k == STEP_PRE || k == STEP_PRE48; }
constexpr bool step_post_only(int k) { return k == STEP_POST; }
// forward dynamics only, at the stored state with the stored targets: the pass ends behind the Newton solve with the contact-force
// outputs (StepArgs::cf_*) and stores nothing else
constexpr bool step_forward_only(int k) { return k == STEP_SENSE48; }
// the body keeps its step loop (n_steps, rollout rows, autoreset); the others take one step per launch or pass
constexpr bool step_has_loop(int k) { return k == STEP_LOOP || k == STEP_FULL || k == STEP_XR16; }
// ... and of those, the ones that hand back packed rows only
constexpr bool step_rows_only(int k) { return k == STEP_LOOP || k == STEP_XR16; }
constexpr bool step_exact_rollout(int k) { return k == STEP_XR16 || k == STEP_XR48; }
// DUAL: the workgroup has TWO waves.  Collision detection (geom poses, broadphase, narrowphase) needs only the link poses, and so
// do the smooth dynamics (subspaces, CRB, RNE, mass matrix, smooth solve): wave 1 does the former while wave 0 does the latter, in
// disjoint LDS areas, between two workgroup barriers.  At 4096 envs there is otherwise ONE wave per SIMD that spends 60 % of its
// life waiting on LDS round trips; the second wave fills those slots and takes ~5 k cycles out of the ~50 k of a step.  Wave 1
// also opens the launch with the forward kinematics of the stored state (its loads -- one qpos row, four quads of lane constants
// -- are back before wave 0's, which brings in the model table and everything else), and after the contacts it accumulates the
// all-rows-active Newton Hessian beside wave 0's warm start and first gradient: four barriers in all.  The step-loop
// instantiations keep one wave (they need the AGPRs a second wave per SIMD would have to give up); both run the same code in the
// same order of operations, so they agree bit for bit.
constexpr int step_waves(int k) { return (step_has_loop(k) || step_post_only(k)) ? 1 : 2; }
constexpr int step_block(int k) { return 64 * step_waves(k); }
// amdgpu_waves_per_eu (min, max): (2, 2) for the rotated one-contact-per-lane launches, (1, 1) with three contacts per lane (one
// wave per SIMD with the whole register file), (1, 10) = no constraint for the rest
constexpr int step_wpe_min(int k) { return (step_rotated(k) && !step_big(k)) ? 2 : 1; }
constexpr int step_wpe_max(int k) { return (step_rotated(k) && !step_big(k)) ? 2 : (step_big(k) ? 1 : 10); }
// exact contacts: an env with more candidate points than the kind holds is DEFERRED (StepArgs::exact)
constexpr bool step_defers(int k) { return k == STEP_SINGLE || k == STEP_POST || k == STEP_ROTATED || k == STEP_ROTATED_LIST || k == STEP_XR16 || step_big(k); }
// serves the envs of StepArgs::env_list where one is given
constexpr bool step_reads_env_list(int k) { return k == STEP_PRE || k == STEP_ROTATED_LIST || step_big(k); }
// stores host-visible terminated bytes / takes completion tickets where the launch asks for them
constexpr bool step_sends_host_bytes(int k) { return k != STEP_LOOP && !step_forward_only(k); }
// ... and may send the bytes from inside the solver loop, before it has converged (mir_model.h: term_bound_ok)
constexpr bool step_early_bytes_in_solver(int k) { return k == STEP_SINGLE || k == STEP_ROTATED || k == STEP_POST48 || k == STEP_ROTATED_LIST; }
// FEAT_SPEC: the instantiation still stores link poses for the rasteriser (the others leave that to the generic-scene one)
constexpr bool step_spec_stores_poses(int k) { return step_rotated(k) || step_big(k); }
// ---- what the launch does to the handle's state (launch() in mir_api.hip)
// advances qpos / qvel (everything but the action-independent half alone)
constexpr bool step_integrates(int k) { return !step_pre_only(k) && !step_forward_only(k); }
// leaves `pre` as valid as it was: the first halves (their callers mark it valid), and the list launch, which writes the scratch
// rows for the state it leaves itself
constexpr bool step_keeps_pre(int k) { return step_pre_only(k) || k == STEP_LIST48; }
// steps a LIST of envs of a step that another launch has already counted (state_version)
constexpr bool step_completes_counted_step(int k) { return k == STEP_LIST48 || k == STEP_ROTATED_LIST; }
// reads or writes the rows of up to 48 contacts in `pre_big`
constexpr bool step_uses_pre_big(int k) { return k == STEP_LIST48 || k == STEP_POST48 || k == STEP_PRE48; }

struct StepArgs {
  const DevModel* model;
  float* qpos;    // (B, qstride)
  float* qvel;    // (B, 16)
  float* target;  // (B, 16) indexed by dof
  float* qacc_ws; // (B, 16)
  float* poses;   // (B, 2, 16, 4) or null: link positions then quaternions written for the rasteriser (mode 2 only)
  const float* action;  // (B, nu) or null
  float* agent_pos;     // (B, 7+n_grip) or null
  float* env_state;     // (B, 11) or null
  float* reward;        // (B) or null
  uint8_t* terminated;  // (B) or null
  // host-visible tail of GenesisEnv.step (mir_step_begin / mir_step_end): the same bytes as `terminated`, stored straight into
  // pinned host memory (system-scope stores), and the launch's completion published by its LAST workgroup
  uint8_t* term_host;     // (B padded to 4) device address of pinned host memory, or null; byte = terminated | term_tag << 1
  uint32_t term_tag;      // 0..127: stamped into every byte so that the host can tell this launch's bytes from older ones
  uint32_t* done_ticket;  // device counter, 0 between launches; or null (completion is then signalled by the stream)
  uint32_t* done_flag;    // device address of a pinned host word <- done_seq once every workgroup has stored its bytes
  uint32_t done_seq;
  int32_t* diag;        // (B, 4): ncon, nefc, niter, flags; or null
  // debug / per-stage parity outputs (mir_forward), all nullable
  float* out_M;         // (B, nv, nv)
  float* out_bias;      // (B, nv)
  float* out_qas;       // (B, nv)
  float* out_qacc;      // (B, nv)
  float* out_xpos;      // (B, nbody, 3)
  float* out_xquat;     // (B, nbody, 4)
  unsigned long long* prof; // debug: 16 phase timestamps (shader clock) from block 0, or null
  float* rows;          // (B, row_stride) packed [agent | env_state | reward | terminated] or null
  int row_stride;
  long act_step;   // floats between the action blocks of consecutive steps (rollout mode), 0 = one action for all steps
  long rows_step;  // floats between the row blocks of consecutive steps (rollout mode), 0 = only the final row
  AutoResetArgs ar;  // per-step episode bookkeeping + re-spawn inside the launch (rollout mode only)
  int B;
  int qst, nu;  // qpos row stride and action width (copies of the model's, so the state loads do not wait for the model)
  int mode;     // 0: full steps; 1: forward dynamics only (mir_forward); 2: kinematics + outputs only
  int n_steps;  // mode 0 only
  int features; // FEAT_* bits (below)
  // which instantiation the launcher picks (a StepKind, below; the kernel itself never reads it).  STEP_FULL asks for a whole step:
  // mir_launch_step narrows it to STEP_SINGLE / STEP_LOOP where the arguments allow.  `pre`: K16_PRE_STRIDE floats per env.
  int kind;
  float* pre;
  // [0] env-steps that ended with a non-finite state (divergence guard, counted while diag is set; mir_get_bad);
  // early terminated bytes (mir_step.hip, mir_model.h: term_bound_ok): [1] workgroups whose early bytes differed from the integrated
  // state (must be 0: a non-zero count also raises the sticky word `term_bad`), [2 + w] launches in which workgroup w sent its bytes
  // from inside the solver loop (a contention-free counter per workgroup, always counted; summed by mir_debug_early_mask_stats)
  uint32_t* early_stats;
  uint32_t* term_bad;  // device address of a pinned host word <- 1 when early bytes turned out wrong (checked by the next API call: MIR_E_MASK)
  int no_early_mask;  // MIR_NO_EARLY_MASK=1: the bytes always wait for the integrator
  int term_wstride;   // 32-bit words between the term_host words of consecutive workgroups (mir_scene.h)
  // EXACT CONTACTS (mir_set_exact_contacts; single-step launches of the mir_step_begin path only).  An env whose narrowphase found
  // more candidate points than this kernel's contact capacity -- the count travels in bits 20 .. 27 of the `coupled` word, through the
  // scratch row of a split step too -- is DEFERRED: the launch stores nothing for it (state, targets, observations, diagnostics, the
  // scratch row of the next step) and sets bit 7 of its host-visible terminated byte.  mir_step_end then steps exactly those envs on the
  // wave-per-env kernel (48 points, no thinning) from the untouched state rows and recomputes their scratch rows (`env_list`).
  int exact;
  int over_cap;  // STEP_LIST48 / STEP_HEAVY48 (three contacts per lane): bit 6 of an env's terminated byte says that it had more candidate points than this (0: never set)
  // the kinds of step_reads_env_list: the launch serves the envs env_list[0 .. B) (B = the list's length) instead of envs 0 .. B; may point into pinned host memory
  const int32_t* env_list;
  // EXACT CONTACTS, the kinds of step_uses_pre_big (three contacts per lane): K48_STRIDE floats per env -- the scratch row of an env whose NEXT step has 17 .. 48
  // contacts (head, row constants and unpacked Jacobian rows of all of them; the mass-matrix rows and the bias force stay in `pre`).  The
  // head of the env's row in `pre` then holds ncon = 0, the count in the `coupled` word and K48_MAGIC in its third word: a launch of the
  // one-contact-per-lane kernel defers the env on the count, STEP_POST48 picks the big row up.  Null: such rows are not written.
  float* pre_big;
  // STEP_PRE48: device address of pinned host words, one per workgroup -- byte k = term_tag << 1 | (the NEXT step finds the workgroup's env k
  // with more candidate points than over_cap) -- or null
  uint32_t* next_host;
  // DEVICE-RESIDENT ROLLOUT THAT KEEPS EVERY CONTACT POINT (mir_rollout_exact: STEP_XR16 / STEP_XR48).  Nothing
  // of it is read by the host between two steps: the lists and counters stay in device memory.
  //  STEP_XR16 (the one-wave step loop with hand-off): an env whose step k finds more candidate points than the one-contact-per-lane
  //    capacity (or saturates the 16 candidate lanes) stores its state of step k's start, xr_start[env] = k, and is appended to
  //    xr_list (one device-scope atomicAdd on *xr_count); nothing more is stored for it in this launch.
  //  STEP_XR48 (the three-contacts-per-lane step loop, passes of the whole step): serves xr_list[0 .. *xr_count) -- the grid is fixed, a
  //    workgroup past the count exits at once -- and steps each env from xr_start[env] to n_steps - 1 (pass s: the actions and rows of
  //    step s of the call, autoreset inside; xr_step is set per pass).  An env beyond ITS capacity (48 points, 16 candidate pairs)
  //    stores nothing more, gets xr_start[env] = s | XR_TIER2 and goes on xr_list2 (*xr_count2) for the wave-per-env kernel.
  int32_t* xr_list;
  int32_t* xr_count;
  int32_t* xr_list2;
  int32_t* xr_count2;
  int32_t* xr_start;
  unsigned long long* xr_stats;  // STEP_XR48: [0] += env-steps taken (one device atomic per workgroup and pass)
  int xr_step;
  // CONTACT FORCE SENSING (mir_contact_forces: STEP_SENSE48 alone reads these; at the END of the struct, so that no other field's
  // kernel-argument offset moved when they came).  All nullable.  Contact rows in the solver's contact order, rows >= n_contacts zeroed.
  int32_t* cf_ncon;   // (B)
  uint8_t* cf_flags;  // (B) bit 0: more candidate points / pairs than the kind holds (forces of the thinned manifold)
  int32_t* cf_ids;    // (B, MIR_MAX_CONTACT, 4): geom_a, geom_b, link_a, link_b
  float* cf_geom;     // (B, MIR_MAX_CONTACT, 7): position, normal (a -> b), penetration
  float* cf_force;    // (B, MIR_MAX_CONTACT, 3): world force on link b
  float* cf_link;     // (B, nbody, 3): per link, sum over its contacts as b minus sum over its contacts as a
};
#ifndef XR_TIER2
#define XR_TIER2 (1 << 20) /* xr_start: the env is on the second list (the wave-per-env kernel); the low bits keep its step */
#endif
#define K48_HEAD 0    /* ncon, second-tree flags of contacts 16 .. 31, of 32 .. 47 (int bits), pad */
#define K48_CMETA 4   /* MIR_MAX_CONTACT x 4 */
#define K48_JB (K48_CMETA + 4 * MIR_MAX_CONTACT) /* MIR_MAX_CONTACT rows of 48 floats (n, t1, t2 x 16 dofs) */
#define K48_STRIDE (((K48_JB + 48 * MIR_MAX_CONTACT) + 15) / 16 * 16)
#define K48_MAGIC 0x42494721 /* "BIG!" */
#define K16_PRE_MROW 0     /* 16 lanes x 16: rows of the regularised mass matrix */
#define K16_PRE_BIAS 256   /* 16: qfrc_bias */
#define K16_PRE_HEAD 272   /* ncon, coupled (int bits), 2 pad */
#define K16_PRE_CMETA 276  /* K16_MAX_CONTACT x 4 */
#define K16_PRE_JB (K16_PRE_CMETA + 4 * K16_MAX_CONTACT) /* K16_MAX_CONTACT rows of 52 floats */
#define K16_PRE_STRIDE (((K16_PRE_JB + 52 * K16_MAX_CONTACT) + 15) / 16 * 16)


// enqueue the fused kernel on `stream`; returns a hipError_t as int
extern "C" __attribute__((visibility("hidden"))) int mir_launch_step(const StepArgs* args, hipStream_t stream);
extern "C" __attribute__((visibility("hidden"))) int mir_launch_debug_convex(const float* in, float* out, int n, hipStream_t stream);
