// mir_scene.h — the object behind a MirHandle (shared by every translation unit of the library)
#pragma once
#include <stdint.h>

#include "mir_model.h"
#include "mir_model64.h"
#include "mir_route.h"

// EXACT CONTACTS (mir_set_exact_contacts; 16-lane scenes).  The launches of mir_step_begin defer every env whose candidate contact points
// exceed the 16-lane kernel's capacity (bit 7 of its terminated byte), and mir_step_end completes the step for those envs -- on the list
// launch of the three-contacts-per-lane instantiation, on the wave-per-env kernel (hm64 / dm64 = the same scene compiled for it with 48
// points) for what is beyond that one too -- or the whole batch takes the three-contacts-per-lane instantiation from the start: a heavy
// step, or the two launches of an overflow run.  Which route a step takes is decided in mir_route.h (its header describes them) from
// cfg and phase; the launches and waits are in mir_api.hip (begin / end) and mir_exact.hip.  Nothing else touches this struct.
struct ExactRes {
  // pinned, device-mapped, one allocation: [deferred envs of the step being closed (B x i32) | terminated byte of list entry k, tagged
  // like the others (B, padded to 64)] twice -- the second pair for the envs the list launch hands on to the wave-per-env kernel --
  // then two permutations of the envs (B x i32 each), double-buffered: the order in which a heavy or two-launch step serves them
  int32_t *ovf_list_host, *ovf_list_dev;
  uint8_t *ovf_term_host, *ovf_term_dev;
  int32_t *perm_host[2], *perm_dev[2];
  void* ovf_stream;         // hipStream_t of the library's own: the launches for the deferred envs run beside the launch that deferred them, the first-half launch of a two-launch step beside the caller's work
  void* ovf_event;          // hipEvent_t: recorded behind them; the step's stream waits for it before anything queued after mir_step_end
  int ovf_event_live;       // ... it has been recorded behind launches the NEXT step must come after
  void* ovf_waited_stream;  // ... and this stream has been made to wait for it
  void* main_event;         // hipEvent_t: recorded on the step's stream in front of a launch the side stream's launch must come behind
  void* light_event;        // hipEvent_t behind the second list's launch on the side stream: the step's stream waits for it
  float* pre_big;           // (B, K48_STRIDE) device: scratch rows of an env with 17 .. 48 contacts (STEP_PRE48 -> STEP_POST48)
  uint32_t *next_host, *next_dev;  // pinned, device-mapped, (B + 3) / 4 words: which envs the first-half launch found above 16 points (StepArgs::next_host)
  // device-resident rollout that keeps every contact point (mir_rollout_exact; allocated by mir_set_exact_contacts, never by the call):
  // [stats: 4 x u64 -- list env-steps, wave env-steps, most envs handed off in one call, pad | counts: 16 x i32 -- list 1, list 2 |
  //  list 1 (B x i32) | list 2 (B x i32) | start step per env (B x i32)], device memory
  unsigned long long* xr_stats;
  int32_t* xr_count;
  int32_t *xr_list, *xr_list2, *xr_start;
  unsigned long long xr_calls;  // calls that went the device-resident way (host counter)
};

struct ExactRoute {
  int on;            // 0 off, 1 on, 2 (tests) every env is deferred: the whole batch takes the list launch
  ExactCfg cfg;      // set once by mir_set_exact_contacts
  ExactPhase phase;  // written by mir_step_end (rt_*: by mir_step_begin), read by the next mir_step_begin
  ExactPend pend;    // what the pending step was launched as
  ExactRes res;
  ExactStats stats;
};

struct MirScene {
  int device;
  int B;
  int kernel;       // 16: 16-lanes-per-env kernel (DevModel); 64: wave-per-env kernel (DevModel64)
  DevModel hm;      // host copy of the compiled model (kernel 16)
  DevModel64 hm64;  // host copy of the compiled model (kernel 64)
  HostConsts hc;
  PlumbTab pt;      // dof-order <-> storage maps (host copy)
  int nbody, nv, nq, nu, ngeom, npair, agent_dim, env_dim;
  DevModel* dm;     // device copies
  DevModel64* dm64;
  PlumbTab* dpt;
  GeomTab* dgeom;
  float *qpos, *qvel, *target, *qacc_ws, *poses;
  int32_t *diag, *fkvalid;
  uint8_t* cost = nullptr;  // wave kernel: two buffers of per-env cost flags (B padded to 64 each) for the dispatch order, see mir_step64.h
  int cost_par = 0;         // which of the two the next single-step launch reads
  int cost_stride = 0;
  uint32_t* early_stats = nullptr;  // 16-lane kernel: [1] mismatches of the early terminated bytes, [2 + w] launches in which workgroup w sent early (mir_step.h)
  int no_early_mask = 0;    // MIR_NO_EARLY_MASK=1, or a mismatch was seen (MIR_E_MASK)
  int spec_pick = 0;        // 16-lane kernel: the compiled model matches SpecPick (mir_spec_pick.h) and MIR_NO_SPEC is unset: specialised instantiation
  float* prims;     // render primitives (B, ngeom, 32) f32, allocated by the first mir_render
  int* bins = nullptr;      // per-strip primitive lists of the binned pixel kernel (grown on demand)
  size_t bins_cap = 0;      // ints
  int render_th = 0;        // strip height override (mir_debug_render_path; 0 = default)
  int render_generic = 0;   // force the generic pixel kernel (mir_debug_render_path)
  int render_round = 0;     // the scene has a sphere or a capsule: MIR_VIS_ROUND_GEOMS takes the round instantiations (mir_render.hip)
  unsigned long long* zbuf = nullptr;  // depth / colour buffer of the global view of many envs (mir_render.hip, k_global_splat)
  size_t zbuf_cap = 0;
  unsigned* vis = nullptr;         // [0] boxes with a non-empty screen rectangle this render, [1 ..] their indices (k_render_setup -> k_global_splat)
  size_t vis_cap = 0;
  unsigned long long state_version = 0;  // bumped by every call that changes qpos (launches that integrate, resets, state writes): mir_get_state_version
  int poses_live = 0;       // a render has been asked for: step launches also leave their final link poses in `poses` (mir_api.hip, launch())
  int poses_current = 0;    // `poses` matches qpos for every env (cleared by resets and state writes): mir_render skips the pose-refresh launch
  // host-visible tail of env.step() (mir_step_begin / mir_step_end): one pinned, device-mapped allocation
  //   [terminated bytes (B, padded to 64) | completion word]
  float* scratch_row;       // one qpos row (device), used while the scene is created
  uint8_t* pin_host;        // host address
  size_t pin_flag_off = 0;  // byte offset of the completion word behind the terminated area
  int term_wstride = 0;     // 16-lane kernel: 32-bit words between the terminated words of consecutive workgroups in the pinned area (16 = one
                            // 64-byte line each, see mir_step_end); 0 = one byte per env (wave kernel)
  uint8_t* pin_dev;         // the same memory as the device sees it
  uint32_t* done_ticket;    // device counter for the kernel-side completion (sync mode 2)
  uint32_t seq;             // sequence number of the completion word (sync modes 1 / 2, mir_debug_null_roundtrip)
  uint32_t tag;             // tag of the last mir_step_begin's terminated bytes, 1..31 (five bits of a byte); advances in mir_step_begin ONLY
  int sync_mode;            // 0 hipStreamSynchronize, 1 stream write-value + host spin, 2 kernel-side ticket + host spin
  int diag_on;              // step kernels write the per-env diagnostics (mir_set_diag)
  int pending;              // a mir_step_begin is waiting for its mir_step_end
  void* pending_stream;
  void* prep[4];            // output pointers registered by mir_step_prepare for the next mir_step_go
  int prepared;
  unsigned long long* dbg_prof = nullptr;  // (mir_debug_profile_next_step: shader-clock stamps of the next mir_step_begin launch)
  int32_t* dbg_ik_iters = nullptr;  // (mir_debug_ik_iters)
  unsigned long long* dbg_prof_list = nullptr;  // (mir_debug_profile_next_list_step: of the next launch of the list instantiation, exact contacts)
  // split step of the GenesisEnv.step path (16-lane kernel; MIR_SPLIT_STEP=0 switches it off): mir_step_begin launches the
  // action-independent half of the NEXT step right behind the current one; `pre_valid` says that `pre` holds that half for the
  // state as it is now (any other launch or state write clears it), `pre_stream` the stream it was launched on
  float* pre;
  int split_step, pre_valid;
  void* pre_stream;
  // EXACT CONTACTS (mir_set_exact_contacts; 16-lane scenes): see ExactRoute below
  ExactRoute xc;
  // RANGE SENSING (mir_raycast, mir_ray.hip): the geometry table with the hulls' face planes, built by the first call
  void* ray_tab;            // device
  int ray_state;            // 0 not built yet, 1 built, -1 the scene has a hull without volume (every call fails)
  // SIGNED DISTANCE (mir_signed_distance, mir_dist.hip): its geometry table with the hulls' face planes and triangle fans, built by the first call
  void* dist_tab;           // device
  int dist_state;           // as ray_state
  int dist_nplane;          // planes in the table (the triangles follow them)
};

// library-internal helpers implemented in mir_api.hip
int mir_set_error(int code, const char* msg);
int mir_refresh_poses(MirScene* h, void* stream);  // make h->poses match qpos for every env (mode-2 launch)
