/*
 * mirigid.h — C ABI of libmirigid.so, the MI355X-native batched rigid-body
 * step backend that sits behind gym-genesis's env.step() hot path.
 *
 * The reference (huggingface/gym-genesis) has NO FFI for this path: every
 * FLOP of env.step() runs inside the external `genesis-world` package through
 * its Python object API.  The entry points below are therefore the C-level
 * restatement of exactly those Genesis calls the reference makes on the path
 * (file:line cited per function, paths relative to /root/reference):
 *
 *   gs.Scene(...) + add_entity + scene.build(n_envs=B)
 *        gym_genesis/tasks/franka/cube_pick.py:34-68      -> mir_create
 *   cube.set_pos / cube.set_quat / franka.set_qpos(zero_velocity=True)
 *        gym_genesis/tasks/franka/cube_pick.py:96-102     -> mir_reset
 *   franka.control_dofs_position(target, dofs_idx)
 *        gym_genesis/tasks/franka/cube_pick.py:104-105,123-124 -> mir_set_pd_targets
 *   scene.step()
 *        gym_genesis/tasks/franka/cube_pick.py:107,125 ; gym_genesis/env.py:60 -> mir_step
 *   step() = control + scene.step() + compute_reward() + get_obs() + (reward==1)
 *        gym_genesis/tasks/franka/cube_pick.py:122-181 ; gym_genesis/env.py:61-69 -> mir_step_fused
 *   link.get_pos / link.get_quat / entity.get_dofs_position / get_qpos
 *        gym_genesis/tasks/franka/cube_pick.py:140-146    -> mir_get_links / mir_get_state
 *
 * Conventions
 *   - All device buffers are caller-owned raw device pointers (torch
 *     tensor.data_ptr()), row-major (B, D), float32 unless stated.  Nothing
 *     is retained past the call.  Internal state is env-major
 *     rows (B, D) in HBM (one 64-byte-aligned row group per env).
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  No
 *     entry point synchronises the device.
 *   - Quaternions are wxyz (Genesis convention, cube_pick.py:94).
 *   - Return 0 on success, negative MIR_E_* on error; text in mir_last_error().
 *   - The scene description (MirSceneSpec) is plain host data in doubles.
 */
#ifndef MIRIGID_H
#define MIRIGID_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIR_VERSION 3

/* capacity limits of the spec.  Two step kernels sit behind the ABI: scenes with nv <= 15, nbody <= 16,
 * ngeom <= 24, <= 64 candidate pairs and max_contacts <= 16 (the pick tasks) run on the 16-lanes-per-env kernel
 * (4 envs per wave); anything larger (the 5-cube stack tasks) on the wave-per-env kernel, whose limits these are.
 * Every kinematic tree must have <= 16 dofs. */
#define MIR_MAX_BODY 32 /* including world = body 0 */
#define MIR_MAX_DOF 48  /* nv */
#define MIR_MAX_Q 56    /* nq */
#define MIR_MAX_GEOM 40
#define MIR_MAX_PAIR 256   /* candidate geom pairs after static filtering */
#define MIR_MAX_CONTACT 48 /* contacts kept per env per step (plane-box <= 4, box-box <= 8 per pair) */
#define MIR_MAX_GRIP 4
#define MIR_MAX_FREE 8     /* free bodies (cubes) */
#define MIR_MAX_HULL_VERT 32 /* vertices of one MIR_GEOM_HULL geom */
#define MIR_MAX_VERT 96      /* the scene's vertex pool */

/* error codes */
#define MIR_OK 0
#define MIR_E_INVALID (-1) /* bad argument / spec */
#define MIR_E_CAPACITY (-2) /* spec exceeds MIR_MAX_* */
#define MIR_E_HIP (-3)      /* HIP runtime error */
#define MIR_E_NODEVICE (-4) /* no gfx950 device visible */
#define MIR_E_MASK (-5)     /* early terminated bytes (mir_step_begin) turned out wrong; see mir_step_begin */

/* joint types (one joint per body, anchored at the body origin) */
#define MIR_JNT_FIXED 0
#define MIR_JNT_REVOLUTE 1
#define MIR_JNT_PRISMATIC 2
#define MIR_JNT_FREE 3 /* qpos = pos3 + quat4(wxyz); qvel = world lin3 + world ang3 */

/* geom types */
#define MIR_GEOM_PLANE 0 /* z = 0 plane of its body frame, normal +z */
#define MIR_GEOM_BOX 1   /* size = half extents */
#define MIR_GEOM_SPHERE 2  /* size[0] = radius */
#define MIR_GEOM_CAPSULE 3 /* size[0] = radius, size[1] = half length of the axis segment, axis = z of the geom frame */
#define MIR_GEOM_HULL 4    /* convex hull of size[1] vertices of the scene's pool starting at vertex size[0] (MirSceneSpec.vert, geom
                            * frame; the frame's origin must lie inside the hull: MPR starts from it); size[2] is ignored.  The
                            * stand-in for the reference's mesh collision geometry (convex hulls of link meshes).  Support mapping
                            * = the vertex of largest projection, lowest index on ties.  Plane - hull: the penetrating vertices,
                            * reduced to four like plane - box; every other pair through GJK on the cores (the hull is its own core,
                            * radius 0) and MPR.  Both step kernels: up to 40 vertices per scene in the 16-lane kernel, up to
                            * MIR_MAX_VERT in the wave kernel (a scene with more than 40 goes there). */
/* Narrowphase by pair type: plane-box / plane-sphere / plane-capsule in closed form (<= 4 / 1 / 2 points), box-box by
 * separating axes and face clipping (<= 8 points), every other convex pair by Minkowski Portal Refinement on the shapes'
 * support mappings (one point: deepest penetration) -- the default convex-convex path of Genesis.
 * Every geom type is supported by both step kernels (the wave-per-env kernel since round 3 for spheres and capsules, since
 * round 4 for hulls). */

/* dof control modes */
#define MIR_CTRL_NONE 0
#define MIR_CTRL_POSITION 1 /* tau = kp (target - q) - kv qd, clamped (control_dofs_position) */

typedef struct MirBodySpec {
  int32_t parent; /* index < own index; 0 = world */
  int32_t jtype;  /* MIR_JNT_* */
  double pos[3];  /* frame in parent (FREE: initial world pose) */
  double quat[4]; /* wxyz */
  double axis[3]; /* joint axis in body frame (REVOLUTE / PRISMATIC) */
  double mass;
  double ipos[3];    /* COM in body frame */
  double inertia[6]; /* about COM, body axes: xx yy zz xy xz yz */
} MirBodySpec;

typedef struct MirDofSpec {
  int32_t limited;   /* joint range active */
  int32_t ctrl_mode; /* MIR_CTRL_* */
  double range[2];
  double armature;
  double damping;
  double kp, kv;
  double frc_range[2];
  double solref[2]; /* timeconst, dampratio (limit constraint) */
  double solimp[5]; /* dmin dmax width mid power */
} MirDofSpec;

typedef struct MirGeomSpec {
  int32_t body;
  int32_t type; /* MIR_GEOM_* */
  int32_t contype;
  int32_t conaffinity;
  double size[3];
  double pos[3];  /* in body frame */
  double quat[4]; /* wxyz */
  double friction;
  double solref[2];
  double solimp[5];
} MirGeomSpec;

typedef struct MirOptions {
  double dt;         /* cube_pick.py:45 -> 0.01 */
  double gravity[3]; /* (0,0,-9.81) */
  double tolerance;  /* Newton scaled-improvement / gradient tolerance */
  double ls_tolerance;
  int32_t iterations; /* max Newton iterations */
  int32_t ls_iterations;
  int32_t enable_collision;
  int32_t enable_joint_limit;
  int32_t enable_self_collision;     /* geoms of one articulated entity may collide */
  int32_t enable_adjacent_collision; /* parent/child link geoms may collide */
  int32_t max_contacts;              /* <= MIR_MAX_CONTACT */
  int32_t implicit_damping;          /* M += dt (damping + kv) on the diagonal */
} MirOptions;

/* reward rules */
#define MIR_REWARD_LIFT 0  /* obj_z > reward_z                                   (cube_pick.py:130-135) */
#define MIR_REWARD_STACK 1 /* |obj.xy - obj2.xy| < reward_xy && obj.z - obj2.z > reward_dz
                              (cube_stack_batch.py:143-153, cube_stack_kitchen_batch.py:138-146) */
/* agent_pos layouts */
#define MIR_AGENT_EEF 0  /* [eef pos3, eef quat4, grip q...]                    (cube_pick.py:140-151) */
#define MIR_AGENT_QPOS 1 /* qpos of every scalar joint, body order               (cube_stack_batch.py:169) */

/* what the fused step extracts (reference get_obs / compute_reward) */
typedef struct MirTaskSpec {
  int32_t eef_body;               /* franka.get_link("hand"), cube_pick.py:68 */
  int32_t obj_body;               /* cube / cube_1 */
  int32_t n_grip;                 /* gripper dofs appended to agent_pos (MIR_AGENT_EEF) */
  int32_t grip_dof[MIR_MAX_GRIP]; /* dof indices (cube_pick.py:142 -> 7,8) */
  double reward_z;                /* MIR_REWARD_LIFT threshold (cube_pick.py:134 -> 0.1) */
  int32_t obj2_body;              /* cube_2, or -1: env_state gets obj2 pos3 appended (11 -> 14 columns) */
  int32_t reward_mode;            /* MIR_REWARD_* */
  int32_t agent_mode;             /* MIR_AGENT_* */
  int32_t _pad;
  double reward_xy, reward_dz;    /* MIR_REWARD_STACK thresholds (0.05, 0.03) */
} MirTaskSpec;

typedef struct MirSceneSpec {
  int32_t struct_size; /* = sizeof(MirSceneSpec), ABI check */
  int32_t version;     /* = MIR_VERSION */
  int32_t nbody, ndof, ngeom, _pad;
  MirOptions opt;
  MirTaskSpec task;
  MirBodySpec body[MIR_MAX_BODY];
  MirDofSpec dof[MIR_MAX_DOF]; /* in body order: 1 per REVOLUTE/PRISMATIC, 6 per FREE */
  MirGeomSpec geom[MIR_MAX_GEOM];
  int32_t nvert, _pad2;
  double vert[MIR_MAX_VERT][3]; /* vertex pool of the MIR_GEOM_HULL geoms, geom frame */
} MirSceneSpec;

typedef struct MirScene* MirHandle;

/* sizes of the batched state vectors for a created scene */
typedef struct MirDims {
  int32_t num_envs, nbody, nq, nv, ngeom, npair, agent_dim, env_dim;
  int32_t nfree, kernel; /* free bodies; 16 = 16-lanes-per-env kernel, 64 = wave-per-env kernel */
} MirDims;

int mir_version(void);
int mir_spec_sizeof(void);
const char* mir_last_error(void);

/* gs.Scene + add_entity + scene.build(n_envs): compile spec, allocate env-major state
 * for num_envs on device_id, set state to the spec's initial pose. */
int mir_create(const MirSceneSpec* spec, int32_t num_envs, int32_t device_id, MirHandle* out);
int mir_destroy(MirHandle h);
int mir_get_dims(MirHandle h, MirDims* out);

/* derived model constants, for parity tests (host doubles; arrays sized nv / nbody) */
int mir_get_model_consts(MirHandle h, double* dof_invweight0, double* body_invweight0, double* meaninertia);

/* cube.set_pos/set_quat + franka.set_qpos(zero_velocity=True) (+ PD targets = qpos).
 * obj_pos (B,nfree,3) / obj_quat (B,nfree,4): world poses of ALL free bodies in body order (the pick scenes
 * have one, task.obj_body; the stack scenes five: cube_stack_kitchen_batch.py:70-96); arm_qpos (B,n_arm):
 * values for every non-FREE joint in body order.  All velocities and the solver
 * warm start are zeroed.  env_mask (B) u8 nullable: reset only envs with mask!=0. */
int mir_reset(MirHandle h, const float* obj_pos, const float* obj_quat, const float* arm_qpos,
              const uint8_t* env_mask, void* stream);

/* Device-side episode bookkeeping and re-spawn.  The reference can only reset the
 * whole batch from the host after a D->H read of `terminated` (README.md:41-43, env.py:64,
 * cube_pick.py:86-112); this call keeps the loop on the device.  Per env:
 *   episode_len += 1;  truncated = !terminated && max_len > 0 && episode_len >= max_len;
 *   done = terminated || truncated.
 * Done envs are reset exactly as mir_reset does (arm_qpos, zero velocity, PD targets = arm_qpos,
 * free bodies at spawn_pool[cursor % pool_len][env] with obj_quat), episode_len = 0, cursor += 1.
 * spawn_pool (pool_len,B,nfree,3) f32, obj_quat (B,nfree,4): spawn poses drawn ahead by the caller (the task's host
 * RandomState stays the source of randomness).  terminated (B) u8 nullable; episode_len, cursor (B)
 * i32 in/out; truncated_out, done_out (B) u8 nullable.  No physics step is consumed. */
int mir_autoreset(MirHandle h, const uint8_t* terminated, int32_t* episode_len, int32_t max_len,
                  const float* spawn_pool, int32_t pool_len, int32_t* cursor, const float* obj_quat,
                  const float* arm_qpos, uint8_t* truncated_out, uint8_t* done_out, void* stream);

/* control_dofs_position over all position-controlled dofs, in dof order: tgt (B,nu) */
int mir_set_pd_targets(MirHandle h, const float* tgt, void* stream);

/* scene.step() x n_steps */
int mir_step(MirHandle h, int32_t n_steps, void* stream);

/* FrankaCubePickBatch.step + GenesisEnv.step in one launch:
 * targets <- action (B,nu); one physics step; agent_pos (B,agent_dim) = [eef_pos3, eef_quat4, grip_q]
 * (MIR_AGENT_EEF) or the scalar-joint qpos (MIR_AGENT_QPOS); env_state (B,env_dim) = [obj_pos3, obj_quat4,
 * eef-obj 3, |eef-obj| 1] (+ obj2_pos3 when task.obj2_body >= 0); reward (B) f32 by task.reward_mode;
 * terminated (B) u8 = reward == 1.  action may be NULL (keep current targets).  action is read once, by the launch, with its first
 * loads: it may also point into pinned host memory (hipHostMalloc / a pinned torch tensor), which the kernel then reads in place
 * over PCIe -- the buffer must stay untouched until the launch has started (mir_step_end of the same step has returned). */
int mir_step_fused(MirHandle h, const float* action, float* agent_pos, float* env_state, float* reward,
                   uint8_t* terminated, void* stream);

/* GenesisEnv.step's host-visible tail, in two halves (gym_genesis/env.py:61-69):
 *     is_success = (reward == 1); terminated = is_success.detach().cpu().numpy().astype(bool)        (env.py:63-64)
 * mir_step_begin = mir_step_fused (same arguments, `terminated` = the device copy, nullable) that also stores the
 * terminated bytes into a pinned host buffer owned by the handle, straight from the kernel (no copy command);
 * mir_step_end blocks until THAT launch has delivered its terminated bytes and copies the B bytes into terminated_host (plain
 * host memory, nullable).  In mode 3 the kernel stores those bytes before its device-side outputs, so the other outputs of the
 * launch are ordered by the stream as after any launch (a later launch, copy or synchronize on it sees them), not by this call.  Between the two calls the host is free (the Python side prepares its return values there).
 * One mir_step_end per mir_step_begin; a step left open (the caller raised between the two calls) is closed by the next
 * mir_step_begin / mir_step_go / mir_reset, which wait for its bytes and drop them.  mir_step_end is otherwise the only entry point
 * of the library that waits for the device.
 * How the wait is done (mir_get_sync_mode; environment variable MIR_SYNC_MODE overrides at mir_create):
 *   3  (default) every terminated byte carries a 5-bit tag (1..31 in bits 1 .. 5, a counter only mir_step_begin advances; bits 6 and 7: exact contacts) that changes from
 *      launch to launch; the host spins until all B bytes show the tag of this launch -- no fence, no flag, nothing in the kernel
 *      waits for the PCIe acknowledgement
 *   2  every wave waits for its host store, the kernel's last workgroup then writes a sequence word into pinned host memory
 *      and the host spins on it (16-lane kernel only)
 *   1  hipStreamWriteValue32 behind the launch writes that word, the host spins on it
 *   0  hipStreamSynchronize
 * EARLY BYTES (mode 3, 16-lane kernel, scenes whose task object is a free body under the world: DevModel::term_bound_ok).  The
 * bytes mir_step_end returns may PRECEDE the end of the solve they belong to: a workgroup stores them from inside its Newton loop
 * once  |z_pred - reward_z| > 2 dt^2 ((1 + sqrt 2) |g|_w + 1 m/s^2) + 1e-5 m  holds for its four envs, where z_pred is the object's
 * height integrated from the current iterate and |g|_w^2 = sum_i w_i g_i^2 >= |g|^2_{Mt^-1} / mass over the dofs of the object's
 * block of the problem (all dofs while a contact joins it to the arm).  The solver's cost is 1-strongly convex in the Mt norm and
 * no accepted step raises it -- per tree, steps being accepted tree by tree, when the problem separates -- so the final iterate is within
 * 2 |g|_{Mt^-1} of the current one whatever makes the solver stop; the bound is that with a 2.4 x margin for float32 evaluation.
 * The kernel still compares the bytes it sent with the integrated state.  A difference (none in any test or soak run) is counted
 * (mir_debug_early_mask_stats), raises a sticky word in pinned memory, and the NEXT mir_step_begin / mir_step_go / mir_step_end /
 * mir_reset on the handle fails ONCE with MIR_E_MASK after switching the handle to late bytes for good (the step that failed the
 * check has already returned its mask: the caller learns that one of the masks since the last successful call was wrong).
 * MIR_NO_EARLY_MASK=1 at mir_create: the bytes always wait for the integrator. */
int mir_step_begin(MirHandle h, const float* action, float* agent_pos, float* env_state, float* reward,
                   uint8_t* terminated, void* stream);
int mir_step_end(MirHandle h, uint8_t* terminated_host);
int mir_get_sync_mode(MirHandle h);
/* How mir_step_begin launches (16-lane kernel; environment variable MIR_SPLIT_STEP overrides at mir_create):
 *   1  (default) ROTATED: a step's launch runs the action-dependent half of THIS step (smooth force with the new targets, solves,
 *      integration, terminated bytes, observations) and then the action-independent half of the NEXT step (poses, dynamics, collision
 *      detection, contact Jacobians) into a scratch buffer of the handle -- work that so runs while the host is between two calls.
 *      Bit-identical to the fused launch.  Whatever touches the state in between (reset, state write, any other step entry point)
 *      makes the next mir_step_begin start over with a fused launch.
 *   2  the same split as two launches (also the fallback where a scene's closing forward kinematics cannot be shared by the waves)
 *   0  one fused launch per step (the wave kernel always) */
int mir_get_split_step(MirHandle h);
/* mir_step_begin with the four output pointers registered ahead of time (mir_step_prepare touches no device state and is meant to
 * be called while the previous step's kernel is still running): the GPU idles in front of mir_step_go, which then takes three
 * arguments instead of seven.  One mir_step_prepare per mir_step_go (the registration is consumed when a launch is queued; the
 * latest registration wins). */
int mir_step_prepare(MirHandle h, float* agent_pos, float* env_state, float* reward, uint8_t* terminated);
int mir_step_go(MirHandle h, const float* action, void* stream);

/* EXACT CONTACTS for scenes on the 16-lane kernel (no reference counterpart: Genesis keeps every contact point of its 100+ candidate
 * pairs -- RigidOptions at gym_genesis/tasks/franka/cube_pick.py:46 -- while the 16-lane kernel keeps 16 per env and thins the
 * manifolds beyond that; the reference's own expert, examples/franka/pick_cube_state.py:33-41,86-88, drives 29 % of its env-steps
 * there).  With the switch on, a step launched by mir_step_begin / mir_step_go DEFERS every env whose narrowphase found more than 16
 * candidate points: the launch stores nothing for it and says so in bit 7 of its terminated byte; mir_step_end then steps exactly those
 * envs with MIR_MAX_CONTACT points, never thinned below that, from their untouched state rows, with the step's action and into the
 * step's output pointers, recomputes their part of the split step's hand-over, and returns when their terminated bytes have arrived
 * too.  Since round 6 they take ONE launch of the 16-lane kernel's list instantiation (three contacts per lane, four envs per
 * workgroup, the next step's hand-over included); an env beyond THAT capacity too -- more than 48 points (thinned to 48 as before) or
 * more than 16 candidate geom pairs -- goes to the wave-per-env kernel (the same scene compiled for it; 64 candidate pairs) as every
 * deferred env did in round 5 (MIR_EXACT_WAVE=1 in the environment at the time of the call: all of them still do).
 * `action` of the pending mir_step_begin / mir_step_go is read AGAIN by those launches: with the switch on it must stay valid, and
 * unchanged, until mir_step_end has returned; and the next mir_step_begin may name another stream (it is made to wait for them).  An env that is not deferred is computed exactly as without the switch; a
 * step without deferred envs launches nothing extra.  The state rows, outputs and link poses of a deferred env are those of the step
 * only once mir_step_end has returned: anything queued between mir_step_begin and mir_step_end -- a mir_render of the observation's
 * images, say -- sees its OLD rows (the task classes close the step before they draw).  `spec`: the spec the scene was created from (compiled once more, for the wave
 * kernel; may be NULL when switching back on).  While the switch is on, mir_step and mir_step_fused run as begin + end (they wait for the
 * step), and mir_step_packed / mir_rollout / mir_rollout_autoreset return MIR_E_INVALID (their steps are never closed on the host);
 * mir_rollout_exact / mir_rollout_autoreset_exact are the K-step rollouts that keep every contact point without the host (below).
 * MIR_E_INVALID for scenes of the wave kernel (nothing to do) and for sync modes other than 3.
 * mir_get_exact_stats: out4 = {steps closed by mir_step_end, steps that had deferred envs, deferred env-steps, most deferred envs in one
 * step} since the last reset of the counters (reset != 0 clears them).  mir_get_exact_route: out4 = {deferred env-steps handed to the
 * list instantiation, env-steps stepped by the wave-per-env kernel, HEAVY steps, steps of overflow runs as two launches} over the same period.  A heavy step: while at least
 * 1 / 16 of the envs are above 16 points (and until fewer than 1 / 32 are; MIR_EXACT_HEAVY="enter,leave" in envs, enter <= 0: never)
 * the whole batch is stepped by ONE launch of the three-contacts-per-lane instantiation instead of a launch that defers most envs and
 * a list launch behind it (an env with at most 16 points is computed there bit for bit as by the one-contact-per-lane kernel); the
 * statistics count its envs above 16 points as deferred.
 * OVERFLOW RUNS in a loop that leaves room between two steps (second session of round 6): when the caller spent at least 40 us
 * (MIR_EXACT_BIG_GAP) between mir_step_end's return and this mir_step_begin -- a policy, its IK -- a step of a run (from the step after
 * one that deferred envs until a step in which no env is above 16 points) is TWO launches of the three-contacts-per-lane instantiation for
 * the whole batch: the second half of the step from the scratch rows up to the outputs and the terminated bytes, on `stream`; and the first
 * half of the next step on the library's side stream, beside whatever the caller queues on `stream` next (the next mir_step_begin is made
 * to wait for it) -- the second half as two list launches once the first half has said which envs are above 16 points: those on the
 * three-contacts-per-lane instantiation, the others in one round of the one-contact-per-lane kernel's workgroups on the side stream.
 * Same results bit for bit; less time inside the two calls, a third more GPU time per step.  MIR_EXACT_BIG=0: never
 * (heavy phase / list launches), 2: whenever the rows are there.  out4[3] of mir_get_exact_route counts such steps.
 * on = 2 (tests): every env of every step is deferred, i.e. the whole batch is stepped by the launches that otherwise serve the
 * deferred envs only -- the twin the parity tests compare a deferred env with, bit for bit. */
int mir_set_exact_contacts(MirHandle h, const MirSceneSpec* spec, int32_t on);
int mir_get_exact_contacts(MirHandle h);
int mir_get_exact_stats(MirHandle h, uint64_t* out4, int32_t reset);
int mir_get_exact_route(MirHandle h, uint64_t* out4);

/* Same step, but every output of an env lands in ONE packed float32 row
 * rows[e*row_stride + ...] = [agent_pos (agent_dim) | env_state (env_dim) | reward | terminated(0/1)]
 * so a sharded run gathers all per-step outputs with a single collective
 * (row_stride >= agent_dim + env_dim + 2, in floats). */
int mir_step_packed(MirHandle h, const float* action, float* rows, int32_t row_stride, void* stream);

/* K consecutive env.step() calls in ONE launch (the "multi-step variant for rollouts" of SURVEY.md 7-7; the loop shape of
 * README.md:30-43 with the actions already on the device): for k < n_steps: targets <- actions[k] (B,nu); one physics step;
 * rows[k] (B,row_stride) <- packed outputs as in mir_step_packed.  actions (n_steps,B,nu), rows (n_steps,B,row_stride).
 * Bit-identical to n_steps calls of mir_step_packed; the state never leaves the chip between the steps. */
int mir_rollout(MirHandle h, const float* actions, int32_t n_steps, float* rows, int32_t row_stride, void* stream);

/* mir_rollout with the episode loop of mir_autoreset inside the launch: after every step the packed row (the terminal
 * observation of envs that just ended) is written, then episode_len / truncation / re-spawn are applied exactly as
 * mir_autoreset does, on chip.  rows[k][e][agent_dim + env_dim + 2] = truncated (row_stride >= agent_dim + env_dim + 3).
 * Bit-identical to n_steps x (mir_step_packed; mir_autoreset). */
int mir_rollout_autoreset(MirHandle h, const float* actions, int32_t n_steps, float* rows, int32_t row_stride, int32_t* episode_len,
                          int32_t max_len, const float* spawn_pool, int32_t pool_len, int32_t* cursor, const float* obj_quat,
                          const float* arm_qpos, void* stream);

/* K-step rollouts that KEEP EVERY CONTACT POINT (exact contacts on) without the host between the steps: arguments and rows as
 * mir_rollout / mir_rollout_autoreset, results bit-identical to n_steps x (mir_step_begin; mir_step_end) -- with mir_autoreset behind
 * each step for the second call -- under the same switch.  With the switch off they ARE mir_rollout / mir_rollout_autoreset.  The call
 * queues a fixed chain on `stream` (no host read, no pinned memory, no host wait): a memset of two device counters; the one-wave step
 * loop for the whole batch, which hands an env off to a device list at its first step above the one-contact-per-lane capacity (more
 * candidate points than 16 lanes, or more than 16 candidate pairs; on = 2: every env at step 0); one launch of the
 * three-contacts-per-lane instantiation (48 points) whose step loop takes each env of that list from its own step -- an env that comes back to
 * 16 points or fewer stays there for the rest of the call, which is the same bits (an env within 16 points is computed there bit for
 * bit as by the one-contact-per-lane kernel); the wave-per-env kernel (48 points, 64 candidate pairs) for an env beyond THAT
 * capacity, from that step to the end of the call; and a one-thread statistics kernel.  The bits are the host-closed route's for every
 * env that stays within 48 points and 16 candidate pairs, or that once beyond them stays beyond them for the rest of the call: an env
 * that comes back under that capacity after the wave kernel has taken it finishes the call on the wave kernel -- the same contact
 * model (48 points, 64 candidates), other bits.  A scene without the split closing forward kinematics (or with MIR_EXACT_WAVE set),
 * whose host-closed route sends every deferred env to the wave kernel, hands them to the wave kernel here too.  n_steps < 2^20.  A pending step is closed first; `stream` waits for the side-stream launches of an
 * earlier host-closed step.  MIR_E_INVALID: null arguments, a short row_stride, a scene of the wave kernel (nothing to switch).
 * mir_get_rollout_exact_stats: out4 = {calls that went the device-resident way, env-steps on the three-contacts-per-lane
 * instantiation, env-steps on the wave kernel, most envs handed off in one call} since the last reset (reset != 0 clears them).  It
 * reads device counters: it synchronises the device. */
int mir_rollout_exact(MirHandle h, const float* actions, int32_t n_steps, float* rows, int32_t row_stride, void* stream);
int mir_rollout_autoreset_exact(MirHandle h, const float* actions, int32_t n_steps, float* rows, int32_t row_stride, int32_t* episode_len,
                                int32_t max_len, const float* spawn_pool, int32_t pool_len, int32_t* cursor, const float* obj_quat,
                                const float* arm_qpos, void* stream);
int mir_get_rollout_exact_stats(MirHandle h, uint64_t* out4, int32_t reset);

/* get_obs() without stepping */
int mir_get_obs(MirHandle h, float* agent_pos, float* env_state, float* reward, uint8_t* terminated,
                void* stream);

/* full simulation state; any pointer may be NULL.  qpos (B,nq) qvel (B,nv)
 * target (B,nu) warmstart (B,nv) */
int mir_get_state(MirHandle h, float* qpos, float* qvel, float* target, float* warmstart, void* stream);
int mir_set_state(MirHandle h, const float* qpos, const float* qvel, const float* target,
                  const float* warmstart, void* stream);

/* link.get_pos / get_quat for all bodies: pos (B,nbody,3) quat (B,nbody,4) */
int mir_get_links(MirHandle h, float* pos, float* quat, void* stream);

/* per-env diagnostics of the last step: ncon (B) i32, nefc (B) i32, niter (B) i32; nullable.  The step kernels write them
 * (16 B per env-step) while they are switched on: mir_set_diag(h, 0) drops that traffic (the task classes do), after which
 * mir_get_diag is an error until they are switched on again.  On by default. */
int mir_set_diag(MirHandle h, int32_t on);
int mir_get_diag(MirHandle h, int32_t* ncon, int32_t* nefc, int32_t* niter, void* stream);
/* mir_get_diag + ncand_points (B) i32, nullable: the contact points the narrowphase found BEFORE the scene's contact capacity was
 * applied (MirOptions.max_contacts; 16 at most in the 16-lane kernel, 48 in the wave kernel).  ncand_points > capacity = the
 * manifolds of that env-step were thinned (oracle/orc_rigid.c: thin_manifolds); the fraction of such env-steps is what bench.py and
 * the reference-expert tests report as cap_hit_frac.  Saturates at 255. */
int mir_get_diag4(MirHandle h, int32_t* ncon, int32_t* nefc, int32_t* niter, int32_t* ncand_points, void* stream);

/* Divergence guard (the reference's users get Genesis's own error on a NaN state, scene.step() at
 * gym_genesis/tasks/franka/cube_pick.py:107,125).  While diagnostics are on, a step kernel flags every env whose integrated qpos / qvel
 * holds a NaN or an Inf: bad (B) u8 device, nullable <- 1 for the envs flagged by the LAST step launch (sticky over the steps of a
 * rollout launch); *env_steps (host, nullable) <- env-steps flagged since the counter was last reset (synchronises the stream);
 * reset != 0 clears the counter.  Off the hot path: nothing is computed or stored while diagnostics are off (mir_set_diag(h, 0)).
 * A flagged env keeps stepping (its state stays non-finite until it is reset); its reward is 0 and its `terminated` False -- the
 * threshold tests hold for finite heights only -- and no other env is affected (bit-identical to a run without it). */
int mir_get_bad(MirHandle h, uint8_t* bad, uint32_t* env_steps, int32_t reset, void* stream);

/* stage outputs of one forward-dynamics evaluation at the current state (no
 * integration), for per-stage parity tests: M (B,nv,nv), qfrc_bias (B,nv),
 * qacc_smooth (B,nv), qacc (B,nv); nullable */
int mir_forward(MirHandle h, float* M, float* qfrc_bias, float* qacc_smooth, float* qacc, void* stream);

/* ---- contact force sensing -----------------------------------------------------------------------
 * entity.get_links_net_contact_force() / entity.get_contacts() of Genesis (RigidEntity; the reference's tasks do not call them --
 * gym_genesis/tasks/franka/cube_pick.py:140-163 reads poses only -- but they are what its users reach for next: grasp detection,
 * force rewards, tactile observations).
 * One forward-dynamics evaluation AT THE CURRENT STATE WITH THE CURRENT PD TARGETS (as mir_forward: poses, dynamics, collision,
 * constraint rows, Newton solve, no integration): the contact forces that the next step applies if the targets stay as they are.
 * (Genesis and MuJoCo report the forces of the step just taken, i.e. of the state BEFORE the last step.)
 * The read changes nothing a later call can see: state, targets, warm start, episode bookkeeping, the state version, link poses,
 * diagnostics and all counters stay as they were, and the steps around it are bit for bit those of a run without it.
 *   n_contacts (B) i32; flags (B) u8 -- bit 0: the narrowphase found more candidate points (or pairs) than the serving kernel holds
 *     (MIR_MAX_CONTACT points; 16 candidate pairs on the 16-lane kernel), the forces are those of the thinned manifold;
 *   ids (B, MIR_MAX_CONTACT, 4) i32: geom_a, geom_b, link_a, link_b (indices of the spec), in the solver's contact order; the
 *     pointer must be 16-byte aligned (a row is one vector store);
 *   pos_normal_pen (B, MIR_MAX_CONTACT, 7): position (world), normal (world, from a to b), penetration depth (> 0 = overlap);
 *   force (B, MIR_MAX_CONTACT, 3): world force ON LINK b (link a receives the opposite), sum over the contact's four friction-pyramid
 *     rows of f_r (n + s_r mu t), f_r = -D min(0, J_r a - aref_r);
 *   link_force (B, nbody, 3): per link the sum of `force` over its contacts as b minus the sum over its contacts as a (the world,
 *     link 0, included: the links of an env sum to zero).  Joint-limit rows contribute to neither output.
 * Rows >= n_contacts of the three lists are zeroed.  Every output is nullable, each is written only when asked for (link_force alone
 * costs no list traffic).  Scenes on the 16-lane kernel are served by a launch of their own with 48 points per env whatever the
 * scene's max_contacts (every point a step with exact contacts keeps); scenes on the wave-per-env kernel by its forward mode.
 * MIR_E_INVALID while a mir_step_begin is open.  (An added entry point: MIR_VERSION and every struct stay as they are.) */
int mir_contact_forces(MirHandle h, int32_t* n_contacts, uint8_t* flags, int32_t* ids, float* pos_normal_pen, float* force,
                       float* link_force, void* stream);

/* ---- link poses, velocities and Jacobians -----------------------------------------------------------
 * robot.get_jacobian(link) / entity.get_links_pos / get_links_quat / get_links_vel / get_links_ang / link.get_vel() / link.get_ang()
 * of Genesis (RigidEntity, RigidLink; the reference's tasks read poses only -- gym_genesis/tasks/franka/cube_pick.py:140-146 -- but
 * these are what operational-space, resolved-rate and impedance controllers and velocity observations are written on).
 * ONE launch of a kernel of its own for a LIST of links of a LIST of envs: it reads qpos / qvel and the compiled model and writes only
 * its outputs (mir_get_links, the other way to a link pose, runs the step kernel over every body of every env).
 *   R = n_rows, or num_envs when env_idx is NULL; row k belongs to env env_idx[k] (int64, device; repeats and any order allowed; an
 *   index outside the batch is clamped as in mir_inverse_kinematics_rows).  L = q->n_links.
 * Definitions (the oracle's conventions: oracle/orc_rigid.c orc_fk for the poses; MIR_JNT_FREE above for the free joint -- qvel = world
 * linear velocity of the body origin, then world angular velocity; the integrator's q <- exp(w dt) (x) q).  With o_b, R_b the world pose
 * of body b from the forward kinematics of the current qpos, and p = o_link + R_link local_point:
 *   pos  (R, L, 3) = p;   quat (R, L, 4) = the link's world quaternion (wxyz), normalised, with the sign the forward kinematics gives it;
 *   jac  (R, L, 6, n_dofs) row-major: rows 0-2 map qvel to the world linear velocity of p, rows 3-5 to the link's world angular
 *        velocity; its columns are the scene dofs [dof0, dof0 + n_dofs).  The column of scene dof d, which belongs to body b:
 *            b on the path world -> link, revolute with world axis a = R_b axis:   [a x (p - o_b); a]
 *            b on the path, prismatic:                                             [a; 0]
 *            b on the path, free, linear dof k:                                    [e_k; 0]
 *            b on the path, free, angular dof k:                                   [e_k x (p - o_b); e_k]
 *            b not on the path:                                                    zeros (written, not left as they were)
 *   vel  (R, L, 6) = J_full qvel over ALL scene dofs on the path: world linear velocity of p, then world angular velocity of the link.
 *        It does not depend on dof0 / n_dofs.
 * Every output is nullable and written only when asked for; all four NULL, or R == 0, or an empty result: MIR_OK without a launch.
 * jac should be 16-byte aligned (a block then leaves as 16-byte stores; any 4-byte aligned address works).
 * A read changes nothing: state, targets, warm start, state version, pose cache, diagnostics, counters and the scratch row of a split
 * step stay as they are, and the steps around it are bit for bit those of a run without it.  Between two steps of any stepping path
 * the poses are those of the state mir_get_links sees at that moment.
 * MIR_E_INVALID: a NULL handle or query, struct_size != sizeof(MirKinQuery), n_links outside 1 .. MIR_MAX_BODY, a link outside
 * 1 .. nbody - 1, columns outside [0, nv], a call while a mir_step_begin is open (the state is between the two halves of a step: the
 * rule of mir_contact_forces).  MIR_E_CAPACITY: a path world -> link of more than 16 bodies (the limit of mir_inverse_kinematics).
 * None of them launches anything.  (An added struct and entry point: MIR_VERSION and every other struct stay as they are.) */
typedef struct MirKinQuery {
  int32_t struct_size;                  /* = sizeof(MirKinQuery) */
  int32_t n_links;                      /* 1 .. MIR_MAX_BODY */
  int32_t link_body[MIR_MAX_BODY];      /* body indices of the spec, 1 .. nbody-1, repeats allowed */
  float local_point[MIR_MAX_BODY][3];   /* per queried link: point in the link's frame (0 = link origin) */
  int32_t dof0, n_dofs;                 /* Jacobian columns = scene dofs [dof0, dof0 + n_dofs) */
} MirKinQuery;
int mir_kin_query_sizeof(void);
int mir_link_kinematics(MirHandle h, const MirKinQuery* q, const int64_t* env_idx /* device, nullable */, int32_t n_rows,
                        float* pos /* (R, L, 3) */, float* quat /* (R, L, 4) wxyz */, float* vel /* (R, L, 6) lin, ang */,
                        float* jac /* (R, L, 6, n_dofs) */, void* stream);

/* ---- rigid-body dynamics queries: mass matrix, bias forces, inverse dynamics --------------------------------
 * entity.get_mass_mat() / entity.get_dofs_control_force() of Genesis (RigidEntity), and with them gravity compensation and the
 * feed-forward torque tau = M qacc + c along a planned trajectory: beside the Jacobian of mir_link_kinematics, the objects that
 * operational-space and impedance controllers are written on.  ONE launch of a kernel of its own for a WINDOW of scene dofs of a LIST of
 * envs: it reads qpos / qvel / the PD targets and the compiled model and writes only its outputs (mir_forward, the other way to M and
 * qfrc_bias, runs the step kernel with collision, constraint rows and the Newton solve over every env and returns all nv x nv).
 *   R = n_rows, or num_envs when env_idx is NULL; row k belongs to env env_idx[k] (int64, device; repeats and any order allowed; an
 *   index outside the batch is clamped as in mir_link_kinematics).  n = q->n_dofs; the window is the scene dofs [dof0, dof0 + n).
 * State overrides: qpos (R, nq) and / or qvel (R, nv), in the public layout of mir_get_state; row k replaces the current state of env
 * env_idx[k] for this evaluation only (a free joint's quaternion is normalised as the forward kinematics does).  What is not
 * overridden comes from the current state of env env_idx[k]; the PD targets always do.
 * Definitions (the oracle's conventions: oracle/orc_rigid.c orc_crb, orc_rne, orc_smooth; MIR_JNT_FREE above for the free joint --
 * qvel = world linear velocity of the body origin, then world angular velocity; generalized forces are dual to that qvel):
 *   M          (R, n, n) row-major: the window block of the joint-space inertia by the composite-rigid-body algorithm, WITH the dofs'
 *              armature on the diagonal and WITHOUT the dt (damping + kv) the implicit integrator adds for its own solve.  Symmetric,
 *              both triangles written; entries that couple different kinematic trees are exact zeros (written, not left as they were).
 *   bias       (R, n): recursive Newton-Euler at qacc = 0 with gravity: Coriolis, centrifugal and gravity forces, on the LEFT of
 *              M qacc + bias = tau_applied.
 *   gravity    (R, n): bias evaluated at qvel = 0: the torque that holds the pose at rest.
 *   tau        (R, n): the window of M_full qacc + bias for the full-length qacc (R, nv): inverse dynamics.  Passive damping and the
 *              PD torques are not in it.
 *   ctrl_force (R, n): clamp(kp (target - q) - kv qvel, force range) for MIR_CTRL_POSITION dofs, 0 for the others: the PD torque the
 *              next step applies if the targets stay as they are.
 * Every output is nullable and written only when asked for; all five NULL, or R == 0, or n == 0: MIR_OK without a launch.
 * A read changes nothing: state, targets, warm start, state version, pose cache, diagnostics, counters and the scratch row of a split
 * step stay as they are, and the steps around it are bit for bit those of a run without it.
 * MIR_E_INVALID: a NULL handle or query, struct_size != sizeof(MirDynQuery), a window outside [0, nv], an unknown flag bit, tau without
 * qacc, a free joint that is not the root of its tree, a call while a mir_step_begin is open (the rule of mir_contact_forces).
 * MIR_E_CAPACITY: R x n x n does not fit 2^31 - 1; a
 * kinematic tree of more than 16 bodies or 15 dofs, or more than 20 trees with dofs (neither compiler produces such a scene today).
 * None of them launches anything.  (An added struct and entry point: MIR_VERSION and every other struct stay as they are.) */
typedef struct MirDynQuery {
  int32_t struct_size;   /* = sizeof(MirDynQuery) */
  int32_t dof0, n_dofs;  /* window of scene dofs [dof0, dof0 + n_dofs) */
  uint32_t flags;        /* 0; unknown bits are MIR_E_INVALID */
} MirDynQuery;
int mir_dyn_query_sizeof(void);
int mir_dynamics(MirHandle h, const MirDynQuery* q, const int64_t* env_idx /* device, nullable */, int32_t n_rows,
                 const float* qpos /* (R, nq) device, nullable: evaluate here instead of at the current state */,
                 const float* qvel /* (R, nv) nullable, likewise */, const float* qacc /* (R, nv) nullable; needed for tau only */,
                 float* M /* (R, n_dofs, n_dofs) */, float* bias /* (R, n_dofs) */, float* gravity /* (R, n_dofs) */,
                 float* tau /* (R, n_dofs) */, float* ctrl_force /* (R, n_dofs) */, void* stream);

/* ---- link accelerations and IMU readings -------------------------------------------------------------
 * entity.get_links_acc() and gs.sensors.IMU of Genesis (RigidEntity; parity with Genesis unpinned: the reference's tasks read neither),
 * and the term Jdot qvel of operational-space control, a = J qacc + Jdot qvel with J the Jacobian of mir_link_kinematics.
 * ONE launch of a kernel of its own for a LIST of links of a LIST of envs: it reads qpos / qvel, the caller's qacc and the compiled
 * model and writes only its outputs.
 *   R = n_rows, or num_envs when env_idx is NULL; row k belongs to env env_idx[k] (int64, device; repeats and any order allowed; an
 *   index outside the batch is clamped as in mir_link_kinematics).  L = q->n_links.  qacc (R, nv) is in the public dof order of
 *   mir_get_state, row k for row k of the outputs; the state is the current one.
 * Definitions (the conventions of mir_link_kinematics: a free joint's qvel is the world linear velocity of the body origin, then the
 * world angular velocity, qacc its time derivative).  With o, R, w the world pose and angular velocity of the link,
 * p = o + R local_point the material point of the link that is there now:
 *   acc      (R, L, 6): rows 0-2 the classical world linear acceleration d^2 p / dt^2, rows 3-5 the link's world angular acceleration:
 *            J qacc + Jdot qvel over all scene dofs.  Gravity is not added: it is in qacc already.
 *   bias_acc (R, L, 6): the same at qacc = 0, Jdot qvel.  It needs no qacc and does not depend on it, to the bit.
 *   imu      (R, L, 6): rows 0-2 R_s^T (d^2 p / dt^2 - g), rows 3-5 R_s^T w, with R_s = R R(quat_offset[l]) the sensor's axes and g the
 *            gravity vector of the scene spec (opt.gravity): a sensor at rest reads +9.81 along the world's up axis, in its own frame.
 * Every output is nullable and written only when asked for; all three NULL, or R == 0: MIR_OK without a launch.
 * A read changes nothing: state, targets, warm start, state version, pose cache, diagnostics, counters and the scratch row of a split
 * step stay as they are, and the steps around it are bit for bit those of a run without it.
 * MIR_E_INVALID: a NULL handle or query, struct_size != sizeof(MirAccQuery), n_links outside 1 .. MIR_MAX_BODY, a link outside
 * 1 .. nbody - 1, a local_point or quat_offset that is not finite, an unknown flag bit, acc or imu without qacc (the rule of tau in
 * mir_dynamics), a free joint below another body (its qvel would mix two conventions: the rule of mir_dynamics), a call while a
 * mir_step_begin is open.  MIR_E_CAPACITY: a path world -> link of more than 16 bodies.  None of them launches anything.
 * (An added struct and entry point: MIR_VERSION and every other struct stay as they are.) */
typedef struct MirAccQuery {
  int32_t struct_size;                  /* = sizeof(MirAccQuery) */
  int32_t n_links;                      /* 1 .. MIR_MAX_BODY */
  int32_t link_body[MIR_MAX_BODY];      /* body indices of the spec, 1 .. nbody-1, repeats allowed */
  float local_point[MIR_MAX_BODY][3];   /* per queried link: point in the link's frame (0 = link origin) */
  float quat_offset[MIR_MAX_BODY][4];   /* per queried link: sensor axes in the link's frame, wxyz, normalised by the library; all-zero = identity */
  uint32_t flags;                       /* 0; unknown bits are MIR_E_INVALID */
} MirAccQuery;
int mir_acc_query_sizeof(void);
int mir_link_accelerations(MirHandle h, const MirAccQuery* q, const int64_t* env_idx /* device, nullable */, int32_t n_rows,
                           const float* qacc /* (R, nv) device, public layout, nullable: needed for acc and imu */,
                           float* acc /* (R, L, 6) lin, ang */, float* bias_acc /* (R, L, 6) */, float* imu /* (R, L, 6) lin, gyro */,
                           void* stream);

/* ---- operational-space dynamics: M^-1, task-space inertia, J-bar ---------------------------------------------
 * The step from M (mir_dynamics), J (mir_link_kinematics) and Jdot qvel (mir_link_accelerations) to an operational-space or impedance
 * controller, and forward dynamics qacc = M^-1 (tau - bias) (parity with Genesis unpinned: the reference's tasks call none of it).
 * ONE launch of a kernel of its own for a LIST of links of a LIST of envs: it reads qpos and the compiled model and writes only its
 * outputs.  Everything here depends on qpos only.
 *   R = n_rows, or num_envs when env_idx is NULL; row k belongs to env env_idx[k] (int64, device; repeats and any order allowed; an
 *   index outside the batch is clamped as in mir_dynamics).  L = q->n_links; n = q->n_dofs, the window of scene dofs [dof0, dof0 + n).
 *   The window selects which rows and columns are WRITTEN; it never changes the matrix that is inverted, which is always the whole
 *   block of a kinematic tree.
 * State override: qpos (R, nq) in the public layout of mir_get_state, the rule of mir_dynamics: row k replaces the current qpos of env
 * env_idx[k] for this evaluation only.
 * Definitions.  M is the full joint-space inertia of mir_dynamics (armature on the diagonal, no dt (damping + kv)).  J is the 6 x nv
 * Jacobian of mir_link_kinematics at p = o_link + R_link local_point: linear rows first, then angular, with the free-joint convention
 * of MIR_JNT_FREE.
 *   minv       (R, n, n) row-major: the window of M^-1.  Symmetric, both triangles written, bitwise symmetric; entries between
 *              different kinematic trees are exact zeros (written, not left as they were).
 *   solve      (R, n): the window of M^-1 x for the full-length x (R, nv), public dof order.  Forward dynamics is x = tau - bias with
 *              the bias of mir_dynamics.
 *   lambda_inv (R, L, 6, 6): J M^-1 J^T, the task-space mobility.  Both triangles written by one owner: bitwise symmetric.  Always finite.
 *   lambda     (R, L, 6, 6): (J M^-1 J^T + damping^2 I)^-1, the operational-space inertia.
 *   jbar       (R, L, n, 6): the window rows of M^-1 J^T lambda, the dynamically consistent generalised inverse of J.  With
 *              damping = 0, J jbar = I.
 * Singular task spaces (a link with fewer than six dofs on its path; an arm at a singularity).  The 6 x 6 matrix
 * A = J M^-1 J^T + damping^2 I is factored by Cholesky without pivoting.  If a pivot -- the remainder a_jj - sum_k c_jk^2 of which the
 * square root would be taken -- is <= 1e-5 x the largest diagonal entry of A, lambda and jbar of that (row, link) are written as quiet
 * NaNs; nothing else is affected and the call still returns MIR_OK.  A relative pivot of 1e-5 means a condition number beyond what
 * float32 can invert meaningfully; damping > 0 is the remedy.
 * Every output is nullable and written only when asked for; all five NULL, or R == 0, or an empty result (n == 0 with no lambda_inv /
 * lambda asked for): MIR_OK without a launch.  Any 4-byte aligned address works; every element is written exactly once.
 * A read changes nothing: state, targets, warm start, state version, pose cache, diagnostics, counters and the scratch row of a split
 * step stay as they are, and the steps around it are bit for bit those of a run without it.
 * MIR_E_INVALID: a NULL handle or query, struct_size != sizeof(MirTaskQuery), n_links outside 0 .. MIR_MAX_BODY, a link outside
 * 1 .. nbody - 1, a link whose kinematic tree has no dofs, a local_point or damping that is not finite, damping < 0, a window outside
 * [0, nv], an unknown flag bit, solve without x, lambda_inv / lambda / jbar with n_links == 0, a free joint that is not the root of its
 * tree, a call while a mir_step_begin is open.  MIR_E_CAPACITY (the limits of mir_dynamics): a kinematic tree of more than 16 bodies
 * or 15 dofs, more than 20 trees with dofs, an output asked for whose element count exceeds 2^31 - 1.  None of them launches anything.
 * (An added struct and entry point: MIR_VERSION and every other struct stay as they are.) */
typedef struct MirTaskQuery {
  int32_t struct_size;                  /* = sizeof(MirTaskQuery) */
  int32_t n_links;                      /* 0 .. MIR_MAX_BODY (0: only minv / solve) */
  int32_t link_body[MIR_MAX_BODY];      /* body indices of the spec, 1 .. nbody-1, repeats allowed */
  float local_point[MIR_MAX_BODY][3];   /* task point in the link frame (0 = link origin) */
  int32_t dof0, n_dofs;                 /* window of scene dofs for the dof-indexed outputs */
  float damping;                        /* >= 0, finite; damping^2 is added to the diagonal of lambda_inv before it is inverted */
  uint32_t flags;                       /* 0; unknown bits are MIR_E_INVALID */
} MirTaskQuery;
int mir_task_query_sizeof(void);
int mir_task_dynamics(MirHandle h, const MirTaskQuery* q, const int64_t* env_idx /* device, nullable */, int32_t n_rows,
                      const float* qpos /* (R, nq) device, nullable: evaluate here instead of at the current qpos */,
                      const float* x /* (R, nv) nullable; needed for solve only */,
                      float* minv /* (R, n, n) */, float* solve /* (R, n) */,
                      float* lambda_inv /* (R, L, 6, 6) */, float* lambda /* (R, L, 6, 6) */,
                      float* jbar /* (R, L, n, 6) */, void* stream);

/* ---- range sensing: batched ray casts ------------------------------------------------------------------
 * scene.add_sensor(gs.sensors.Lidar / Raycaster / DepthCamera(...)) + sensor.read() -> points, distances of Genesis (parity with
 * Genesis unpinned: the reference's tasks cast no rays and the package is not in the reference tree; the names follow its sensor API
 * as far as it is remembered).  Obstacle distances, wrist range finders, height scans, clearance rewards.  cam.render(depth=True),
 * the other way to a distance, is tied to a pinhole raster, reports planar depth and draws every hull as its bounding box.
 * ONE launch of a kernel of its own for N rays of ONE sensor on R rows: it reads the link poses and the compiled model and writes only
 * its outputs.
 *   R = n_rows, or num_envs when env_idx is NULL; row k belongs to env env_idx[k] (int64, device; repeats and any order allowed; an
 *   index outside the batch is clamped as in mir_link_kinematics).  N = q->n_rays; dirs (N, 3) is shared by all rows.
 * Ray.  With o_link, R_link the world pose of body q->link_body (0: the world, identity):  sensor origin o = o_link + R_link pos_offset,
 *   sensor axes R_s = R_link R(quat_offset);  ray i is  o + t R_s d_i / |d_i|,  t >= 0 -- t is Euclidean range.  A zero direction
 *   reports no hit.
 * Surfaces.  Every geom of the spec whose bit in skip_geoms is clear, in the env's own frame (no env offsets).  Plane: two-sided,
 *   unbounded.  Box, sphere, capsule: exact (a sphere is a capsule with hl = 0).  Hull: the exact convex polytope of its vertices, not
 *   its bounding box (face planes by brute force over vertex triples, once per handle, at the first call).  A solid that contains the
 *   origin is not seen (the rasteriser's rule for a camera inside a solid: a sensor inside its own link's capsule works without
 *   skip_geoms).  The nearest entry wins, ties go to the lower geom index.
 * Outputs.  With t_hit the winning entry (no hit, or a hit beyond max_range: a miss):
 *   distance (R, N)    = clamp(t_hit, min_range, max_range); max_range on a miss;
 *   geom     (R, N)    = the hit's geom index of the spec, -1 on a miss (a hit nearer than min_range keeps its geom and normal);
 *   points   (R, N, 3) = distance x the unit direction in the sensor's frame (distance d^), or with MIR_RAY_POINTS_WORLD the origin plus
 *                        that, in world axes;
 *   normal   (R, N, 3) = the unit outward normal at the hit in the axes of `points`, 0 on a miss; a plane's normal faces the origin.
 * Every output is nullable and written only when asked for; all four NULL, or R == 0: MIR_OK without a launch.  points / normal leave
 * as 16-byte stores whatever their alignment (any 4-byte aligned address works).
 * A read changes nothing a later call can see: state, targets, warm start, state version, diagnostics, counters and the scratch row of
 * a split step stay as they are, and the steps around it are bit for bit those of a run without it.  The link poses come from the
 * rasteriser's pose cache: when the state has moved since the cache was written the call first refreshes it, exactly as mir_render
 * does (one forward-kinematics launch; tests/test_gpu_raycast.py holds the steps around it to the bits).  Unlike mir_render it does not
 * make the step launches write the cache themselves: they stay the launches they were.
 * MIR_E_INVALID: a NULL handle, query or dirs; struct_size != sizeof(MirRayQuery); n_rays < 1; a link outside 0 .. nbody - 1; ranges
 * that are not finite or not 0 <= min_range < max_range; an unknown flag bit; a skip_geoms bit at or above ngeom; an offset that is not
 * finite or a zero quat_offset; a call while a mir_step_begin is open (the rule of the two other sensing calls); a hull without volume.
 * MIR_E_CAPACITY: R x N, or the R x ceil(N / 256) workgroups, do not fit 2^31 - 1.  None of them launches anything.
 * (An added struct and entry point: MIR_VERSION and every other struct stay as they are.) */
#define MIR_RAY_POINTS_WORLD 1u   /* points / normal in world axes (default: the sensor's frame) */
typedef struct MirRayQuery {
  int32_t  struct_size;           /* = sizeof(MirRayQuery) */
  int32_t  link_body;             /* 0 = fixed in the world, else body 1 .. nbody-1 the sensor rides on */
  float    pos_offset[3], quat_offset[4]; /* sensor frame in the link's frame (wxyz, normalised by the library) */
  float    min_range, max_range;  /* 0 <= min_range < max_range, finite */
  int32_t  n_rays;                /* N >= 1 */
  uint32_t flags;
  uint64_t skip_geoms;            /* bit g set: geom g is not tested (MIR_MAX_GEOM = 40 < 64) */
} MirRayQuery;
int mir_ray_query_sizeof(void);
int mir_raycast(MirHandle h, const MirRayQuery* q, const float* dirs /* (N,3) device, sensor frame, shared by all rows */,
                const int64_t* env_idx /* device, nullable */, int32_t n_rows,
                float* distance /* (R,N) */, float* points /* (R,N,3) */, int32_t* geom /* (R,N) */, float* normal /* (R,N,3) */,
                void* stream);

/* ---- signed distance: batched point / sphere to scene queries ------------------------------------------
 * "How far is this point, or this arm, from the nearest thing?"  Proximity sensors, clearance rewards, potential fields, and the
 * clearance of a sphere model of an arm (spheres that ride on its links) at the current state or at candidate configurations, before
 * they are commanded (EntityView.get_clearance / in_collision; parity with Genesis unpinned).  mir_raycast measures along a direction and
 * does not see a solid that contains its origin; mir_contact_forces knows only pairs that already touch.
 * ONE launch of a kernel of its own for N probes, shared by all rows, on R rows: it reads the link poses (or the qpos rows given) and
 * the compiled model and writes only its outputs.
 *   R = n_rows, or num_envs when env_idx is NULL; row k belongs to env env_idx[k] (int64, device; repeats and any order allowed; an
 *   index outside the batch is clamped as in mir_link_kinematics).  N = q->n_probes <= 1024.
 * Probes.  probes (N, 4), device: centre xyz in the frame of the probe's link, radius >= 0.  probe_link (N), HOST memory, nullable (all
 *   probes stand in the world): 0 = the world, else body 1 .. nbody-1 the probe rides on.  It is a host array so that it is checked
 *   without a read-back; the library copies it into the launch's arguments, one byte per probe, which is where the cap of 1024 probes
 *   comes from.  Nothing of it is kept after the call returns.
 * Per-geom signed distance d_g, with the probe centre p in the geom's frame: negative inside, `closest` the nearest surface point.
 *   Plane: the solid is the half space z <= 0 (as in the step kernel): d = p.z, closest = (p.x, p.y, 0), normal +z.
 *   Sphere: d = |p| - r.  Capsule: d = |p - c| - r with c the point of the axis segment nearest p.
 *   Box: outside, the distance to clamp(p, -h, h); inside, max_i(|p_i| - h_i), closest on that face.
 *   Hull: the exact convex polytope of its vertices (as mir_raycast treats it).  Inside (every face plane <= 0): max_f(n_f . p - d_f),
 *   closest = the projection on that face.  Outside: the minimum over the hull's triangles of the closed-form point - triangle
 *   distance; the triangles are a fan per face, built with the face planes once per handle on the host at the first call.
 *   normal = the unit outward gradient of d_g in world axes.  Where it is not unique: +z of the geom frame at a sphere's centre and on
 *   a capsule's axis; the face of the lower index for an interior point equidistant from two faces and for a point exactly on the
 *   surface of a box or hull (box faces are indexed by axis x, y, z; hull faces in the order the table finds them, triples of vertex
 *   indices ascending).
 * Result per (row, probe).  s_g = d_g - radius over every geom whose bit in skip_geoms is clear; the lowest wins, ties go to the lower
 *   geom index.  s <= max_distance: distance = s, geom = its index of the spec, closest = the surface point in world axes (the env's own
 *   frame, no env offsets), normal as above.  Otherwise a miss: distance = max_distance, geom = -1, closest = the probe centre (world),
 *   normal = 0.  row_min (R) / row_argmin (R) = the lowest distance of the row and its probe index, the lower index on a tie (a row of
 *   misses: max_distance and 0).
 * Poses.  qpos NULL: the rasteriser's pose cache, refreshed exactly as mir_raycast does (one forward-kinematics launch, only when the
 *   state has moved since it was written).  qpos (R, nq), device: row k is the full configuration in the layout of mir_get_state, for
 *   this evaluation only; free-joint quaternions are normalised; the kernel computes the world pose of every body itself from the
 *   compiled model, parent before child (a free body's pose is its qpos pose; paths longer than 16 bodies: MIR_E_CAPACITY).  The pose
 *   cache is neither read nor written on this path.
 * Every output is nullable and written only when asked for; all six NULL, or R == 0: MIR_OK without a launch.
 * A call changes nothing a later call can see: state, targets, warm start, state version, diagnostics, counters and the scratch row of
 * a split step stay as they are, and the steps around it are bit for bit those of a run without it.
 * MIR_E_INVALID: a NULL handle, query or probes; struct_size != sizeof(MirDistQuery); n_probes < 1; a max_distance that is not finite
 * or not > 0; an unknown flag bit; a skip_geoms bit at or above ngeom; a probe_link outside 0 .. nbody - 1; a call while a
 * mir_step_begin is open; a hull without volume.  MIR_E_CAPACITY: N > 1024; R x N beyond 2^31 - 1.  None of them launches anything.
 * Not covered: robot geoms other than through spheres.  The sphere model against ITSELF is mir_self_distance's question
 * (below, "self-collision"); what lies BETWEEN two configurations is mir_path_clearance's, and the way from one to the other
 * mir_plan_path's (below).
 * (An added struct and entry point: MIR_VERSION and every other struct stay as they are.) */
typedef struct MirDistQuery {
  int32_t  struct_size;   /* = sizeof(MirDistQuery) */
  int32_t  n_probes;      /* N, 1 .. 1024 */
  float    max_distance;  /* > 0, finite */
  uint32_t flags;         /* 0; unknown bits are MIR_E_INVALID */
  uint64_t skip_geoms;    /* bit g set: geom g is not tested */
} MirDistQuery;
int mir_dist_query_sizeof(void);
int mir_signed_distance(MirHandle h, const MirDistQuery* q,
                        const float* probes /* (N,4) device: centre xyz in the link's frame, radius >= 0 */,
                        const int32_t* probe_link /* (N) HOST, nullable = all in the world; 0 = world, else body 1..nbody-1 */,
                        const int64_t* env_idx /* device, nullable */, int32_t n_rows,
                        const float* qpos /* (R,nq) device, nullable: evaluate at these configurations, not the current state */,
                        float* distance /* (R,N) */, int32_t* geom /* (R,N) */, float* closest /* (R,N,3) */, float* normal /* (R,N,3) */,
                        float* row_min /* (R) */, int32_t* row_argmin /* (R) */, void* stream);

/* ---- motion planning: batched collision-checked paths between two configurations ------------------------
 * `robot.plan_path(qpos_goal=q, num_waypoints=100)`: for R rows, ONE launch takes each row's arm from a start configuration to a goal
 * configuration through configurations whose sphere model (probes and probe_link exactly as in mir_signed_distance) keeps `margin`
 * from every geom that is not skipped.  mir_path_clearance answers the other question, "is this trajectory I already have clear?":
 * the swept check that mir_signed_distance disclaims.  Both read the state (or the start rows given) and the compiled model and write
 * only their outputs; rows, env_idx and clamping as in mir_signed_distance.  Parity with Genesis (OMPL) is unpinned: the planner is
 * this library's own, fixed in every detail below so that a reference can mirror it.  These two entry points test the sphere model
 * against the scene only; mir_plan_path_self and mir_path_clearance_self (below, "self-collision") add the model against itself.
 * Planned dofs.  dof_qadr (D), HOST: the qpos address of each planned dof, a revolute or prismatic joint with limits (an unlimited
 *   one, an address that is no such joint, a joint named twice: MIR_E_INVALID).  A configuration is the D values in this order.
 *   Every other entry of the row -- other joints, free bodies -- stays at qpos_start (R, nq), or at the current state when it is NULL.
 *   Every geom that is tested must ride on a body with no planned dof on its path to the world (MIR_E_INVALID otherwise: a moving
 *   obstacle is out of scope; put the arm's own geoms, and what it carries, into skip_geoms).
 * clear(q): the planned dofs of the row set to q, forward kinematics, the lowest (signed distance - radius) over the probes, capped at
 *   max_distance: clear when >= margin.  A configuration with a NaN or an infinity in it, one that puts a probe centre at such a
 *   value, and every configuration of a row in which a tested geom's pose is not finite (a free body's qpos) have the clearance
 *   -infinity: blocked, never "nothing near".
 * edge(a, b): n_sub = max(1, ceil(max_j |b_j - a_j| / resolution)), at most 4096; the configurations a + (i / n_sub)(b - a),
 *   i = 1 .. n_sub in order (the last one is b itself), the first blocked one ends the check.  Both quotients are float32 divisions
 *   refined by one Newton step (within an ulp of the exact quotient, independent of the build's division flags).  A query whose
 *   (hi_j - lo_j) / resolution exceeds 4096 for a planned dof is refused, so that inside the limits no edge reaches the cap.  Only the
 *   goal is checked against the limits: a start (or a point of a mir_path_clearance trajectory) so far outside them that an edge
 *   would need more than 4096 samples is sampled 4096 times, more coarsely than `resolution`, and nothing reports it.
 * u(env, c, j) = (x >> 8) 2^-24, x = mix(mix(mix(seed ^ env) ^ c) ^ j), mix = the 32-bit finaliser of MurmurHash3; env is the ENV
 *   index, not the row: a row's plan does not depend on the other rows of the call.
 * Algorithm (RRT-Connect).  1. goal outside [lo, hi] in a planned dof: GOAL_OUT_OF_LIMITS.  2. start not clear: START_IN_COLLISION;
 *   goal not clear: GOAL_IN_COLLISION.  3. edge(start, goal) holds: the polyline is [start, goal], iterations = 0.  4. Otherwise
 *   Ta = {start}, Tb = {goal}; for it = 0 .. max_iterations - 1 (iterations = it + 1): the active tree is Ta on even it, Tb on odd;
 *   q_rand_j = lo_j + u(env, it, j)(hi_j - lo_j); near = the node of the active tree nearest to q_rand (squared L2 over the planned
 *   dofs, summed j ascending; the lower index on a tie); q_new = near + min(1, step / |q_rand - near|)(q_rand - near); if
 *   edge(near, q_new) fails, next iteration; q_new joins the active tree.  Connect: c = the node of the other tree nearest to q_new;
 *   repeat: d = |q_new - c|; the target is q_new itself when d <= step, else c + (step / d)(q_new - c); if edge(c, target) fails, stop;
 *   the target joins the other tree with parent c and becomes c; when it was q_new the trees have met.  A node that has to join a tree
 *   of max_nodes nodes: NODE_LIMIT.  After the last iteration: ITERATION_LIMIT.  5. The parents of both trees give the polyline, start
 *   first, the meeting node once; more than MIR_PLAN_MAX_POLY nodes: PATH_TOO_LONG.  6. For s = 0 .. smooth_passes - 1, while the
 *   polyline has n >= 3 nodes: i = min(floor(u(env, 0x80000000 | s, 0) (n - 2)), n - 3), j = i + 2 + min(floor(u(env, 0x80000000 | s, 1)
 *   (n - 2 - i)), n - 3 - i) (float32 products); if edge(poly[i], poly[j]) holds the nodes between them are deleted.  7. Waypoint w of
 *   W = num_waypoints: the start's bits for w = 0, the goal's for w = W - 1, else the point at arc length (w / (W - 1)) x total of the
 *   polyline (L2 over the planned dofs), by linear interpolation inside its segment; a polyline of one segment is interpolated at
 *   t = w / (W - 1) itself.
 * Outputs.  path (R, W, D); status (R): MIR_PLAN_*; poly (R, MIR_PLAN_MAX_POLY, D), nullable: the polyline after smoothing, zeros behind
 *   its n_poly (R, nullable) nodes; stats (R, 4), nullable: iterations, nodes of Ta, nodes of Tb, configurations checked.  A row that
 *   fails returns its start W times (the arm stays put) and a polyline of one node.
 *   MIR_PLAN_IGNORE_COLLISION: every clear() is true and nothing is evaluated: the straight line (limits are still checked).
 * mir_path_clearance.  paths (R, K, D), K >= 2: seg_min (R, K-1) = the lowest clear() value over the samples of the edge rule on each
 *   segment (the segment's first point counts for segment 0 only); row_min (R); row_first_blocked (R) = the first segment whose minimum
 *   is < margin, or -1.  Every sample is evaluated, K is streamed.  It reads n_probes, n_dofs, resolution, margin, max_distance, flags
 *   and skip_geoms of the query.  All three outputs NULL: MIR_OK without a launch.
 * The trees live in LDS: sizeof of the fixed part + 2 max_nodes (4 D + 2) bytes must fit 64 KB, else MIR_E_CAPACITY, as N > 1024.
 * MIR_E_INVALID: a NULL handle, query, probes, dof_qadr, goal, path or status; a struct_size that is not sizeof(MirPlanQuery); n_probes
 * < 1; n_dofs outside 1 .. 16; num_waypoints < 2; max_nodes < 2; negative max_iterations or smooth_passes; resolution or step not
 * finite or <= 0; margin < 0; max_distance <= margin; an unknown flag bit; a skip_geoms bit at or above ngeom; a probe_link outside
 * 0 .. nbody - 1; a call while a mir_step_begin is open; a hull without volume; K < 2.  None of them launches anything.
 * A call changes nothing a later call can see, as for mir_signed_distance.
 * (Added structs and entry points: MIR_VERSION and every other struct stay as they are.) */
#define MIR_PLAN_MAX_POLY 128
#define MIR_PLAN_IGNORE_COLLISION 1u /* MirPlanQuery.flags */
#define MIR_PLAN_OK 0
#define MIR_PLAN_GOAL_OUT_OF_LIMITS 1
#define MIR_PLAN_START_IN_COLLISION 2
#define MIR_PLAN_GOAL_IN_COLLISION 3
#define MIR_PLAN_NODE_LIMIT 4
#define MIR_PLAN_ITERATION_LIMIT 5
#define MIR_PLAN_PATH_TOO_LONG 6
typedef struct MirPlanQuery {
  int32_t  struct_size;     /* = sizeof(MirPlanQuery) */
  int32_t  n_probes;        /* N, 1 .. 1024 */
  int32_t  n_dofs;          /* D, 1 .. 16 */
  int32_t  num_waypoints;   /* W >= 2 */
  int32_t  max_nodes;       /* per tree, >= 2 */
  int32_t  max_iterations;  /* >= 0 */
  int32_t  smooth_passes;   /* >= 0 */
  uint32_t flags;           /* MIR_PLAN_IGNORE_COLLISION; unknown bits are MIR_E_INVALID */
  uint32_t seed;
  float    resolution;      /* > 0: the largest joint step between two checked configurations */
  float    step;            /* > 0: the L2 length of a tree extension */
  float    margin;          /* >= 0 */
  float    max_distance;    /* > margin: the cap of a clearance */
  int32_t  _pad;
  uint64_t skip_geoms;      /* bit g set: geom g is not tested */
} MirPlanQuery;
int mir_plan_query_sizeof(void);
int mir_plan_path(MirHandle h, const MirPlanQuery* q,
                  const float* probes /* (N,4) device */, const int32_t* probe_link /* (N) HOST, nullable */,
                  const int32_t* dof_qadr /* (D) HOST: qpos address of each planned dof; revolute or prismatic only */,
                  const int64_t* env_idx /* device, nullable */, int32_t n_rows,
                  const float* qpos_start /* (R,nq) device, nullable = the current state */, const float* qpos_goal /* (R,D) */,
                  float* path /* (R,W,D) */, int32_t* status /* (R) */, float* poly /* (R,MIR_PLAN_MAX_POLY,D) nullable */,
                  int32_t* n_poly /* (R) nullable */, int32_t* stats /* (R,4) nullable */, void* stream);
int mir_path_clearance(MirHandle h, const MirPlanQuery* q,
                       const float* probes, const int32_t* probe_link, const int32_t* dof_qadr,
                       const int64_t* env_idx, int32_t n_rows, const float* qpos_start,
                       const float* paths /* (R,K,D) */, int32_t K,
                       float* seg_min /* (R,K-1) */, float* row_min /* (R) */, int32_t* row_first_blocked /* (R) */, void* stream);

/* ---- self-collision: the sphere model against itself ----------------------------------------------------
 * Genesis plans with self-collision whenever the scene enables it.  Here the arm is its sphere model (mir_signed_distance), so the self
 * test is sphere against sphere: mir_self_distance answers it at the state or at candidate configurations, and mir_plan_path_self /
 * mir_path_clearance_self are mir_plan_path / mir_path_clearance with the self test added to clear(q).
 * The model.  probes (N + E, 4) and probe_link (N + E), as in mir_signed_distance: the first N probes are the sphere model of the scene
 *   test; the E = n_extra probes behind them take part in the self test ONLY (the spheres of a base bolted to the floor, which sit in
 *   the floor by construction).  N + E <= 1024, else MIR_E_CAPACITY.
 * The pair filter.  link_mask[a] bit b set: the spheres on body a are tested against the spheres on body b.  The mask must be symmetric
 *   with a zero diagonal and name no body at or above nbody (MIR_E_INVALID otherwise).  An all-zero mask is legal: nothing is tested.
 * s(i, j), float32: d = c_i - c_j per component (world centres, the forward kinematics of mir_signed_distance), n2 = fma(d_z, d_z,
 *   fma(d_y, d_y, d_x d_x)), s = sqrt(n2) - (r_i + r_j), the root within an ulp (the hardware's v_sqrt_f32).  s(i, j) and s(j, i) are
 *   the same bits.
 * Per probe i: self_i = the lowest s(i, j) over j = 0 .. N + E - 1 with bit link[j] of link_mask[link[i]] set, j ascending, the lower j on
 *   a tie (a strict < replaces the holder).
 * mir_self_distance.  distance (R, N + E) = self_i and other (R, N + E) = its j when self_i <= max_distance; else max_distance and -1.
 *   row_min (R) = the lowest distance of the row over the probes that have a partner, row_pair (R, 2) = (i, other_i) of the lowest i
 *   that holds it: i < j, the lowest i, then the lowest j.  A row without a partner within max_distance: max_distance and (-1, -1).
 *   A row in which a probe centre is not finite: every distance and row_min are -infinity (blocked, as in the planner), other and
 *   row_pair are -1.  Poses (pose cache or qpos rows), rows, env_idx, clamping, "every output is nullable", "a call changes nothing a
 *   later call can see" and MIR_E_CAPACITY (N + E > 1024; R x (N + E) beyond 2^31 - 1) are those of mir_signed_distance.  self_margin
 *   is checked and otherwise not read.
 * mir_plan_path_self / mir_path_clearance_self.  Every argument of mir_plan_path / mir_path_clearance keeps its meaning; q->n_probes is
 *   N, and probes / probe_link hold N + sq->n_extra entries.  self(q) = min(min_i self_i, sq->max_distance) at the poses of clear(q),
 *   -infinity where clear(q)'s value is -infinity for a configuration or a probe centre (any of the N + E) that is not finite.
 *   clear(q) holds when the scene clearance (the first N probes, the arithmetic of mir_plan_path) is >= margin AND self(q) >=
 *   self_margin; the planner evaluates self(q) only when the scene test holds.  Step 2 of the algorithm becomes: start's scene test
 *   fails: START_IN_COLLISION; its self test fails: START_IN_SELF_COLLISION; then the goal's scene test: GOAL_IN_COLLISION; its self
 *   test: GOAL_IN_SELF_COLLISION (for one configuration the scene test decides first).  Everything else of the algorithm is
 *   unchanged, so with an all-zero mask and n_extra = 0 every output is that of mir_plan_path / mir_path_clearance bit for bit.
 *   mir_path_clearance_self: seg_min / row_min are the scene values as before; seg_self_min (R, K-1) / row_self_min (R) the lowest
 *   self(q) over the same samples; row_first_blocked = the first segment with seg_min < margin or seg_self_min < self_margin, or -1.
 *   All five outputs NULL: MIR_OK without a launch.  MIR_PLAN_IGNORE_COLLISION switches both tests off (the values reported are
 *   q->max_distance and sq->max_distance).
 *   The sphere list lives in LDS behind the trees: the fixed part + 2 max_nodes (4 D + 2) + 16 (N + E) bytes must fit 64 KB, else
 *   MIR_E_CAPACITY.
 * MIR_E_INVALID, besides the refusals of the entry point each one extends: a NULL sq; struct_size != sizeof(MirSelfQuery); n_extra
 * < 0; self_margin < 0 or not finite; max_distance <= self_margin or not finite; an unknown flag bit; a mask that is not symmetric,
 * has a diagonal bit or a bit at or above nbody.  None of them launches anything.
 * Not covered: link geoms other than through spheres.  A carried object against the scene and against the arm is the question of
 * mir_plan_path_carry / mir_path_clearance_carry (below, "carried object").
 * (Added structs and entry points: MIR_VERSION, MirDistQuery, MirPlanQuery and the entry points above stay as they are.) */
#define MIR_PLAN_START_IN_SELF_COLLISION 7
#define MIR_PLAN_GOAL_IN_SELF_COLLISION 8
typedef struct MirSelfQuery {
  int32_t  struct_size;    /* = sizeof(MirSelfQuery) */
  int32_t  n_extra;        /* E >= 0: probes behind the first N, self test only */
  float    self_margin;    /* >= 0 */
  float    max_distance;   /* > self_margin, finite: the cap of a self distance */
  uint32_t flags;          /* 0; unknown bits are MIR_E_INVALID */
  uint32_t link_mask[MIR_MAX_BODY]; /* bit b of word a: body a's spheres against body b's; symmetric, zero diagonal */
} MirSelfQuery;
int mir_self_query_sizeof(void);
int mir_self_distance(MirHandle h, const MirSelfQuery* sq, int32_t n_probes /* N */,
                      const float* probes /* (N+E,4) device */, const int32_t* probe_link /* (N+E) HOST, nullable */,
                      const int64_t* env_idx /* device, nullable */, int32_t n_rows, const float* qpos /* (R,nq) device, nullable */,
                      float* distance /* (R,N+E) */, int32_t* other /* (R,N+E) */, float* row_min /* (R) */,
                      int32_t* row_pair /* (R,2) */, void* stream);
int mir_plan_path_self(MirHandle h, const MirPlanQuery* q, const MirSelfQuery* sq,
                       const float* probes /* (N+E,4) device */, const int32_t* probe_link /* (N+E) HOST, nullable */,
                       const int32_t* dof_qadr, const int64_t* env_idx, int32_t n_rows, const float* qpos_start,
                       const float* qpos_goal, float* path, int32_t* status, float* poly, int32_t* n_poly, int32_t* stats, void* stream);
int mir_path_clearance_self(MirHandle h, const MirPlanQuery* q, const MirSelfQuery* sq,
                            const float* probes, const int32_t* probe_link, const int32_t* dof_qadr,
                            const int64_t* env_idx, int32_t n_rows, const float* qpos_start,
                            const float* paths /* (R,K,D) */, int32_t K,
                            float* seg_min /* (R,K-1) */, float* seg_self_min /* (R,K-1) */, float* row_min /* (R) */,
                            float* row_self_min /* (R) */, int32_t* row_first_blocked /* (R) */, void* stream);

/* ---- carried object: planning and checking with a grasped body attached to the arm -----------------------
 * Genesis's plan_path takes an attached object (`ee_link_name` names the link, `with_entity` the object).  Here the object is a free
 * body of the scene whose pose follows a link of the arm by a rigid transform that is set per row, and whose spheres are probes like
 * the arm's own: mir_plan_path_carry / mir_path_clearance_carry are mir_plan_path(_self) / mir_path_clearance(_self) with one more
 * step in clear(q).  sq is nullable: without it there is no self test, and the call extends mir_plan_path / mir_path_clearance.
 * The attachment.  C = cq->body, a free-joint body without child bodies; Lk = cq->link, any body 0 .. nbody - 1 but C; the grasp
 *   transform G = (p_G, q_G), the pose of C in Lk's frame, one per row, fixed for the call.
 * G, once per row at row set-up.  grasp NULL: from the start row (qpos_start, or the state) after the full forward kinematics,
 *   p_G = qrot(conj(q_L), p_C - p_L), q_G = qmul(conj(q_L), q_C), with (p_L, q_L) and (p_C, q_C) the world poses of Lk and C, q_C the
 *   free-joint quaternion as the forward kinematics normalises it (float32, the qrot and qmul of that forward kinematics).  Otherwise
 *   row k of grasp (R, 7), device: p_G = its xyz, q_G = its wxyz normalised by the routine used for free-joint quaternions (n2 = the
 *   sum of the four squares, times 1 / sqrt(n2) within an ulp).  A row whose G is not finite after this (a NaN or an infinity in the
 *   grasp row or in the poses it is taken from, squares that overflow), or whose grasp quaternion has n2 < 1e-30 (zero: the free-joint
 *   routine would make it the identity), is blocked: every clearance of the row, scene and self, is -infinity, as for a geom pose that
 *   is not finite, and the planner reports START_IN_COLLISION.  grasp_used (R, 7), nullable: the G each row used, xyz then wxyz (the
 *   identity quaternion for a zero one).  G is computed by the kernel: no host read-back.
 * clear(q).  After the forward kinematics of the bodies below a planned dof, C's pose is overwritten: p_C = p_L + qrot(q_L, p_G),
 *   q_C = qmul(q_L, q_G).  Nothing else of clear(q) changes: probes whose probe_link is C ride on that pose; the scene test sees those
 *   among the first N like any probe; with sq they are in the sphere list, and link_mask[C] says which links they are tested against
 *   (symmetric, as for every body).  C's entry in the qpos row is never written, and C's own geoms must be in skip_geoms: C counts as
 *   riding on the planned joints.  Statuses are unchanged: a carried sphere in a geom at the start is START_IN_COLLISION, a carried
 *   sphere in the arm START_IN_SELF_COLLISION.  A call in which no probe rides on C returns, bit for bit, what the entry point it
 *   extends returns.
 * mir_path_clearance_carry: the outputs of mir_path_clearance_self plus grasp_used; seg_self_min and row_self_min must be NULL when sq
 *   is NULL (MIR_E_INVALID).  All six outputs NULL: MIR_OK without a launch.
 * MIR_E_INVALID, besides the refusals of the entry point each one extends: a NULL cq; struct_size != sizeof(MirCarryQuery); an unknown
 * flag bit; C not a free-joint body (outside 1 .. nbody - 1 included) or with a child body; Lk outside 0 .. nbody - 1 or Lk == C; a geom
 * of C that is not in skip_geoms (unless MIR_PLAN_IGNORE_COLLISION).  None of them launches anything.
 * Not covered: mir_signed_distance and mir_self_distance with a carried body (send the two-point trajectory [q, q] through
 * mir_path_clearance_carry); a carried body with geoms that are tested as themselves.
 * (Added struct and entry points: MIR_VERSION and every other struct and entry point stay as they are.) */
typedef struct MirCarryQuery {
  int32_t  struct_size;  /* = sizeof(MirCarryQuery) */
  int32_t  body;         /* C: the carried body, a free-joint body without children */
  int32_t  link;         /* Lk: the link C follows */
  uint32_t flags;        /* 0; unknown bits are MIR_E_INVALID */
} MirCarryQuery;
int mir_carry_query_sizeof(void);
int mir_plan_path_carry(MirHandle h, const MirPlanQuery* q, const MirSelfQuery* sq /* nullable: no self test */, const MirCarryQuery* cq,
                        const float* probes /* (N+E,4) device */, const int32_t* probe_link /* (N+E) HOST, nullable */,
                        const int32_t* dof_qadr, const int64_t* env_idx, int32_t n_rows, const float* qpos_start,
                        const float* grasp /* (R,7) device, nullable: from the start row */, const float* qpos_goal,
                        float* path, int32_t* status, float* poly, int32_t* n_poly, int32_t* stats,
                        float* grasp_used /* (R,7) nullable */, void* stream);
int mir_path_clearance_carry(MirHandle h, const MirPlanQuery* q, const MirSelfQuery* sq /* nullable */, const MirCarryQuery* cq,
                             const float* probes, const int32_t* probe_link, const int32_t* dof_qadr,
                             const int64_t* env_idx, int32_t n_rows, const float* qpos_start,
                             const float* grasp /* (R,7) nullable */, const float* paths /* (R,K,D) */, int32_t K,
                             float* seg_min /* (R,K-1) */, float* seg_self_min /* (R,K-1), NULL without sq */, float* row_min /* (R) */,
                             float* row_self_min /* (R), NULL without sq */, int32_t* row_first_blocked /* (R) */,
                             float* grasp_used /* (R,7) nullable */, void* stream);

/* ---- goal sets: planning to whichever of several goal configurations can be reached ----------------------
 * `robot.plan_path_to_goals(qpos_goals)`: two grasp approaches, the symmetric grasps of a cube, several inverse-kinematics branches of
 * one pose.  mir_plan_path_goals is mir_plan_path_carry with a SET of goals per row: ONE launch judges the goals, tries the direct edge
 * to the valid ones and otherwise plans to whichever the trees meet through, with no host decision in between.  Every argument of
 * mir_plan_path_carry keeps its meaning, but sq AND cq are nullable (neither: the scene test of mir_plan_path; grasp and grasp_used
 * must be NULL without cq), so that this one entry point serves all four forms.
 * Goals.  gq->max_goals = G, 1 .. MIR_PLAN_MAX_GOALS; qpos_goals (R, G, D); n_goals (R) int32, nullable: G for every row.  A row value
 *   outside 0 .. G is clamped; the entries at or beyond the row's count are never read (a NaN there is harmless).
 * Algorithm.  1. The start: its scene test fails: START_IN_COLLISION; with sq, its self test: START_IN_SELF_COLLISION (clear() of the
 *   form the call selects; the goals are then not judged: every goal_status of the row is -1).  2. Each goal g < n_goals[r], g
 *   ascending, gets goal_status[r, g]: a value that is not finite or outside [lo, hi] in a planned dof: GOAL_OUT_OF_LIMITS (nothing
 *   is evaluated for it); its scene test fails (the carried body's spheres among the first N included): GOAL_IN_COLLISION; its self
 *   test: GOAL_IN_SELF_COLLISION; otherwise MIR_PLAN_OK: the goal is valid.  These are the statuses mir_plan_path and its forms give the
 *   same goal.  No valid goal (n_goals[r] = 0 included): the row ends with MIR_PLAN_NO_VALID_GOAL; as for every failed plan the arm
 *   stays put.  3. edge(start, goal_g) is tried for the valid goals in ascending squared L2 distance from the start (summed j ascending
 *   as in `nearest`; the lower g on a tie); the first edge that holds gives the polyline [start, goal_g], iterations = 0.  4. Otherwise
 *   RRT-Connect exactly as step 4 of mir_plan_path, with one change: Tb starts as a FOREST, its first nodes are the valid goals in
 *   ascending g, each without a parent.  nearest, extend, connect, NODE_LIMIT and ITERATION_LIMIT are unchanged (odd iterations extend
 *   the forest from its nearest node, whichever root that hangs on).  5. The extraction walks Tb's parents to whichever root it reaches:
 *   that root is the row's goal, the last node of the polyline and the last waypoint are its bits.  6., 7. Smoothing and resampling
 *   unchanged (the smoothing never removes the last node).  With G = 1 and a valid goal every output is that of mir_plan_path /
 *   _self / _carry bit for bit; the two differ only in the order of the refusals of a row: mir_plan_path looks at the goal's limits
 *   before the start.  max_iterations must stay below 2^30: the counters from 0x40000000 on are kept for goal sampling.
 * Outputs.  path, status, poly, n_poly, stats, grasp_used: those of mir_plan_path_carry; stats[2], the nodes of Tb, counts the roots
 *   from the moment the trees are set up (1 before, as in mir_plan_path).  goal_index (R), nullable: the g the plan ends at, -1 for a
 *   row that fails.  goal_status (R, G), nullable: as above, -1 behind n_goals[r].
 * The trees live in LDS as for mir_plan_path (the same MIR_E_CAPACITY); the goals need no LDS of their own.
 * MIR_E_INVALID, besides the refusals of mir_plan_path_carry with a nullable cq: a NULL gq or qpos_goals; struct_size !=
 * sizeof(MirGoalQuery); an unknown flag bit; max_goals outside 1 .. 8; max_nodes <= max_goals; grasp or grasp_used without cq.  None of
 * them launches anything.
 * Not done (a goal given as a POSE of a link is mir_plan_path_pose, below): goal regions or orientation tolerances about an axis; a ranking of the goals other than by distance from the
 * start; parity with Genesis (OMPL) or MoveIt, which is unpinned as for mir_plan_path.
 * (Added struct, status and entry point: MIR_VERSION and every other struct and entry point stay as they are.) */
#define MIR_PLAN_MAX_GOALS 8
#define MIR_PLAN_NO_VALID_GOAL 9
typedef struct MirGoalQuery {
  int32_t  struct_size;  /* = sizeof(MirGoalQuery) */
  int32_t  max_goals;    /* G: 1 .. MIR_PLAN_MAX_GOALS, < MirPlanQuery.max_nodes */
  uint32_t flags;        /* 0; unknown bits are MIR_E_INVALID */
  int32_t  _pad;
} MirGoalQuery;
int mir_goal_query_sizeof(void);
int mir_plan_path_goals(MirHandle h, const MirPlanQuery* q, const MirSelfQuery* sq /* nullable: no self test */,
                        const MirCarryQuery* cq /* nullable: no carried body */, const MirGoalQuery* gq,
                        const float* probes /* (N+E,4) device */, const int32_t* probe_link /* (N+E) HOST, nullable */,
                        const int32_t* dof_qadr, const int64_t* env_idx, int32_t n_rows, const float* qpos_start,
                        const float* grasp /* (R,7) device, nullable; NULL without cq */, const float* qpos_goals /* (R,G,D) */,
                        const int32_t* n_goals /* (R) device, nullable: G */, float* path, int32_t* status, float* poly, int32_t* n_poly,
                        int32_t* stats, float* grasp_used /* (R,7) nullable; NULL without cq */, int32_t* goal_index /* (R) nullable */,
                        int32_t* goal_status /* (R,G) nullable */, void* stream);

/* ---- pose goals: planning to a pose of a link ---------------------------------------------------------------
 * `robot.plan_path_to_pose(link, pos, quat)`: mir_plan_path_pose is mir_plan_path_goals whose goal set is not read but MADE by the
 * row's wave before the planner starts: inverse-kinematics solutions of the pose, sampled, judged and kept inside the same launch.
 * Every argument of mir_plan_path_goals keeps its meaning but qpos_goals / n_goals, which are outputs here.
 * Chain and options.  gq->link: the body whose pose is asked for; the chain world -> link, its moving joints (the planned dofs on it,
 *   at least one, else MIR_E_INVALID) and opt (damping, pos_tol, rot_tol, max_iters, max_step, respect_joint_limit; NULL: the defaults)
 *   are those of mir_cartesian_path.  target_pos (R, 3); target_quat (R, 4) wxyz, nullable: position only.  A target value that is
 *   not finite or a quaternion with n2 < 1e-30: the row ends with MIR_CART_NOT_FINITE before anything is evaluated.
 * Then the start checks of mir_plan_path_goals.  Then, for s = 0 .. max_samples - 1, until G = max_goals goals are kept:
 *   seed: the start row's chain joints for s = 0; for s > 0 every moving LIMITED joint of the chain is lo + u(env, 0x40000000 | s,
 *   j)(hi - lo), j its planned dof, u the planner's hash: the counters are disjoint from the iterations' (max_iterations < 2^30 is
 *   required) and from 0x80000000 | s of the smoothing.  The iteration of mir_cartesian_path from that seed.  The candidate is the
 *   planner's configuration with the chain's moving joints from the iteration and every other planned dof (the fingers) at its start
 *   value.  It is kept when (a) the iteration converged within pos_tol / rot_tol, (b) every planned dof lies inside its limits, (c)
 *   clear(candidate) holds with the scene, self and carried-object tests of the call, (d) max_j |candidate_j - kept_j| >= dedup for
 *   every goal already kept (dedup = 0 in the query: the planner's resolution).  Sampling does not stop early once an edge would hold.
 * The kept goals are Tb's first nodes, in the order kept; steps 3 - 7 of mir_plan_path_goals follow.  None kept: MIR_PLAN_NO_VALID_GOAL.
 * Outputs.  Those of mir_plan_path_goals (goal_status: MIR_PLAN_OK for the kept goals, -1 behind them), plus, all nullable: goals
 *   (R, G, D) the kept configurations, zeros behind them; n_goals (R); goal_stats (R, 4) int32: samples tried, samples converged,
 *   converged but rejected by (b) or (c), IK iterations in total.  converged = 0 tells "unreachable" from "every solution collides".
 * MIR_E_INVALID, besides the refusals of mir_plan_path_goals: a NULL gq or target_pos; struct_size; an unknown flag bit; max_samples
 * outside 1 .. 2^30 - 1; dedup negative or not finite; max_iterations >= 2^30; the refusals of the chain and of opt as in
 * mir_cartesian_path.  None of them launches anything.
 * Not done: goal regions or orientation tolerances about an axis; one link; no ranking of the goals other than by distance from the
 * start; sampling does not stop early; parity with Genesis / MoveIt is unpinned. */
typedef struct MirPoseGoalQuery {
  int32_t  struct_size;  /* = sizeof(MirPoseGoalQuery) */
  int32_t  link;         /* the body whose pose is the goal */
  int32_t  max_goals;    /* G: 1 .. MIR_PLAN_MAX_GOALS, < MirPlanQuery.max_nodes */
  int32_t  max_samples;  /* >= 1 */
  uint32_t flags;        /* 0 */
  float    dedup;        /* >= 0; 0: MirPlanQuery.resolution */
} MirPoseGoalQuery;
struct MirIkOptions; /* (defined below, "batched inverse kinematics") */
int mir_pose_goal_query_sizeof(void);
int mir_plan_path_pose(MirHandle h, const MirPlanQuery* q, const MirSelfQuery* sq /* nullable */, const MirCarryQuery* cq /* nullable */,
                       const MirPoseGoalQuery* gq, const float* probes, const int32_t* probe_link, const int32_t* dof_qadr,
                       const int64_t* env_idx, int32_t n_rows, const float* qpos_start, const float* grasp /* nullable */,
                       const float* target_pos /* (R,3) */, const float* target_quat /* (R,4) nullable */,
                       const struct MirIkOptions* opt /* nullable */, float* path, int32_t* status, float* poly, int32_t* n_poly, int32_t* stats,
                       float* grasp_used, int32_t* goal_index /* (R) */, int32_t* goal_status /* (R,G) */, float* goals /* (R,G,D) */,
                       int32_t* n_goals /* (R) */, int32_t* goal_stats /* (R,4) */, void* stream);

/* ---- time parameterisation: a joint path as targets at a chosen sample period, within velocity, acceleration and torque limits ----
 * mir_plan_path ends at geometry: W waypoints at equal arc length.  mir_retime_path says how long such a path takes and turns it into
 * targets: time-optimal path parameterisation by reachability analysis (TOPP-RA; Pham & Pham 2018) with the interpolation collocation
 * scheme on the caller's waypoints, R rows in one launch, one wave64 per row (mir_retime.hip).  Per row:
 * Inputs.  A path P (K, D), K >= 2, D <= 16; vmax[D], amax[D] (the query: shared by the rows); max_path_speed in waypoints per second;
 *   E >= 0 extra rows per waypoint ea, eb, elo, ehi (R, K, E) on the device, 2 (D + E) <= 64; a sample period dt and a capacity T.
 * 1. Compaction.  Waypoint k is dropped when all D values compare equal to the last kept waypoint (a failed mir_plan_path row holds
 *   its start W times); the kept ones are Q_0 .. Q_{M-1}, and extra rows of dropped waypoints are ignored.  In this order: a value of
 *   the row's path (anywhere) or of its extra rows at a kept waypoint that is not finite: NOT_FINITE.  M = 1: NO_MOTION (duration 0,
 *   one sample; no error).  M = 2: TOO_FEW_WAYPOINTS (a constant path acceleration per interval cannot go rest to rest over one
 *   interval).  An extra row at a kept waypoint without lo < 0 < hi: INFEASIBLE (rest must be strictly feasible).
 * 2. Geometry, path parameter s = waypoint index.  d_i = Q_{i+1} - Q_i; c_0 = c_{M-1} = 0, m_0 = d_0, m_{M-1} = d_{M-2}; inside,
 *   c_i = d_i - d_{i-1} and m_i = (d_i + d_{i-1}) / 2.
 * 3. Speed cap, x = (ds/dt)^2.  cap_i = min(max_path_speed^2, (vmax_j / |d_ej|)^2) over the adjacent intervals e in {i-1, i} and the
 *   dofs j with d_ej != 0.  Positions are piecewise linear in s (9.) and x is linear in s within an interval, so the velocity limit
 *   holds at every instant, not only at the waypoints.
 * 4. Rows at gridpoint i, lo <= alpha u + beta x <= hi with u = d2s/dt2: D acceleration rows (m_ij, c_ij, -amax_j, amax_j), then the
 *   E extra rows as given.
 * 5. Interval i: (x, u) satisfies the rows of gridpoint i at (x, u), those of gridpoint i+1 at (x + 2u, u) -- the row
 *   (alpha' + 2 beta', beta', lo', hi') in (u, x) -- and 0 <= x + 2u <= Kmax_{i+1}.
 * 6. Backward.  Kmax_{M-1} = 0; for i = M-2 .. 1, Kmax_i = the largest x in [0, cap_i] for which a u exists under 5.; Kmax_0 = 0.
 * 7. Forward.  x_0 = 0; u_i = the largest u the rows of 5. allow at x_i with x_i + 2u <= Kmax_{i+1}, raised to -x_i / 2 if rounding
 *   put it below; x_{i+1} = max(x_i + 2 u_i, 0), x_{M-1} = 0.
 * 8. Times.  t_0 = 0, t_{i+1} = t_i + 2 / (sqrt x_i + sqrt x_{i+1}); a zero denominator: INFEASIBLE.  duration = t_{M-1}.
 * 9. Samples.  n_samples = ceil(duration / dt) + 1 (at most 2 000 000 001); sample n at tau = n dt.  Sample 0 carries the bits of P_0;
 *   a sample with tau >= duration the bits of P_{K-1} and velocity 0; else, in the interval t_i <= tau < t_{i+1}, with
 *   delta = tau - t_i and u_i = (x_{i+1} - x_i) / 2: f = clamp(sqrt(x_i) delta + u_i delta^2 / 2, 0, 1), q = Q_i + f d_i,
 *   velocity = d_i (sqrt(x_i) + u_i delta).  All T samples of a row are written.  With a sample array given and n_samples > T the row is
 *   TRUNCATED: x, t and duration stay valid and the first T samples are written.  A row with another failure status writes P_0 to
 *   every sample, zeros to x and t, duration 0 and n_samples 1: following it keeps the arm where it is.
 * The LPs of 6. and 7. have two variables and at most 66 constraints: a lane holds one row (the lower D + E lanes the left collocation,
 *   the upper D + E the right one) as bounds on u that are linear in x; 6. is a bisection on x with 32 halvings (a wave minimum and a
 *   wave maximum each), 7. one wave minimum.  A row with alpha == 0 bounds x alone.  Every loop is bounded by K, T or a constant.
 * Outputs use the caller's indexing: x, t (R, K), a dropped waypoint repeats the values of the waypoint kept before it; duration (R);
 *   status (R): MIR_RETIME_*; n_samples (R); samples, sample_vel (R, T, D), each nullable.  K <= MIR_RETIME_MAX_WAYPOINTS: the row's
 *   Kmax, x and t live in LDS.  The call reads no state and changes nothing a later call can see; n_rows = 0 returns MIR_OK.
 * MIR_E_INVALID: a NULL handle, query, paths or x / t / duration / status / n_samples; struct_size != sizeof(MirRetimeQuery); K < 2,
 *   D outside 1 .. 16, E < 0, E > 0 with a NULL extra array, n_rows < 0, num_samples < 0; an unknown flag bit; a vmax, amax, dt or
 *   max_path_speed that is not finite and > 0; samples or sample_vel with num_samples < 1; a call while a mir_step_begin is open.
 *   MIR_E_CAPACITY: 2 (D + E) > 64; K > MIR_RETIME_MAX_WAYPOINTS; R x T x D beyond 2^31 - 1.  None of them launches anything, and
 *   mir_last_error() names the entry point.
 * What it does not do.  The acceleration and torque limits are collocated: they bound the path acceleration averaged over each
 *   waypoint-to-waypoint traversal, as in TOPP-RA and MoveIt's parameterisers.  The samples stay exactly on the polyline that was
 *   collision-checked, so a dof's velocity changes at a kink within one sample: the finite difference of the samples keeps vmax, their
 *   second difference can exceed amax many times over at a kink (finer waypoints shrink that).  No blending of corners, no jerk limit,
 *   no start or end speed other than rest, no contact forces in the torque rows (those are the caller's extra rows).
 * (Added struct and entry point: MIR_VERSION and every other struct and entry point stay as they are.) */
#define MIR_RETIME_MAX_WAYPOINTS 2048
#define MIR_RETIME_OK 0
#define MIR_RETIME_NO_MOTION 1
#define MIR_RETIME_TOO_FEW_WAYPOINTS 2
#define MIR_RETIME_NOT_FINITE 3
#define MIR_RETIME_INFEASIBLE 4
#define MIR_RETIME_TRUNCATED 5
typedef struct MirRetimeQuery {
  int32_t  struct_size;    /* = sizeof(MirRetimeQuery) */
  int32_t  n_dofs;         /* D: 1 .. 16 */
  int32_t  n_extra;        /* E >= 0 extra rows per waypoint, 2 (D + E) <= 64 */
  int32_t  num_waypoints;  /* K: 2 .. MIR_RETIME_MAX_WAYPOINTS */
  int32_t  num_samples;    /* T >= 0: the capacity of samples / sample_vel per row */
  uint32_t flags;          /* 0; unknown bits are MIR_E_INVALID */
  float    dt;             /* the sample period, s */
  float    max_path_speed; /* waypoints per second */
  float    vmax[16];       /* per dof, finite and > 0 (the first D are read) */
  float    amax[16];
} MirRetimeQuery;
int mir_retime_query_sizeof(void);
int mir_retime_path(MirHandle h, const MirRetimeQuery* q, int n_rows, const float* paths /* (R,K,D) device */,
                    const float* ea, const float* eb, const float* elo, const float* ehi /* (R,K,E) device, NULL when E == 0 */,
                    float* x /* (R,K) */, float* t /* (R,K) */, float* duration /* (R) */, int32_t* status /* (R) */,
                    int32_t* n_samples /* (R) */, float* samples /* (R,T,D) nullable */, float* sample_vel /* (R,T,D) nullable */,
                    void* stream);

/* ---- Cartesian paths: a link follows a straight-line polyline, collision-checked, in one launch -------------
 * `robot.plan_cartesian_path(link, pos, quat)`: the approach, the lift and the place of a grasp, where the hand itself must follow a
 * line (MoveIt: computeCartesianPath(eef_step, jump_threshold) -> fraction).  For R rows ONE launch (mir_cart.hip, one wave64 per row)
 * takes each row's link along K straight segments: inverse kinematics at every sample, seeded with the sample before, a joint-jump
 * test and the planner's edge check between consecutive samples.  It reads the state (or the start rows) and the compiled model and
 * writes only its outputs.  Parity with Genesis and MoveIt is unpinned: the rule is this library's own, fixed here to the operand.
 * Arguments.  pq supplies the clearance side exactly as for mir_path_clearance (n_probes, n_dofs, resolution, margin, max_distance,
 *   flags, skip_geoms; its planner fields are ignored); sq and cq, both nullable, mean what they mean in mir_plan_path_self and
 *   mir_plan_path_carry (the grasp transform is taken from the start row).  probes, probe_link, dof_qadr (D <= 16), env_idx, n_rows,
 *   clamping and qpos_start are those of mir_plan_path.  opt: the options of mir_inverse_kinematics (NULL: its defaults; pos_tol and
 *   rot_tol must be > 0).  target_pos (R, K, 3); target_quat (R, K, 4) wxyz or NULL: the link keeps no orientation target and the
 *   rotation part of the IK error is dropped.
 * Per row:
 * 1. Set-up.  a0 = the planned dofs of the start row.  The chain world -> link_body is that of mir_inverse_kinematics (fixed bodies
 *   folded, <= 16 elements).  A joint MOVES when it is a scalar joint on the chain and a planned dof; every other entry keeps its
 *   start bits.  X_0 = (p_0, q_0), the link's pose at a0 by the chain's forward kinematics.  p_k = target_pos[k - 1]; q_k =
 *   target_quat[k - 1] normalised by the routine used for free-joint quaternions (k = 1 .. K).
 * 2. NOT_FINITE: a NaN or an infinity in any target of the row, or a target quaternion whose four squares sum to less than 1e-30 or
 *   to no finite float32.
 * 3. Sample counts.  dp_k = sqrt(dx^2 + dy^2 + dz^2) of p_k - p_{k-1}.  d_k = conj(q_{k-1}) q_k, negated when d_k.w < 0 (the shorter
 *   arc; the antipodal case d_k.w == 0 is NOT negated: the half turn about +d_k.xyz); sn_k = |d_k.xyz|, ang_k = 2 atan2(sn_k, d_k.w)
 *   (0 without target_quat).  n_k = max(1, ceil(max(dp_k / max_pos_step, ang_k / max_rot_step))), at most 2^30 (a quotient that is
 *   not finite counts as 2^30).  Every quotient here and below is the planner's: a float32 division refined by one Newton step.
 *   S = sum n_k.  S + 1 > max_points: TOO_MANY_POINTS.
 * 4. Start.  clear(a0) of mir_plan_path: its scene test fails: MIR_PLAN_START_IN_COLLISION; with sq, its self test fails:
 *   MIR_PLAN_START_IN_SELF_COLLISION.  In 2. - 4. nothing moves: n_points = 1, fraction = 0.
 * 5. Samples, in order: segment k = 1 .. K, i = 1 .. n_k, from the last accepted configuration c (a0 at first).
 *   Target.  i == n_k: (p_k, q_k) themselves.  Else t = i / n_k, p = p_{k-1} + t (p_k - p_{k-1}), q = q_{k-1} (cos h, sin h d_k.xyz /
 *     sn_k) with h = t ang_k / 2; sn_k <= 1e-9 (the zero-angle case): q = q_{k-1}.
 *   IK.  The iteration of mir_inverse_kinematics (below) word for word -- accept / reject / stall, the lambda^2 schedule (from
 *     damping^2 at every sample), the max_step scaling, the limit clamp, max_iters -- on the moving joints, seeded with c.  Its result
 *     q_acc gives the candidate c' (the moving joints from q_acc, the other planned dofs from a0).  |e_pos| < pos_tol and |e_rot| <
 *     rot_tol do not both hold at q_acc: IK_FAILED.
 *   Jump.  max_j |c'_j - c_j| > jump_threshold over the planned dofs: JOINT_JUMP.
 *   Collision.  edge(c, c') of mir_plan_path: its samples in order, each by the scene test and then, with sq and only when the scene
 *     test holds, the self test.  The first test that fails decides: the scene test: BLOCKED; the self test: BLOCKED_SELF (the tie
 *     rule: within one configuration the scene test is asked first, so a configuration that fails both is BLOCKED).
 *   The first failure ends the row, which keeps what it achieved; otherwise c' is accepted: point a = the count of accepted samples.
 * 6. Outputs.  points (R, P, D): points[0] = a0's bits, points[a] = accepted sample a, and every point behind n_points = a + 1 repeats
 *   the last accepted one (what mir_retime_path compacts and mir_path_clearance accepts).  fraction = a / S (float32, refined).
 *   status (R): MIR_PLAN_OK, the two start statuses or MIR_CART_*.  path (R, W, D), with num_waypoints = W >= 2: waypoint 0 = the bits
 *   of points[0], waypoint W - 1 those of points[n_points - 1]; else u = (w / (W - 1)) (n_points - 1), i0 = min(floor(u), n_points -
 *   2), t = u - i0, waypoint = points[i0] + t (points[i0 + 1] - points[i0]); n_points == 1: the start W times.  stats (R, 4): IK
 *   iterations summed over the samples, configurations checked for clearance, S (saturated at 2^31 - 1), the segment (0-based) whose
 *   sample failed or -1.
 * Every loop is bounded by K, P, W, max_iters or the 4096 samples of the edge rule; no input can keep a wave running.
 * MIR_E_INVALID: a NULL handle, q, pq, probes, dof_qadr, target_pos, points, n_points, fraction or status; struct_size != sizeof of
 *   any query given; K < 1, P < 2, W < 0 or W == 1, W >= 2 without path or path with W == 0; an unknown flag bit; a step or the
 *   threshold not finite or <= 0; bad IK options; a link out of range or that hangs off a free body; no moving joint; everything
 *   mir_path_clearance (and the _self / _carry forms, when sq / cq are given) refuses.  MIR_E_CAPACITY: R x max(P, W) x D beyond
 *   2^31 - 1; a chain of more than 16 elements.  None of them launches anything; n_rows == 0 returns MIR_OK without a launch.
 * What it does not do.  No escape from a blocked line (that is mir_plan_path's job); no null-space objective or redundancy resolution
 *   beyond the damped least-squares step; one link, no axis masks; clearance between two samples is as coarse as the edge rule.
 * (Added struct and entry point: MIR_VERSION and every other struct and entry point stay as they are.) */
#define MIR_CART_TOO_MANY_POINTS 16
#define MIR_CART_NOT_FINITE 17
#define MIR_CART_IK_FAILED 18
#define MIR_CART_JOINT_JUMP 19
#define MIR_CART_BLOCKED 20
#define MIR_CART_BLOCKED_SELF 21
typedef struct MirCartQuery {
  int32_t  struct_size;    /* = sizeof(MirCartQuery) */
  int32_t  link_body;      /* the link that follows the line */
  int32_t  num_targets;    /* K >= 1 */
  int32_t  max_points;     /* P >= 2: the capacity of points per row */
  int32_t  num_waypoints;  /* W: 0, or >= 2 with path */
  uint32_t flags;          /* 0; unknown bits are MIR_E_INVALID */
  float    max_pos_step;   /* > 0, metres between two samples */
  float    max_rot_step;   /* > 0, radians between two samples */
  float    jump_threshold; /* > 0, radians or metres per sample and joint */
} MirCartQuery;
int mir_cart_query_sizeof(void);
struct MirIkOptions; /* (defined below, "batched inverse kinematics") */
int mir_cartesian_path(MirHandle h, const MirCartQuery* q, const MirPlanQuery* pq, const MirSelfQuery* sq /* nullable */,
                       const MirCarryQuery* cq /* nullable */, const float* probes, const int32_t* probe_link, const int32_t* dof_qadr,
                       const int64_t* env_idx, int32_t n_rows, const float* qpos_start /* (R,nq) nullable */,
                       const float* target_pos /* (R,K,3) */, const float* target_quat /* (R,K,4) wxyz, nullable */,
                       const struct MirIkOptions* opt /* nullable: the IK defaults */, float* points /* (R,P,D) */, int32_t* n_points /* (R) */,
                       float* fraction /* (R) */, int32_t* status /* (R) */, float* path /* (R,W,D) nullable */,
                       int32_t* stats /* (R,4) nullable */, void* stream);

/* ---- corner blending: the corners of a joint-space polyline rounded, collision-checked, in one launch -------------
 * `robot.blend_path(poly)`: mir_plan_path and mir_cartesian_path turn their corners at a point, and mir_retime_path keeps the
 * acceleration limit only on average there (above, "What it does not do").  For R rows ONE launch (mir_blend.hip, one wave64 per row)
 * replaces each interior corner of a row's polyline by a quadratic Bezier blend within a stated deviation from the corner, checks the
 * blend with the planner's clear(q), halves a blocked blend and returns the smoothed path dense enough for mir_retime_path.  It reads
 * the state (or the start rows) and the compiled model and writes only its outputs.  The rule is this library's own.
 * Arguments.  pq supplies the clearance side exactly as for mir_path_clearance (n_probes, n_dofs, resolution, margin, max_distance,
 *   flags, skip_geoms; its planner fields are ignored); sq, cq, probes, probe_link, dof_qadr (D <= 16), env_idx, n_rows and qpos_start
 *   are those of mir_cartesian_path (the grasp transform is taken from the start row).  poly (R, K, D): row k's polyline (row k, not env
 *   env_idx[k]), 2 <= K = num_nodes <= MIR_PLAN_MAX_POLY; n_poly (R), nullable: the count of valid leading nodes as mir_plan_path
 *   writes it, clamped to 1 .. K (NULL: K); nodes behind it are not read.  delta = max_deviation, m = blend_points, s = max_shrinks,
 *   P = max_points, W = num_waypoints.  Every quotient below is the planner's: a float32 division refined by one Newton step; every
 *   sum over the dofs runs j ascending.
 * Per row:
 * 1. Compaction, as mir_retime_path: node k is dropped when all D values compare equal to the last kept node; the kept ones are
 *   Q_0 .. Q_{M-1}.  In this order: a value of a valid node that is not finite: NOT_FINITE.  M = 1: NO_MOTION (no error: the start
 *   repeated, what a failed mir_plan_path row holds).  2 + (M - 2)(m + 1) > P: TOO_MANY_POINTS -- decided from the worst case before
 *   anything is evaluated, so it does not depend on collisions.
 * 2. Start.  clear(Q_0) of mir_plan_path: its scene test fails: MIR_PLAN_START_IN_COLLISION; with sq, its self test fails:
 *   MIR_PLAN_START_IN_SELF_COLLISION.
 * 3. Segments.  d_i = Q_{i+1} - Q_i, L_i = sqrt(sum_j d_ij^2), u_ij = d_ij / L_i (u_i = 0 when L_i underflowed to 0).
 * 4. Half-length of the blend at interior node i = 1 .. M - 2: h_i = min(L_{i-1}, L_i) / 2, so neighbouring blends never overlap; with
 *   du = sqrt(sum_j (u_ij - u_{i-1,j})^2) > 0 also h_i <= 4 delta / du: the curve passes its corner at the distance h du / 4, at its
 *   midpoint, and no point of it lies further than that from the input polyline.  du = 0 (collinear) keeps h_i = min / 2: the blend
 *   lies on the segments.
 * 5. Blend.  A = Q_i - h u_{i-1}, C = Q_i + h u_i, B(t) = (1 - t)^2 A + 2 t (1 - t) Q_i + t^2 C, evaluated by de Casteljau per dof:
 *   p = A + t (Q_i - A), r = Q_i + t (C - Q_i), B = p + t (r - p); B(0) carries A's bits and B(1) C's.  A dof that does not move on
 *   either segment keeps its bits through every step.
 * 6. Check.  n_c = max(1, ceil(2 max_j max(|Q_ij - A_j|, |C_j - Q_ij|) / resolution)), at most 4096 (a quotient that is not finite
 *   counts as 4096); clear(B(k / n_c)) for k = 0 .. n_c in order, the first blocked one ends the check.  |dB_j/dt| <= 2 max(|Q_ij -
 *   A_j|, |C_j - Q_ij|), so consecutive samples differ by at most `resolution` per joint: the promise of the planner's edge rule.
 *   clear is the planner's: the scene test, then (sq) the self test, both with the carried body (cq).
 * 7. Shrinking.  A blocked blend halves h and is checked again, at most s times (s + 1 checks); still blocked, h = 0: the corner
 *   stays sharp and is counted.  h = 0 from 4. (an L that underflowed) is sharp without a check.  MIR_PLAN_IGNORE_COLLISION skips 2.
 *   and every check.  The straight remainders of the input's segments are the caller's and are NOT evaluated: the input polyline
 *   was checked by whoever made it, and mir_path_clearance answers for the dense points.
 * 8. Dense points, in order: Q_0; per interior node B(k / m) for k = 0 .. m of the accepted h (k = 0: A's bits, k = m: C's), or Q_i
 *   itself at h = 0; Q_{M-1}.  A point whose D bit patterns equal the point before is not emitted (two full-length blends meet
 *   mid-segment).  points (R, P, D) holds them, the last one repeated behind n_points (the layout of mir_cartesian_path: what
 *   mir_retime_path compacts and mir_path_clearance accepts).  Every point is a convex combination of input nodes (up to rounding), so
 *   the joint limits the input kept need no new check.
 * 9. Waypoints, W >= 2: path (R, W, D) = the n_points dense points resampled at equal arc length by step 7 of mir_plan_path, the first
 *   and the last carrying the bits of Q_0 and Q_{M-1}.
 * Outputs.  status (R): MIR_PLAN_OK, the two start statuses or MIR_BLEND_*; n_points (R); blend_len (R, MIR_PLAN_MAX_POLY), nullable: the
 *   accepted h at each INPUT node, 0 where there is none (the ends, a dropped node, a sharp corner); stats (R, 4), nullable: M, corners
 *   blended, corners left sharp, configurations checked.  A row with another status than OK returns its first node everywhere
 *   (n_points = 1, blend_len 0): following it keeps the arm still.
 * Every loop is bounded by K, m, s, the 4096 samples of a check, P or W; no input can keep a wave running.
 * MIR_E_INVALID: a NULL handle, q, pq, probes, dof_qadr, poly, points, n_points or status; struct_size != sizeof of any query given;
 *   K < 2; m outside 2 .. 64; s < 0; P < 2; W < 0 or W == 1, W >= 2 without path or path with W == 0; an unknown flag bit; delta not
 *   finite or <= 0; everything mir_path_clearance (and the _self / _carry forms, when sq / cq are given) refuses.  MIR_E_CAPACITY:
 *   K > MIR_PLAN_MAX_POLY; R x max(P, W) x D beyond 2^31 - 1.  None of them launches anything, mir_last_error() names the entry point,
 *   and n_rows == 0 returns MIR_OK without a launch.
 * What it does not do.  A reversal (u_i = -u_{i-1}) is still a stop: its blend lies on the segment.  No jerk limit: the curvature
 *   jumps where a blend meets a straight remainder.  Straight remainders are not re-checked (7.).  A blocked blend is only shrunk
 *   about its corner, never moved to the other side.
 * (Added struct and entry point: MIR_VERSION and every other struct and entry point stay as they are.) */
#define MIR_BLEND_NO_MOTION 32
#define MIR_BLEND_NOT_FINITE 33
#define MIR_BLEND_TOO_MANY_POINTS 34
#define MIR_BLEND_MAX_POINTS_PER_CORNER 64
#define MIR_BLEND_MAX_CHECK 4096
typedef struct MirBlendQuery {
  int32_t  struct_size;    /* = sizeof(MirBlendQuery) */
  int32_t  num_nodes;      /* K: 2 .. MIR_PLAN_MAX_POLY */
  int32_t  blend_points;   /* m: 2 .. 64 chords per blend */
  int32_t  max_shrinks;    /* s >= 0 halvings of a blocked blend */
  int32_t  max_points;     /* P >= 2: the capacity of points per row */
  int32_t  num_waypoints;  /* W: 0, or >= 2 with path */
  uint32_t flags;          /* 0; unknown bits are MIR_E_INVALID */
  float    max_deviation;  /* delta > 0: L2 over the planned dofs */
} MirBlendQuery;
int mir_blend_query_sizeof(void);
int mir_blend_path(MirHandle h, const MirBlendQuery* q, const MirPlanQuery* pq, const MirSelfQuery* sq /* nullable */,
                   const MirCarryQuery* cq /* nullable */, const float* probes, const int32_t* probe_link, const int32_t* dof_qadr,
                   const int64_t* env_idx, int32_t n_rows, const float* qpos_start /* (R,nq) nullable */,
                   const float* poly /* (R,K,D) */, const int32_t* n_poly /* (R) nullable */, float* points /* (R,P,D) */,
                   int32_t* n_points /* (R) */, int32_t* status /* (R) */, float* path /* (R,W,D) nullable */,
                   float* blend_len /* (R,MIR_PLAN_MAX_POLY) nullable */, int32_t* stats /* (R,4) nullable */, void* stream);

/* ---- certified clearance: the continuous minimum clearance of a joint path bracketed, in one launch ----------------
 * `robot.certify_path(path)`: every collision answer above between two configurations is a sampled one (the edge rule evaluates
 * configurations at most `resolution` apart per joint and leaves what lies between them unjudged).  For R rows ONE launch
 * (mir_cert.hip, one wave64 per row) gives, per segment of a row's path, a lower and an upper bound of the minimum over the WHOLE
 * segment of the sphere model's clearance against the tested geoms.  It reads the state (or the start rows) and the compiled model
 * and writes only its outputs.  The rule is this library's own.
 * Why it holds.  The signed distance to a static scene is 1-Lipschitz in a sphere's centre (the planner's front end refuses tested
 *   geoms that ride on planned joints, so the scene is static).  Along q(t) = a + t dq, t in [0, 1], the centre of probe i moves no
 *   faster than v_i = sum_j |dq_j| rho_ij, where for a revolute dof j rho_ij is a bound on the distance between joint j's anchor and
 *   the centre -- the length of the kinematic chain between them, which does not depend on the configuration -- and for a prismatic
 *   dof the length of its axis.  So d_i(t) >= d_i(tm) - |t - tm| v_i: ONE evaluation at the midpoint of an interval bounds the
 *   clearance on all of it, and bisecting where that bound does not decide yields a guaranteed lower bound.
 * Arguments.  pq supplies n_probes, n_dofs, margin, max_distance, flags and skip_geoms exactly as for mir_path_clearance (the rest is
 *   checked as ever and not read); probes, probe_link, dof_qadr (D <= 16), env_idx, n_rows, qpos_start are those of
 *   mir_path_clearance.  paths (R, K, D): row k's path (row k, not env env_idx[k]), K = num_points >= 2.  Segment s runs from a = P_s
 *   to b = P_{s+1}, dq = b - a (float32).
 * Per row and segment:
 * 1. Chain lengths, rebuilt per segment, parent before child: S[0] = 0, S[b] = S[parent] + |pos_b| + pris_b, where pris_b = max(|a_k|,
 *   |b_k|) |axis_b| for a planned prismatic joint (k its dof), |q_b| |axis_b| of the row for an unplanned one, 0 for a revolute or
 *   fixed body.  A body whose parent is the world, and a free body, start a chain: S = 0.  The joint anchor is the body's origin
 *   (MirBodySpec has no joint offset).
 * 2. Speed bound of probe i on link L with local centre c_i: v_i = ((S[L] + |c_i|) A_L - B_L + P_L) 1.0001, never below 0, from
 *   three sums over the planned dofs j on L's path to the world (up to the start of its chain), formed parent before child like S:
 *   A = sum over the revolute ones of |dq_j|, B = sum over the revolute ones of |dq_j| S[body_j], P = sum over the prismatic ones of
 *   |dq_j| |axis_j|.  That is sum_j |dq_j| rho_ij with rho_ij = S[L] - S[body_j] + |c_i| (revolute) or |axis_j| (prismatic); the
 *   factor 1.0001 keeps float32 rounding from making it too low.  Probes on the world, or below no planned dof, have v_i = 0.  Every
 *   product is rounded on its own (no fused multiply-add).
 * 3. Endpoints.  P_0 for segment 0 only, and P_{s+1} for every segment, are evaluated like clear(q) of mir_plan_path: u = min_i d_i
 *   with d_i the capped (distance - radius) of probe i; upper_s = min(upper_s, u).  Without MIR_CERT_BRACKET an endpoint with u <
 *   margin ends the segment as BLOCKED, with lower_s = u - guard.
 * 4. Bisection, stackless, depth first, left child first, from (l, k) = (0, 0).  Node (l, k) covers [k 2^-l, (k + 1) 2^-l]; its
 *   midpoint tm = (2k + 1) 2^-(l+1) and half-width hw = 2^-(l+1) are exact in float32.  d_i at fmaf(tm, dq, a); u = min_i d_i; lo =
 *   min_i (d_i - hw v_i) - guard; upper_s = min(upper_s, u).  Without BRACKET and u < margin: lower_s = min(lower_s, lo), BLOCKED, the
 *   segment ends.  The node is a LEAF when (not BRACKET and lo >= margin) or lo >= upper_s - tol; at l == max_depth it is a leaf
 *   regardless, and if neither test held it marks the segment DEPTH.  A leaf does lower_s = min(lower_s, lo); then, while k is odd,
 *   k >>= 1 and l--; the segment is done at l == 0; otherwise k++.  A node that is no leaf does l++, k *= 2.
 * 5. Budget (takes precedence over 3. and 4.): before EVERY evaluation the row's count is compared with max_evaluations; when it is
 *   spent, this segment and every later one are BUDGET with lower = -INFINITY; upper keeps what was sampled (+INFINITY: nothing).
 * 6. Not finite.  A segment one of whose waypoints (or whose dq) is not finite is NOT_FINITE with lower = -INFINITY and nothing is
 *   evaluated for it; so is a segment at one of whose evaluations a probe centre is not finite, which ends there.  A row whose tested
 *   geom poses are not finite has every segment NOT_FINITE.
 * 7. Status, in this order: NOT_FINITE (6.); BUDGET (5.); BLOCKED: upper < margin (with BRACKET judged here, at the end); DEPTH;
 *   CLEAR: lower >= margin; else UNDECIDED (the bracket is within tol).  row_status: the highest code of the row's segments;
 *   row_first: the first segment that is not CLEAR, -1: none; row_lower, row_upper: the minima over the segments.
 * 8. MIR_PLAN_IGNORE_COLLISION in pq: every segment is CLEAR with lower = upper = max_distance, nothing is evaluated.
 * What the outputs mean.  For a segment that ends CLEAR or UNDECIDED, the continuous minimum over the segment of the sphere model's
 *   clearance against the tested geoms (capped at max_distance) lies in [lower, upper], up to the float32 error of one clearance
 *   evaluation, which `guard` is there to cover; and lower >= margin or upper - lower <= tol.  BLOCKED is a witness: one configuration
 *   below the margin.  A DEPTH segment's lower is still a bound, only a wider one.
 * Outputs, each nullable: seg_lower, seg_upper (R, K-1); seg_status (R, K-1); row_lower, row_upper, row_status, row_first (R); leaves
 *   (R, max_leaves, 3): segment, level and index of the accepted leaves in the order they were accepted -- leaves beyond the capacity
 *   are counted, not stored, and entries behind the count are not written; stats (R, 4): evaluations, leaves, deepest level, segments
 *   whose bisection ran to its end.
 * Every loop is bounded by K, the tree depth, max_depth or max_evaluations; no input can keep a wave running.
 * MIR_E_INVALID: a NULL handle, q, pq, probes, dof_qadr or paths; struct_size != sizeof of a query; K < 2; max_depth outside 0 .. 20;
 *   max_evaluations < 1; max_leaves < 0; leaves NULL while max_leaves > 0; an unknown flag bit; tol not finite; guard not finite or
 *   negative; tol <= guard (the bracket could never close); a step is pending; everything mir_path_clearance refuses.  None of them
 *   launches anything, mir_last_error() names the entry point; n_rows == 0, or every output NULL, returns MIR_OK without a launch.
 * What it does not do.  The arm against itself and a carried object need a bound on RELATIVE motion: that is mir_certify_path_self /
 *   _carry below, not this entry point.  mir_plan_path does not use this rule for its own edges.  The chain bound is loose for
 *   distal spheres when only proximal joints move (the chain is taken at full stretch).
 * (Added struct and entry point: MIR_VERSION and every other struct and entry point stay as they are.) */
#define MIR_CERT_BRACKET 1u /* MirCertQuery.flags: bracket the minimum to tol everywhere instead of stopping at "clear of the margin" */
#define MIR_CERT_MAX_DEPTH 20
#define MIR_CERT_CLEAR 0
#define MIR_CERT_UNDECIDED 1
#define MIR_CERT_DEPTH 2
#define MIR_CERT_BUDGET 3
#define MIR_CERT_BLOCKED 4
#define MIR_CERT_NOT_FINITE 5
typedef struct MirCertQuery {
  int32_t  struct_size;      /* = sizeof(MirCertQuery) */
  int32_t  num_points;       /* K >= 2 waypoints per row */
  int32_t  max_depth;        /* 0 .. 20: the deepest level of the bisection */
  int32_t  max_evaluations;  /* >= 1: clearance evaluations per row */
  int32_t  max_leaves;       /* >= 0: the capacity of leaves per row */
  uint32_t flags;            /* MIR_CERT_BRACKET; unknown bits are MIR_E_INVALID */
  float    tol;              /* > guard: the width a bracket is closed to */
  float    guard;            /* >= 0: subtracted from every bound, for the float32 error of an evaluation */
} MirCertQuery;
int mir_cert_query_sizeof(void);
int mir_certify_path(MirHandle h, const MirCertQuery* q, const MirPlanQuery* pq, const float* probes, const int32_t* probe_link,
                     const int32_t* dof_qadr, const int64_t* env_idx, int32_t n_rows, const float* qpos_start /* (R,nq) nullable */,
                     const float* paths /* (R,K,D) */, float* seg_lower /* (R,K-1) */, float* seg_upper /* (R,K-1) */,
                     int32_t* seg_status /* (R,K-1) */, float* row_lower /* (R) */, float* row_upper /* (R) */, int32_t* row_status /* (R) */,
                     int32_t* row_first /* (R) */, int32_t* leaves /* (R,max_leaves,3) nullable */, int32_t* stats /* (R,4) nullable */,
                     void* stream);

/* ---- certified clearance: self and carried object -----------------------------------------------------------------
 * `robot.certify_sweep(path, self_collision=True, attached_entity=cube, ...)`: mir_certify_path with the two tests it left sampled.
 * For R rows ONE launch (mir_cert.hip, one wave64 per row) brackets, per segment, the continuous minimum of the scene clearance
 * (exactly as mir_certify_path, the carried body's spheres included) AND of the self clearance of mir_path_clearance_self / _carry:
 * the lowest s_ij = |x_i - x_j| - (r_i + r_j) over the enabled pairs of the N + E spheres, capped at self_max = sq->max_distance.
 * Why it holds.  Take sphere i on link a (local centre c_i) and sphere j on link b, D = x_i - x_j.
 *   1. s_ij = |D| - (r_i + r_j) and d|D|/dt = D^ . (x_i' - x_j').
 *   2. Along q(t) = a + t dq a planned joint k on the path to the world of BOTH links adds nothing to d|D|/dt: a revolute one adds
 *      dq_k w_k x D to the relative velocity, which is perpendicular to D; a prismatic one adds 0.
 *   3. Only the joints strictly below c = lca(a, b), on either branch, count.
 *   4. Hence |d s_ij / dt| <= v_ij = rel(i, c) + rel(j, c), with rel(i, c) the sum over the planned dofs k of the bodies from a up
 *      to, not including, c of |dq_k| (S[a] - S[body_k] + |c_i|) for a revolute k and |dq_k| |axis_k| for a prismatic one: the rho_ik
 *      of mir_certify_path, restricted to the branch.
 *   5. Links in different chains (c = the world, or a chain start that is not common): nothing is restricted.  6. a == c: rel(i, c) = 0.
 *   7. Capping at self_max keeps the Lipschitz property, so 8. min(s_ij(t), self_max) >= min(s_ij(tm), self_max) - |t - tm| v_ij, and
 *   9. one evaluation at the midpoint of an interval bounds every enabled pair on all of it, as for the scene test.
 *   A carried body C follows link Lk by the rigid grasp G = (p_G, q_G) of the row, so its spheres are spheres of Lk with local centre
 *   p_G + R_G c_i, whose norm is at most cn_i = |p_G| + |c_i| (this bound is used: no rotation enters the rounding).  In the scene test
 *   a probe on C gets cert_speed(S[Lk], cn_i, A[Lk], B[Lk], P[Lk]); in the pair test it counts as sitting on Lk for the LCA, while its
 *   mask row stays link_mask[C].
 * Arguments mean what they mean in mir_certify_path and mir_path_clearance_self / _carry: N = pq->n_probes probes take the scene test,
 *   N + sq->n_extra the pair test under sq->link_mask at sq->self_margin; cq names C and Lk, C's geoms are in pq->skip_geoms; grasp
 *   (R, 7) nullable: from the start row; grasp_used (R, 7) nullable.
 * Rule per row and segment: that of mir_certify_path with two brackets.
 *   1., 2. as there, with cn_i above for the probes on C, plus the branch sums: per body a and per count t = 0 .. depth(a) + 1 of
 *     bodies walked from a upward (k = a, parent(a), ...: the order is part of the rule), three non-negative float32 sums dA = sum
 *     |dq_k| over revolute k, dSB = sum |dq_k| (S[a] - S[body_k]) over revolute k, dP = sum |dq_k| |axis_k| over prismatic k; each
 *     difference, product and sum is one rounding (no fused multiply-add).  They are NOT formed as differences of A, B, P: the
 *     cancellation would make the error absolute, which the factor 1.0001 does not cover.  rel(i, c) = (cn_i dA + dSB) + dP at t =
 *     the bodies from a up to, not including, c (all of the chain when there is no common ancestor; none for the world);
 *     v_ij = (rel(i, c) + rel(j, c)) 1.0001, never below 0.
 *   3., 4. Every evaluation (endpoints with hw = 0, nodes) yields u = min_i d_i and m = min_i (d_i - hw v_i) over the first N probes,
 *     as mir_certify_path, and in the float32 arithmetic of mir_path_clearance_self u_s = min(self_max, lowest s_ij) and m_s = the
 *     lowest min(s_ij, self_max) - hw v_ij over the enabled pairs (no enabled pair: u_s = m_s = self_max).  upper = min(upper, u),
 *     upper_s = min(upper_s, u_s), lo = m - guard, lo_s = m_s - guard.  Witness (not with BRACKET): u < margin or u_s < self_margin
 *     ends the segment BLOCKED, both lowers lowered by this evaluation's lo and lo_s.  A node is a LEAF when the leaf test of
 *     mir_certify_path holds for (lo, upper, margin) AND for (lo_s, upper_s, self_margin).  max_depth, DEPTH, the dyadic successor
 *     and the budget (an evaluation is a configuration) are as there.
 *   5., 6. BUDGET and NOT_FINITE as there, both lowers -INFINITY; any of the N + E centres not finite ends the segment NOT_FINITE; a
 *     grasp that is not finite (or a given quaternion of squared norm < 1e-30) makes every segment of the row NOT_FINITE.
 *   7. Status, in this order: NOT_FINITE; BUDGET; BLOCKED: upper < margin || upper_s < self_margin; DEPTH; CLEAR: lower >= margin &&
 *     lower_s >= self_margin; else UNDECIDED.  With sq NULL the self half of every conjunction is absent.
 *   8. MIR_PLAN_IGNORE_COLLISION: CLEAR with lower = upper = max_distance and lower_s = upper_s = self_max.
 * Identity.  mir_certify_path_carry with sq NULL and no probe on C returns the bytes of mir_certify_path; so does
 *   mir_certify_path_self with an all-zero mask and n_extra = 0 in the scene outputs, the leaves and the stats.
 * Outputs: those of mir_certify_path, plus seg_self_lower, seg_self_upper (R, K-1), row_self_lower, row_self_upper (R), each nullable.
 * Every loop is bounded by K, nbody, N + E, max_depth or max_evaluations; no input can keep a wave running.
 * Refusals, none of which launches anything, in this order:
 *   a. those of mir_certify_path's own query ("null argument" ... "tol <= guard (the bracket could never close)");
 *   b. _self with sq NULL: "null self query"; _carry with sq and cq both NULL: "neither a MirSelfQuery nor a MirCarryQuery
 *      (mir_certify_path judges the scene test alone)"; sq NULL with a self output: "seg_self_lower / seg_self_upper / row_self_lower /
 *      row_self_upper without a MirSelfQuery"; cq NULL with grasp: "grasp without a MirCarryQuery"; with grasp_used: "grasp_used without
 *      a MirCarryQuery";
 *   c. everything mir_path_clearance_self / _carry refuses (the self query first, then the plan query, the rows, the probes, the dofs,
 *      the carry query);
 *   d. MIR_E_CAPACITY: "rows x max(num_points x n_dofs, 3 max_leaves) beyond 2^31 - 1"; then the LDS of a row, F + 4 N + 4 (N + E), plus
 *      16 (N + E) with sq, with F = 24864 bytes fixed, beyond 65536: "the speed bounds and the sphere list do not fit 64 KB of LDS
 *      (n_probes, n_probes + n_extra)" (with at most 1024 probes per call it always fits today).
 *   n_rows == 0, or every output NULL, returns MIR_OK without a launch.
 * What it does not do.  mir_plan_path does not use this rule for its own edges.  The lever is the chain at full stretch, not the
 *   configuration's.  Link geoms other than spheres do not enter the pair test.
 * (Added entry points: MIR_VERSION and every struct and other entry point stay as they are.) */
int mir_certify_path_self(MirHandle h, const MirCertQuery* q, const MirPlanQuery* pq, const MirSelfQuery* sq, const float* probes,
                          const int32_t* probe_link, const int32_t* dof_qadr, const int64_t* env_idx, int32_t n_rows,
                          const float* qpos_start /* (R,nq) nullable */, const float* paths /* (R,K,D) */, float* seg_lower /* (R,K-1) */,
                          float* seg_upper /* (R,K-1) */, float* seg_self_lower /* (R,K-1) */, float* seg_self_upper /* (R,K-1) */,
                          int32_t* seg_status /* (R,K-1) */, float* row_lower /* (R) */, float* row_upper /* (R) */,
                          float* row_self_lower /* (R) */, float* row_self_upper /* (R) */, int32_t* row_status /* (R) */,
                          int32_t* row_first /* (R) */, int32_t* leaves /* (R,max_leaves,3) nullable */, int32_t* stats /* (R,4) nullable */,
                          void* stream);
int mir_certify_path_carry(MirHandle h, const MirCertQuery* q, const MirPlanQuery* pq, const MirSelfQuery* sq /* nullable */,
                           const MirCarryQuery* cq /* nullable */, const float* probes, const int32_t* probe_link, const int32_t* dof_qadr,
                           const int64_t* env_idx, int32_t n_rows, const float* qpos_start /* (R,nq) nullable */,
                           const float* grasp /* (R,7) nullable */, const float* paths /* (R,K,D) */, float* seg_lower, float* seg_upper,
                           float* seg_self_lower, float* seg_self_upper, int32_t* seg_status, float* row_lower, float* row_upper,
                           float* row_self_lower, float* row_self_upper, int32_t* row_status, int32_t* row_first,
                           float* grasp_used /* (R,7) nullable */, int32_t* leaves, int32_t* stats, void* stream);

/* ---- trajectory optimisation: a joint path moved down the gradient of smoothness plus an obstacle cost, in one launch ----------
 * `robot.optimize_path(path)`: mir_plan_path returns a path that is feasible and nothing more, mir_blend_path rounds its corners towards
 * the obstacle it went round, mir_certify_path can only say BLOCKED.  For R rows ONE launch (mir_opt.hip, one wave64 per row) takes
 * each row's joint path as a seed and moves its interior waypoints by covariant gradient descent (the update of CHOMP: Ratliff,
 * Zucker, Bagnell, Srinivasa 2009) with a backtracking line search, sweeps the result with the planner's edge rule and returns it --
 * or, where the sweep blocks, the input.  It reads the scene's state like mir_path_clearance and writes nothing a later call can see.
 * Inputs.  paths (R, K, D), 3 <= K <= MIR_PLAN_MAX_POLY, the layout mir_plan_path and mir_blend_path(num_waypoints) return; xi =
 *   (q_0 .. q_{K-1}), n = K - 2 interior waypoints.  probes, probe_link, dof_qadr, pq->skip_geoms, margin, max_distance, resolution,
 *   flags, rows, env_idx, clamping and qpos_start are those of mir_path_clearance (pq->n_probes = N; with sq the E extra probes follow);
 *   sq and cq as in mir_blend_path: the carried body's grasp comes from the start row.  w_s = smooth_weight, w_o = obstacle_weight
 *   (MIR_PLAN_IGNORE_COLLISION: w_o counts as 0, nothing is evaluated and the sweep passes), eps = activation, alpha_0 = step.
 *   Constants from the host, rounded once from double: km1 = K - 1, hk = (K - 1) / 2, ik = 1 / (K - 1), r_i = i / (i + 1), i = 1 .. n (the
 *   reciprocal pivots of tridiag(-1, 2, -1): its pivots are (i + 1) / i).  x / y below is the refined division of the planner's edge
 *   rule (1 / y, one Newton step on the quotient).  Every line below is one float32 rounding unless it says otherwise.
 * 1. Checks on the input, in this order: a value of the row's path that is not finite: NOT_FINITE.  Every waypoint compares equal to
 *   the first in every dof (a failed plan): NO_MOTION.  An interior waypoint with a dof outside [lo_j, hi_j]: OUT_OF_LIMITS.  All
 *   three return the input; cost, stats and grad0 are zero, min_d is +infinity (as it is with MIR_PLAN_IGNORE_COLLISION, where nothing is
 *   evaluated).  Waypoints are not compacted.
 * 2. Cost of a path, U = w_s S + w_o O.
 *   S: per dof j, s_j = sum over i = 0 .. K-2, ascending, of e e with e = q_{i+1,j} - q_{i,j}; ss = sum of s_j, j ascending; S = hk ss.
 *   O: at each interior waypoint i = 1 .. K-2, ascending: the forward kinematics of clear(q_i) (mir_path_clearance), then per probe
 *   p < N the winner of mir_signed_distance's minimum over the unskipped geoms, b_ip = signed distance - radius_p; a probe counts when
 *   it has a winner with b_ip <= max_distance; d_ip = b_ip - margin; c(d) = eps / 2 - d for d < 0; ((d - eps)(d - eps)) / (2 eps) for
 *   0 <= d <= eps; 0 above, and 0 for a probe that does not count.  The probes are summed in chunks of 64, a chunk by the butterfly
 *   v_l <- v_l + v_{l xor 32}, then xor 16, 8, 4, 2, 1 (absent probes are 0), chunk sums added ascending to a running sum that passes
 *   from waypoint to waypoint: oo.  O = ik oo.  U = (w_s S) + (w_o O).  A geom record, grasp or probe centre that is not finite
 *   makes O +infinity.
 * 3. Gradient at interior waypoint i, dof j: g_ij = w_s (km1 (((q_i + q_i) - q_{i-1}) - q_{i+1})) + w_o (ik G_ij), with G_ij the sum
 *   over the probes, in the order of O's sum but per waypoint, of c'(d_ip) (n_ip . J_pj): c'(d) = -1 for d < 0, (d - eps) / eps for
 *   0 <= d <= eps, else 0; n_ip = the winner's outward normal turned into the world by the winner's frame; J_pj = a_j x (c_p - o_j)
 *   for a revolute planned joint j on the chain from the world to probe p's link, a_j for a prismatic one, 0 off the chain; a_j = the
 *   joint's axis turned by the world rotation of its body, o_j = the world position of its body, c_p the probe's world centre, all at
 *   q_i.  A probe of the carried body takes the chain of the attach link.  (The products inside n . J are the compiler's to fuse.)
 * 4. Covariant step.  M = km1 tridiag(-1, 2, -1) on the interior waypoints; delta = M^-1 g per dof by the Thomas recurrence:
 *   y_1 = g_1, y_i = g_i + (r_{i-1} y_{i-1}); x_n = r_n y_n, x_i = r_i (y_i + x_{i+1}); delta_i = ik x_i.  Candidate: q'_i = q_i -
 *   (alpha delta_i) at the interior waypoints.  With w_o = 0 and alpha w_s = 1 the candidate is the straight line between the ends at
 *   equal spacing, up to rounding.
 * 5. Line search, per iteration: alpha = alpha_0; a candidate is rejected when an interior waypoint leaves [lo, hi] (it is then not
 *   evaluated), when U(xi') is not finite or when not U(xi') < U(xi); a rejection halves alpha (alpha <- 0.5 alpha), at most
 *   max_halvings times (max_halvings + 1 candidates).  No candidate accepted: the row stops, stop = STALLED.  The pass that gives
 *   U(xi') leaves the gradient at xi'.
 * 6. Stop.  An accepted step with U(xi) - U(xi') < ftol U(xi): stop = CONVERGED.  max_iterations iterations (each accepted or stalled)
 *   done: stop = ITERATIONS (also for max_iterations = 0).
 * 7. Validation.  The configuration q_0, then edge(q_i, q_{i+1}), i = 0 .. K-2, of what the descent reached, by the rule of
 *   mir_plan_path: clear(q) with the scene test at margin first, then (sq) the self test at self_margin, the carried body riding along
 *   (cq); the first sample that fails ends it: BLOCKED (scene) or BLOCKED_SELF, and path_out holds the INPUT's bits.  All clear: OK,
 *   and path_out holds xi.  The end waypoints always hold the input's bits.  The cost has no self term.
 * Outputs.  path_out (R, K, D); status (R): MIR_PLAN_OK or MIR_OPT_*; cost (R, 4), nullable: S and O of the input, S and O of what the
 *   descent reached (also where the sweep then blocked); stats (R, 6), nullable: iterations, accepted steps, halvings, configurations
 *   evaluated in the descent (n per pass, the input's pass included), configurations checked in the sweep, stop (MIR_OPT_STOP_*);
 *   min_d (R), nullable: the lowest d_ip over the interior waypoints and the probes of the path that path_out holds (max_distance -
 *   margin for a probe that does not count); grad0 (R, K, D), nullable: g at the INPUT path, zero rows at the ends -- a test hook that
 *   pins the kernel's arithmetic; it costs one store per value.
 * LDS: the fixed part of mir_path_clearance + 3 K 64 bytes + (sq) 16 (N + E) bytes must fit 64 KB, else MIR_E_CAPACITY.
 * MIR_E_INVALID, besides everything mir_path_clearance(_self, _carry) refuses: a NULL q, pq, paths, path_out or status; struct_size !=
 *   sizeof(MirOptQuery); K outside 3 .. MIR_PLAN_MAX_POLY; an unknown flag bit; a weight, step, activation or ftol that is not finite;
 *   smooth_weight <= 0; obstacle_weight < 0; step <= 0; activation <= 0; ftol < 0; negative max_iterations or max_halvings;
 *   max_distance < margin + activation.  None of them launches anything; n_rows = 0 returns MIR_OK.
 * What it does not do.  No self-collision term in the cost (the sweep alone tests it).  The obstacle cost is collocated at the
 *   waypoints: between them only the sweep looks, as coarsely as the edge rule.  No workspace-velocity weighting of the obstacle cost.
 *   No velocity, acceleration or torque limits (mir_retime_path).  The ends are fixed (a goal SET and a pose goal are the planner's: mir_plan_path_goals, mir_plan_path_pose), no restarts; a BLOCKED
 *   row is not repaired; the planner does not call it.  Parity with MoveIt's CHOMP, TrajOpt and cuRobo is unpinned.
 * (Added struct and entry point: MIR_VERSION and every other struct and entry point stay as they are.) */
#define MIR_OPT_BLOCKED 48
#define MIR_OPT_BLOCKED_SELF 49
#define MIR_OPT_NOT_FINITE 50
#define MIR_OPT_NO_MOTION 51
#define MIR_OPT_OUT_OF_LIMITS 52
#define MIR_OPT_STOP_NONE 0 /* no descent ran (a check of 1. failed) */
#define MIR_OPT_STOP_ITERATIONS 1
#define MIR_OPT_STOP_CONVERGED 2
#define MIR_OPT_STOP_STALLED 3
typedef struct MirOptQuery {
  int32_t  struct_size;     /* = sizeof(MirOptQuery) */
  int32_t  num_waypoints;   /* K: 3 .. MIR_PLAN_MAX_POLY */
  int32_t  max_iterations;  /* >= 0 */
  int32_t  max_halvings;    /* >= 0 halvings of alpha per iteration */
  uint32_t flags;           /* 0; unknown bits are MIR_E_INVALID */
  float    smooth_weight;   /* w_s > 0 */
  float    obstacle_weight; /* w_o >= 0 */
  float    step;            /* alpha_0 > 0 */
  float    activation;      /* eps > 0, m: the distance beyond the margin at which the obstacle cost starts */
  float    ftol;            /* >= 0: relative decrease of U below which the row has converged */
} MirOptQuery;
int mir_opt_query_sizeof(void);
int mir_optimize_path(MirHandle h, const MirOptQuery* q, const MirPlanQuery* pq, const MirSelfQuery* sq /* nullable */,
                      const MirCarryQuery* cq /* nullable */, const float* probes /* (N+E,4) device */,
                      const int32_t* probe_link /* (N+E) HOST, nullable */, const int32_t* dof_qadr /* (D) HOST */,
                      const int64_t* env_idx /* device, nullable */, int32_t n_rows, const float* qpos_start /* (R,nq) nullable */,
                      const float* paths /* (R,K,D) */, int32_t K /* = q->num_waypoints */, float* path_out /* (R,K,D) */,
                      int32_t* status /* (R) */, float* cost /* (R,4) nullable */, int32_t* stats /* (R,6) nullable */,
                      float* min_d /* (R) nullable */, float* grad0 /* (R,K,D) nullable */, void* stream);

/* ---- cameras / pixels (BASELINE.json configs[4]) ---------------------------------
 * scene.add_camera(res=(W,H), pos, lookat, fov)   gym_genesis/tasks/franka/cube_pick.py:56-63
 * cam.set_pose(pos, lookat) + cam.render()[0]      gym_genesis/tasks/franka/cube_pick.py:166-176,
 *                                                  gym_genesis/env.py:97-98
 * The reference renders through Genesis's OpenGL rasteriser over mesh assets that are not in the
 * reference tree; here the image is formed from the scene's own collision primitives (boxes, planes;
 * spheres and capsules as their bounding boxes, or as themselves with MIR_VIS_ROUND_GEOMS; hulls as their
 * bounding boxes) by a tiled HIP kernel: pinhole camera (vertical fov, +z up, pixel-centre sampling, row 0 = top),
 * nearest primitive per pixel, Lambert shading from one directional light, a checker on planes. */
typedef struct MirCameraSpec {
  int32_t width, height; /* res=(W,H) */
  double pos[3], lookat[3], up[3];
  double fov_deg; /* vertical field of view, degrees */
} MirCameraSpec;

typedef struct MirVisualSpec {
  int32_t struct_size; /* = sizeof(MirVisualSpec) */
  int32_t flags;       /* MIR_VIS_* bits; 0 = every sphere, capsule and hull is drawn as its bounding box */
  double geom_rgb[MIR_MAX_GEOM][3]; /* albedo per geom, 0..1 */
  double light_dir[3];              /* direction TOWARDS the light (normalised by the library) */
  double ambient, diffuse;          /* colour = albedo * (ambient + diffuse * max(0, n.l)) */
  double sky_rgb[3];                /* rays that hit nothing */
  double checker_rgb[2][3];         /* plane geoms: albedo of the two checker colours */
  double checker_size;              /* checker cell edge, metres */
} MirVisualSpec;

/* MirVisualSpec.flags.  MIR_VIS_ROUND_GEOMS: spheres and capsules are drawn as the exact sphere and capsule in every render entry point,
 * mode and channel (RGB, depth, segmentation, normal; shading per pixel from the surface normal); hulls stay bounding boxes.  Off (the
 * default) the images are those of the bounding boxes.  Any other bit: MIR_E_INVALID. */
#define MIR_VIS_ROUND_GEOMS 1

#define MIR_RENDER_PER_ENV 0 /* one image per env, camera pose relative to the env (cube_pick.py:166-171) */
#define MIR_RENDER_GLOBAL 1  /* one image of all envs placed at env_offset (cube_pick.py:174-176) */

int mir_visual_sizeof(void);

/* Render RGB8 images of the current state.  mode PER_ENV: pixels (B,H,W,3) u8, env e drawn alone
 * as seen from `cam` in its own frame (env_offset ignored).  mode GLOBAL: pixels (H,W,3) u8, every env
 * drawn displaced by env_offset[e] (B,3 f32 device, NULL = all zero); plane geoms are drawn once.
 * cam / vis are host structs (copied into the launch).  pixels is a device pointer.  B x H x W x 3 may exceed 2^32 bytes (64-bit
 * image bases); MIR_E_CAPACITY when a single image reaches 2^32 bytes or a per-env call has more than 65535 images.
 * Link poses: from the first render on, every call that advances the state also leaves the link poses of its final state for the
 * rasteriser, and a render queued behind it (same stream order as the calls that touched the state, as for every call on a handle)
 * launches no forward kinematics of its own; behind mir_reset / mir_autoreset / mir_set_state it does. */
/* A counter that every call which changes the positions of the bodies advances (steps, resets, state writes): two reads that return
 * the same value bracket calls that left the scene as it was -- an image rendered in between is still the image of the scene.
 * (>= 0: the counter modulo 2^31.) */
int mir_get_state_version(MirHandle h);

int mir_render(MirHandle h, const MirCameraSpec* cam, const MirVisualSpec* vis, int32_t mode, const float* env_offset,
               uint8_t* pixels, void* stream);

/* Per-env images from PER-ENV cameras (the wrist cameras that follow a link:
 * gym_genesis/tasks/franka/cube_stack_kitchen_batch.py:185-192, gym_genesis/tasks/so101/cube_stack_batch.py:199-213).
 * cam gives res / fov / default up; cam_pos, cam_lookat (B,3) f32 device, in the env's own frame; cam_up (B,3) nullable.
 * A view direction parallel to the up hint falls back to up = +y, then +x (also in mir_render). */
int mir_render_cams(MirHandle h, const MirCameraSpec* cam, const MirVisualSpec* vis, const float* cam_pos, const float* cam_lookat,
                    const float* cam_up, uint8_t* pixels, void* stream);

/* The four images of Genesis's cam.render(rgb, depth, segmentation, normal) in one call.  Every pointer is a device pointer and
 * nullable; the shapes are those of mir_render: (B,H,W[,3]) per env, (H,W[,3]) in mode GLOBAL.
 *   rgb:          uint8 (..,3), exactly what mir_render / mir_render_cams write (the same kernels).
 *   depth:        float32, metres along the camera's forward axis (planar z-depth, not the distance along the ray); sky = 0.0.
 *   segmentation: int32, sky = -1, else the id of the visible surface: seg_level 0 ("link") = the geom's body index in the scene
 *                 (static world geoms, floor and slab, are body 0), seg_level 1 ("geom") = the geom's index in the scene's geom table.
 *                 In mode GLOBAL the id carries no env index.
 *   normal:       uint8 (..,3), the unit outward world-frame normal of the visible face as round((n + 1) / 2 * 255), clamped like the
 *                 colours; a plane's normal is the one facing the camera; sky = 0 0 0.
 * Spheres and capsules are drawn as in RGB: as their bounding boxes (depth and normals those of the box), or with MIR_VIS_ROUND_GEOMS
 * as themselves (the normal of the curved surface at the pixel).
 * rgb goes through the kernels of mir_render; depth / segmentation / normal through ONE further pass that writes any subset of them.
 * mode, env_offset and cam_pos / cam_lookat / cam_up mean what they mean for mir_render and mir_render_cams (per-env cameras: cam_pos
 * and cam_lookat non-null, mode PER_ENV).  MIR_E_INVALID: struct_size != sizeof(MirRenderOutputs), seg_level not 0 / 1, every
 * channel null, depth / segmentation / normal not 16-byte aligned, and what mir_render refuses; MIR_E_CAPACITY: width x height x 4
 * reaches 2^32 bytes while an aux channel is asked for (checked before anything is drawn), and what mir_render refuses. */
typedef struct MirRenderOutputs {
  int32_t struct_size;   /* = sizeof(MirRenderOutputs) */
  int32_t seg_level;     /* 0 = link, 1 = geom */
  uint8_t* rgb;          /* nullable: exactly what mir_render / mir_render_cams write */
  float* depth;          /* nullable */
  int32_t* segmentation; /* nullable */
  uint8_t* normal;       /* nullable */
} MirRenderOutputs;
int mir_render_outputs(MirHandle h, const MirCameraSpec* cam, const MirVisualSpec* vis, int32_t mode, const float* env_offset,
                       const float* cam_pos, const float* cam_lookat, const float* cam_up, const MirRenderOutputs* out, void* stream);

/* ---- batched inverse kinematics ---------------------------------------------------
 * robot.inverse_kinematics(link=eef, pos=(B,3), quat=(B,4), init_qpos=..., envs_idx=...) -> (B, n_dofs)
 *      examples/franka/pick_cube_state.py:46-51, examples/franka/stack_cube_state.py:78-83
 * Genesis's IK lives in the external package; this is a damped-least-squares solver on the scene's own kinematics,
 * defined here and restated independently by the oracle (oracle/orc_rigid.c: orc_ik):
 *   q_acc = the seed, lambda^2 = damping^2;  repeat up to max_iters, with q the candidate (the seed at first):
 *     e = [p* - p(q) ; rotvec(q* q(q)^-1)]   (rotation part dropped when target_quat == NULL), m = |e_pos|/pos_tol + |e_rot|/rot_tol;
 *     the candidate is ACCEPTED when m fell below the accepted iterate's (always at first): q_acc = q, its e and its 6 x n geometric
 *     Jacobian J of the chain are kept, lambda^2 <- max(lambda^2 / 4, damping^2 / 256), and the step is STALLED when m fell by less than
 *     1 %; otherwise it is REJECTED: lambda^2 <- min(8 lambda^2, 64 damping^2), also stalled (Levenberg - Marquardt, round 6: fixed damping
 *     crept for 32 iterations towards targets whose Jacobian has a small singular value, and a handful of such envs set the time of
 *     every launch).  Stop the env when |e_pos| < pos_tol and |e_rot| < rot_tol at the accepted iterate, or after three stalled
 *     iterations in a row (a target beyond the joint limits or the reach);
 *     dq = J^T (J J^T + lambda^2 I)^-1 e of the accepted iterate, scaled down so that max |dq_i| <= max_step;  q = q_acc + dq,
 *     clamped to the joint ranges (respect_joint_limit).  The result is q_acc.
 * Only the scalar joints on the chain world -> link move; every other entry of the result is the seed. */
typedef struct MirIkOptions {
  int32_t max_iters;           /* default 20 (Genesis's max_solver_iters, recalled: the package is not in /root/reference; 32 until round 6) */
  int32_t respect_joint_limit; /* default 1 */
  double damping;              /* default 0.05 */
  double pos_tol, rot_tol;     /* defaults 5e-4 m, 5e-3 rad */
  double max_step;             /* default 0.5 rad (or m) per iteration */
} MirIkOptions;

/* target_pos (B,3), target_quat (B,4 wxyz) nullable, init_qpos (B,n_arm) nullable (NULL = the scene's current joint
 * positions), opt nullable (defaults); qpos_out (B,n_arm) = every scalar joint in body order; err_out (B,2) nullable =
 * final |e_pos|, |e_rot|.  The scene state is not modified. */
int mir_inverse_kinematics(MirHandle h, int32_t link_body, const float* target_pos, const float* target_quat, const float* init_qpos,
                           const MirIkOptions* opt, float* qpos_out, float* err_out, void* stream);

/* The same solver for a LIST OF ROWS: robot.inverse_kinematics(link, pos, quat, init_qpos=..., envs_idx=idx) as the reference's experts
 * call it on every step of their loops (examples/franka/pick_cube_state.py:46-51 with envs_idx = arange(B) and ONE quaternion expanded
 * to the batch; examples/so_101/collect_task_stack_cube_batch.py:90-95 with init_qpos of the arm's columns) in ONE launch -- no
 * scatter of the targets to batch rows in front of it, no gather of the result rows behind it.  Row k of qpos_out (n_rows, n_arm) /
 * err_out (n_rows, 2) belongs to env env_idx[k] (int64, device; NULL: n_rows = num_envs, row k = env k; an index outside the batch is
 * clamped).  flags say how the inputs are addressed: by row k -- (n_rows, .) arrays -- unless MIR_IK_POS_BY_ENV / MIR_IK_QUAT_BY_ENV /
 * MIR_IK_INIT_BY_ENV ((num_envs, .) arrays, row of the env); MIR_IK_QUAT_ONE: target_quat is one quaternion for every row.
 * init_qpos holds init_ncols columns of the joint row starting at init_col0 (0, 0: all n_arm columns); the other joints are seeded from
 * the scene state.  rows == NULL: mir_inverse_kinematics. */
#define MIR_IK_POS_BY_ENV 1u
#define MIR_IK_QUAT_BY_ENV 2u
#define MIR_IK_QUAT_ONE 4u
#define MIR_IK_INIT_BY_ENV 8u
typedef struct MirIkRows {
  const int64_t* env_idx;  /* device, n_rows entries, or NULL */
  int32_t n_rows;
  uint32_t flags;
  int32_t init_col0, init_ncols;
} MirIkRows;
int mir_inverse_kinematics_rows(MirHandle h, int32_t link_body, const MirIkRows* rows, const float* target_pos, const float* target_quat,
                                const float* init_qpos, const MirIkOptions* opt, float* qpos_out, float* err_out, void* stream);

/* ---- multi-link inverse kinematics: axis masks, dof subsets, restarts ------------------------------------------
 * robot.inverse_kinematics(link, pos, quat, pos_mask=..., rot_mask=..., dofs_idx_local=..., max_samples=...) and
 * robot.inverse_kinematics_multilink(links=[left_finger, right_finger], poss=..., quats=...) of Genesis (parity with Genesis itself is
 * unpinned, the one-axis rule below included: the package is not in the reference tree; the argument names follow its API as far as it
 * is remembered).  ONE launch of a kernel of its own (csrc/mir_ikm.hip; mir_inverse_kinematics and its kernel are untouched and keep
 * their bits).  The scene state is read and never written.  Restated independently by tests/ikm_ref.py.
 * It is the iteration of mir_inverse_kinematics with these generalisations, for the L = n_links links (1 .. 4) at once:
 *   Task rows of link l.  ep_l = pos_mask o (p*_l - p_l) in world axes, the linear Jacobian rows masked alike.  Orientation:
 *     rot_mask all true:  er_l = rotvec(q*_l q_l^-1) as in mir_inverse_kinematics, rows = the angular Jacobian J_w;
 *     one true entry k:   align the link's own axis k with the target's: a = R_l e_k, a* = R*_l e_k,
 *                         er_l = atan2(|a x a*|, a . a*) (a x a*) / |a x a*|, 0 when |a x a*| < 1e-9; rows = (I - a a^T) J_w, so the
 *                         rotation about the axis is free;
 *     no true entry, or target_quat == NULL: no orientation rows (whatever rot_mask says).
 *     Two true entries: MIR_E_INVALID.  The masks are shared by all links.
 *   Metric m = sum_l (|ep_l| / pos_tol + |er_l| / rot_tol).  A row is converged when every link has |ep_l| < pos_tol and |er_l| < rot_tol
 *     at the accepted iterate.  The accept / reject / stall rules, the lambda^2 schedule, the max_step scaling, the clamp to the joint
 *     ranges and max_iters are those of mir_inverse_kinematics, word for word.
 *   Moving joints: the scalar joints on the chain of at least one link that are also in dof_mask.  Every other entry of the result is
 *     the seed, bit for bit.
 *   Limit rule (only with respect_joint_limit), evaluated when an iterate is accepted, with g = J^T e of that iterate: a limited moving
 *     joint j with q_j == lo_j and g_j < 0, or q_j == hi_j and g_j > 0, has a zero Jacobian column until the next accepted iterate (the
 *     equality is exact: the clamp produced the value).  Without it a joint on its limit keeps being asked to move past it and the
 *     others creep.
 *   Step dq = J^T (J J^T + lambda^2 I)^-1 e = (J^T J + lambda^2 I)^-1 J^T e (the kernel solves the second form; lambda^2 >= damping^2 / 256
 *     keeps the matrix positive definite where the task rows are rank deficient: two rigidly related links, the one-axis projector).
 *   Samples (max_samples >= 1).  Sample 0 starts from the seed.  Sample s >= 1 replaces every moving joint that has a range, of
 *     column k, by lo + (hi - lo) u; joints without a range keep the seed value.  u = (x >> 8) 2^-24 with, in uint32 arithmetic,
 *       x = seed 0x9E3779B1 + env 0x85EBCA77 + s 0xC2B2AE3D + k 0x27D4EB2F + 0x165667B1;
 *       x ^= x >> 16; x *= 0x7FEB352D; x ^= x >> 15; x *= 0x846CA68B; x ^= x >> 16     (env: the env index, not the row).
 *     The first converged sample is the result; if none converges, the sample with the smallest final m, the lower s on a tie.  The
 *     same arguments give the same bits on every call.
 * Rows are addressed as in mir_inverse_kinematics_rows (q->rows; env_idx NULL: n_rows = num_envs, row k = env k; an index outside the
 * batch is clamped).  target_pos (rows or num_envs, L, 3); target_quat (rows or num_envs, L, 4) wxyz, or with MIR_IK_QUAT_ONE (L, 4)
 * for every row, or NULL; init_qpos as in mir_inverse_kinematics_rows.  qpos_out (rows, n_arm); err_out (rows, L, 2) nullable = |ep_l|,
 * |er_l| of the result; iters_out (rows) nullable = iterations summed over the samples the row ran; sample_out (rows) nullable = the
 * sample that produced the result.  Each output element is written once.
 * MIR_E_INVALID: a NULL handle, query, target_pos or qpos_out; struct_size != sizeof(MirIkMulti); n_links outside 1 .. 4; a link outside
 * 1 .. nbody - 1 or hanging off a free body; two true entries in rot_mask; masks that select no task row at all; max_samples < 1; bad
 * options; a bad row description or init columns outside the joint row.  MIR_E_CAPACITY: the union of the chains, with the fixed
 * elements that are no target folded into their children, has more than 16 elements.  n_rows == 0: MIR_OK without a launch.
 * (An added struct and entry point: MIR_VERSION and every other struct stay as they are.) */
typedef struct MirIkMulti {
  int32_t struct_size;      /* = sizeof(MirIkMulti) */
  int32_t n_links;          /* 1 .. 4 */
  int32_t link_body[4];     /* body indices of the spec, 1 .. nbody-1 */
  uint8_t pos_mask[3];      /* world axes x y z of the position error */
  uint8_t rot_mask[3];      /* 0, 1 or 3 true entries */
  uint8_t reserved[2];
  const uint8_t* dof_mask;  /* HOST, n_arm bytes: joint column k may move; NULL: every joint on a chain */
  int32_t max_samples;      /* >= 1 */
  uint32_t seed;
  MirIkRows rows;
} MirIkMulti;
int mir_ik_multi_sizeof(void);
int mir_inverse_kinematics_multilink(MirHandle h, const MirIkMulti* q, const float* target_pos, const float* target_quat /* nullable */,
                                     const float* init_qpos /* nullable */, const MirIkOptions* opt /* nullable */,
                                     float* qpos_out, float* err_out /* nullable */, int32_t* iters_out /* nullable */,
                                     int32_t* sample_out /* nullable */, void* stream);

/* ---- multi-GPU observation gather on the copy path (no reference counterpart: README.md:41-48 is single-device) ----
 * One process per GPU; every rank owns a receive buffer that the other ranks have mapped through HIP IPC (the host side does the
 * handle exchange: gym_genesis/sharding.py: CopyPathGather).  mir_p2p_push enqueues, on `stream` of the CURRENT device, one
 * device-to-device copy of `nbytes` from src to each of the n destinations (addresses inside the peers' buffers; a local address
 * is a plain device copy) and THEN one 4-byte copy of *flag_src to each flag_dst[i]: copies of one stream complete in order, so a
 * receiver that sees the sequence word has the whole block.  No kernel is launched (the copies run on the SDMA engines), which
 * is the point: a collective kernel cannot share a CU with the step kernel's four resident workgroups.
 * mir_p2p_enable makes `peer`'s memory addressable from `device` (idempotent). */
int mir_p2p_enable(int32_t device, int32_t peer);
int mir_p2p_push(void* const* dst, int32_t n, const void* src, uint64_t nbytes, void* const* flag_dst, const void* flag_src, void* stream);
/* mir_p2p_push with one stream per destination (streams[i] carries destination i's block and then its word): the copies to different
 * peers overlap.  nbytes = 0 sends the words only (the acknowledgements of the gather's flow control). */
int mir_p2p_push_streams(void* const* dst, int32_t n, const void* src, uint64_t nbytes, void* const* flag_dst, const void* flag_src,
                         void* const* streams);

/* ---- debug aids (exported for the tests and tools/; not part of the drop-in surface) ---------------------------
 * mir_debug_profile_step: one step with phase timestamps (shader clock) of workgroup 0 into prof (32 x u64, device).
 * mir_debug_poison_lds: overwrite the LDS of every CU with signalling-NaN patterns, so that a kernel reading an LDS slot
 * before writing it yields NaNs instead of plausible stale values (the GPU tests call it before every scene).
 * mir_debug_null_roundtrip: microseconds per (launch of an empty kernel + host-visible completion word), averaged over iters:
 * the floor under one synchronous env.step() on this machine, with none of the physics in it.
 * mir_debug_copy_rows: dst[i] = src[i] for n_floats floats with the step kernel's access shape (64-thread workgroups, 4 B per
 * lane): a known byte count against which rocprofv3's FETCH_SIZE / WRITE_SIZE are calibrated for this access width. */
int mir_debug_profile_step(MirHandle h, unsigned long long* prof, void* stream);
/* profiling builds (-DMIR_PROFILE_SINGLE): the next mir_step_begin / mir_step_go launch -- whichever kernel the split-step protocol
 * picks -- leaves its stamps in prof (160 x u64, device; slot 63 = workgroup to watch) */
int mir_debug_profile_next_step(MirHandle h, unsigned long long* prof);
/* ... and the next launch of the LIST INSTANTIATION of exact contacts (mir_step_end of a step with deferred envs): prof 160 x u64; the
 * first pass's stamps as above, slots 140 / 141 / 142 = end of the second pass on the main / the collision wave, its start */
int mir_debug_profile_next_list_step(MirHandle h, unsigned long long* prof);
/* every following mir_inverse_kinematics call also writes the iterations each env took into iters (B x i32, device; NULL: off) */
int mir_debug_ik_iters(MirHandle h, int32_t* iters);
int mir_debug_null_roundtrip(MirHandle h, int32_t iters, void* stream, double* out_us);
/* n back-to-back launches of the rotated step kernel (split mode 1), cycling through n_actions (B, nu) action blocks, without
 * observation outputs -- or, with outputs = {agent_pos, env_state, reward, terminated} (device pointers, shapes as in
 * mir_step_fused), with the four device outputs of a mir_step_go launch (not its host-visible bytes): lets two events time that kernel the way the fused one is timed (bench.py's roofline).  Advances the state
 * by n steps. */
int mir_debug_rotated_launches(MirHandle h, const float* actions, int32_t n_actions, int32_t n, void* const* outputs, void* stream);
/* n steps in ONE launch, every workgroup through its steps at its own pace, actions (n, B, nu) resident, no outputs: the floor under
 * a launch that would stay resident over several env.step() calls (tools/probes/resident_steps.py).  Advances the state by n steps. */
int mir_debug_resident_steps(MirHandle h, const float* actions, int32_t n, void* stream);
/* the 16-lane kernel's row all-reduce on n_rows rows of 16 floats (device arrays): out[r][l] = lane l's result for row r.  Every lane
 * of a row must hold the same bits (the solver's per-lane decisions rest on it: tests/test_gpu_api.py). */
int mir_debug_row_sum(const float* in, float* out, int32_t n_rows, int device_id, void* stream);
int mir_debug_poison_lds(int device_id, void* stream);
int mir_debug_copy_rows(const float* src, float* dst, int64_t n_floats, int device_id, void* stream);
/* the kernels' convex narrowphase on n pairs given directly (device arrays): in (n,22) = type1, size1[3], pos1[3], quat1[4] wxyz,
 * type2, size2[3], pos2[3], quat2[4]; out (n,8) = hit, pos[3], dist, normal[3] (from geom 1 to geom 2) */
int mir_debug_convex_pairs(const float* in, float* out, int32_t n, int device_id, void* stream);
/* which pixel kernel the following mir_render / mir_render_cams calls of this handle use: generic != 0 forces the kernel that
 * culls per workgroup (the one long primitive lists and odd widths always take), 0 restores the default (per-strip lists built
 * once per render whenever an image has fewer than 64 primitives); strip_rows > 0 (a multiple of 32) overrides the height of a
 * workgroup's strip, 0 restores the default.  The two kernels must agree bit for bit (tests/test_gpu_render.py). */
int mir_debug_render_path(MirHandle h, int32_t generic, int32_t strip_rows);
/* host only (no GPU): the sizes and options of the compiled scene as the text of a C++ struct of literals, `struct <name>` with
 * a `matches(const DevModel&)` member -- the constants of a scene-specialised instantiation of the 16-lane step kernel
 * (csrc/mir_spec_pick.h is this text for the CubePick scene, written by tools/gen_scene_spec.py).  Returns the text length, or
 * MIR_E_* (MIR_E_CAPACITY: the scene belongs to the wave kernel, or cap is too small).  A build-time tool: not thread-safe. */
int mir_debug_emit_spec(const MirSceneSpec* spec, const char* name, char* out, int32_t cap);
/* 1 if this handle's launches use the scene-specialised instantiation (its compiled model matched SpecPick and the environment
 * variable MIR_NO_SPEC was unset at mir_create), else 0 */
int mir_debug_spec_active(MirHandle h);
/* counters of the early terminated bytes (see mir_step_begin): out2[0] = workgroup-launches that sent their bytes from inside the
 * solver loop, out2[1] = workgroup-launches whose early bytes differed from the integrated state (anything but 0 also makes the next
 * API call fail with MIR_E_MASK).  Both always counted (a private counter per workgroup, summed here).  Synchronises the stream;
 * reset != 0 clears the counters. */
int mir_debug_early_mask_stats(MirHandle h, uint32_t* out2, int32_t reset, void* stream);
/* test aid: raises the sticky word by hand, as a kernel that found its early bytes wrong would (the next call fails with MIR_E_MASK) */
int mir_debug_raise_mask_flag(MirHandle h);
/* 1 while mir_step_begin launches may send early bytes on this handle, 0 after MIR_NO_EARLY_MASK=1 or a MIR_E_MASK */
int mir_get_early_mask(MirHandle h);

#ifdef __cplusplus
}
#endif
#endif /* MIRIGID_H */
