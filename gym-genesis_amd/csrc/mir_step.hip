// mir_step.hip — the env.step() hot path as one fused HIP kernel for gfx950 (MI355X).
//
// What it replaces: scene.step() + get_obs() + compute_reward() of the reference
// (/root/reference/gym_genesis/tasks/franka/cube_pick.py:122-181, env.py:61-69), i.e. the
// Genesis rigid-solver pipeline restated in SURVEY.md App. A.
//
// Mapping to CDNA4
//   * workgroup = ONE wave64 = 4 envs x 16 lanes; a 16-lane env group is exactly one DPP "row".
//     Inside a group lane i is "dof i", "body i", "contact i" or "geom i / i+16" depending on the
//     phase, so per-dof / per-body / per-contact solver state is lane-private (registers).
//   * cross-lane traffic inside a group uses DPP: row_ror adds for reductions and row_newbcast
//     for broadcasts (a few cycles each, no LDS round trip).
//   * the two dense solves per Newton iteration (M^-1 f, H^-1 g) are Gauss-Jordan eliminations
//     on register-resident matrix rows (lane i = row i), the pivot row travelling by
//     row_newbcast: no LDS, no sqrt, no forward/back substitution chains.
//   * kinematic-tree recursions are scans: pointer jumping over the parent links for sums over ancestors (forward
//     kinematics, velocities, bias accelerations), DPP suffix sums over the depth-first body lanes for sums over
//     subtrees -- no depth-serial chain; the parent table is a 64-bit register.
//   * per-env working data that other lanes must see (poses, motion subspaces, M, contact
//     Jacobians) lives in ~8 KB of LDS per env, phase-aliased, so 4 workgroups (16 envs) fit a CU
//     and all 4096 envs of the headline batch are co-resident on the 256 CUs.
//   * LDS accesses of a wave execute in order, so the phases of a wave are separated by a compiler-level fence only (WSYNC).
//     The single-step instantiations put a SECOND wave on the same four envs (collision detection, contact arrays, opening and
//     closing forward kinematics, body inertias beside the first wave's dynamics and solves); the two meet at s_barriers.
//   * HBM state is env-major (B, D): with 16 lanes per env a wave touches 4 contiguous 64-byte
//     rows, the coalesced pattern for this lane mapping.  228 B read + 341 B written per env-step (489 B algorithmic:
//     qpos, qvel, warm start, action in; qpos, qvel, warm start, targets, observations, reward, mask out).
//   * the wave runs alone on its SIMD at the headline batch (the batch bounds the occupancy), so the kernel is a serial chain
//     of LDS round trips: loops over contacts / tree masks issue the reads of two or four entries in one batch ahead of
//     the arithmetic, vectors that a whole row needs once travel by row broadcast instead of through LDS, and every global
//     read of a launch (tables, per-lane record, model scalars, state, action, cached poses) leaves before the first LDS
//     store -- one L2 round trip at the start.
//   * instantiations: one step body serves every kind of launch -- single step, rollout loop, the halves of a split step, the
//     rotated launch, the three-contacts-per-lane tier of exact contacts, the contact-force sensor read; StepKind and its table in mir_step.h name and describe them.
#include <hip/hip_runtime.h>

#include <type_traits>
#include <stdint.h>

#include "mir_model.h"
#include "mir_step.h"
#include "mir_spec_pick.h"

#define G MIR_G
#include "mir_dev.h"
#include "mir_convex.h"
#define EPB 4       /* envs per block */
#define JST 52      /* floats per contact in Jb: 3 rows x 16 + 4 pad -> conflict-free ds_read_b128 across contact lanes */
#define MSTR 20     /* row stride of M in LDS (floats): 16-byte aligned rows, conflict-free b128 row reads */
#define JB_SKEW 8   /* see EnvLds::Jb_ */
#define JBROW(Sx, c) (&(Sx).Jb_[(c) * JST + jbs])
static_assert(K16_MAX_CONTACT == G, "lane c owns contact c (one contact per lane; the step_big kinds keep CPL = 3 per lane)");

// optional phase timestamps (debug): block 0, thread 0 records the shader clock at phase boundaries
#ifdef MIR_PROFILE_SINGLE
/* profiling build: the block to stamp is chosen by the host (slot 63 of the buffer), and every Newton iteration gets its own
 * eight slots from 64 on (tools/phase_profile.py) */
/* (prof_mute: the list instantiation's second pass -- the next step's action-independent half -- leaves the first pass's stamps alone and
 *  stamps its own end: slot 140 the main wave, 141 the collision wave) */
#define STAMP(k) do { if (a.prof && !prof_mute && (int)blockIdx.x == prof_blk && threadIdx.x == 0) a.prof[k] = __builtin_readcyclecounter(); } while (0)
#define ITSTAMP(it, k) do { if ((it) < 8) STAMP(64 + 8 * (it) + (k)); } while (0)
#define HSTAMP(k) do { if (a.prof && !prof_mute && (int)blockIdx.x == prof_blk && threadIdx.x == 64) a.prof[k] = __builtin_readcyclecounter(); } while (0)
#else
#define HSTAMP(k) do { } while (0)
#define STAMP(k) do { if (a.prof && blockIdx.x == 0 && threadIdx.x == 0) a.prof[k] = __builtin_readcyclecounter(); } while (0)
#define ITSTAMP(it, k) do { } while (0)
#endif

#ifdef MIR_PROFILE_SINGLE
#define TERMSTAMP() do { if (a.prof && threadIdx.x == 0 && (blockIdx.x & 7) == (unsigned)(prof_blk & 7)) atomicMax(&a.prof[130], (unsigned long long)__builtin_amdgcn_s_memrealtime()); } while (0)
#else
#define TERMSTAMP() do { } while (0)
#endif
namespace {

// ---------------------------------------------------------------------------------------------
// per-env LDS working set (~8 KB).  Three phase-local scratch areas share storage:
//   dyn  (FK .. smooth dynamics)   overlays   contact arrays + Jb
//   col  (collision detection)     overlays   Jb
struct DynScratch {
  float cddq[G][8];               // cdof_dot * qvel: ang(3) pad lin(3) pad
  float cinert[G][12], crb[G][12];
  float cvel[G][8], cfrc[G][8];
};
template <int CPL>
struct ColScratchT {
  float gpos[K16_MAX_GEOM][4], gquat[K16_MAX_GEOM][4];
  int cand[G];
  int cmap[G * CPL];              // contact slot -> candidate lane * 8 + point index
  union {
    float stage[G][8][4];         // narrowphase output per candidate pair: pos, dist
    struct {                      // sweep-and-prune scratch (dead before the narrowphase writes `stage`)
      float lo[K16_MAX_GEOM][4], hi[K16_MAX_GEOM][4];  // world AABB; lo.w = geom type as int bits
      int order[K16_MAX_GEOM];    // non-plane geoms sorted by lo.x
      unsigned hitrow[K16_MAX_GEOM];  // bit b of row a: geoms a < b overlap (AABB) and may collide
      int plist[K16_MAX_PAIR];    // overlapping pairs g1 | g2 << 8 (plane first), in the order of the static list
      int npl, nnp, pad0, pad1;
    } sap;
  };
  float snorm[G][4];
  int count[G];                   // contact points found per candidate (handed from the collision wave to the main wave)
  float clip[48];                 // polygon clipping scratch of the box-box routine (one row)
};
static_assert(sizeof(((ColScratchT<1>*)nullptr)->sap) <= sizeof(((ColScratchT<1>*)nullptr)->stage), "SAP scratch must fit under the staging area");
// CPL = contacts per lane: 1 everywhere but in the step_big kinds (mir_step.h), where lane c owns contacts
// c, c + 16, c + 32 (capacity 48 = MIR_MAX_CONTACT, what the wave-per-env kernel holds).
template <int CPL>
struct ContactArraysT {
  static constexpr int MAXCON = G * CPL;
  float cpos[MAXCON][4];          // pos, dist.  CPL > 1: ALSO the per-iteration base forces (cfb below) -- the positions are dead once the Jacobian rows are built
  float cfrm[MAXCON][12];         // normal, t1, t2 (4-padded)
  float cmeta[MAXCON][4];         // mu, D, k*imp*dist stash / unused, b stash
  float cref[MAXCON][8];          // reference points of body1 / body2 trees (4-padded)
  unsigned cmask[MAXCON][4];      // dof masks of body1, body2, chunk mask, pad
  float cfb[CPL == 1 ? MAXCON : 1][4];  // per-iteration base forces (n, t1, t2), active-row flags (as int bits); CPL > 1: see cpos
};
// (CPL > 1 only: bit c of conB[s] = contact 16 s + c moves dofs of the second tree only -- CPL == 1 keeps those flags in bits 1 .. 16 of
//  `coupled` and has no such words: an empty base, the env block of the one-contact-per-lane instantiations is unchanged)
//  Also CPL > 1 only: what the two waves need to SHARE the narrowphase's box - box trips -- the main wave idles at barrier (2) while the
//  collision wave takes one 5 k-cycle trip after the other, five of them where both fingertips stand on the floor around a cube held by
//  the pads: `bp_ready` (the collision wave has published the candidate list of pass bp_ready - 1), `bb_done` (the main wave has
//  stored the contact points and counts of ITS trips), a polygon-clipping scratch of the main wave's own.)
template <int CPL> struct ConBWords { int conB[CPL]; int bp_ready, bb_done; int conB_pad[(8 - (CPL + 2) % 4) % 4 + 0]; float clip2[48]; };
template <> struct ConBWords<1> {};
template <int CPL>
struct EnvLdsT : ConBWords<CPL> {
  static constexpr int MAXCON = G * CPL;
  float qpos[20], qvel[G], target[G], qacc_ws[G];
  float xpos[G][4], xquat[G][4];
  float cdof[G][8];               // ang(3) pad lin(3) pad
  float M[G][MSTR];
  int ncon, ncand, coupled /* some contact joins the two kinematic trees: the Newton Hessian is not block diagonal */;
  int cin_ready;  // two-wave instantiations: the collision wave has stored the body inertias of this step (main wave spins on it; STEP_LIST48: of pass cin_ready - 1)
  // Phase-aliased working set.  `dyn` (smooth dynamics) and `col` (collision detection) are live AT THE SAME TIME in the
  // single-step instantiation, where a second wave of the workgroup detects collisions while the first one does the dynamics;
  // the contact arrays and the contact Jacobians take the place of both afterwards (CPL == 1: con never overlaps col -- the contact
  // finishing reads the staging area while it writes con; Jb does, and is written after col is dead.  CPL > 1: con reaches into col;
  // the contact finishing there computes all of a lane's contacts into registers first, and stores behind barrier (2)).
  union {
    struct {
      DynScratch dyn;
      ColScratchT<CPL> col;
    };
    struct {
      ContactArraysT<CPL> con;
      // contact Jacobian rows, row c at Jb_[c * JST + jbs]: the rows of the ODD envs of a wave start JB_SKEW floats later.  An env's block
      // is 2280 dwords = 8 mod 32 long, so the 16 consecutive dwords that the 16 lanes of two neighbouring envs read from the same
      // row with one ds_read_b32 (banks = dword mod 32, two envs per 32-lane group) would overlap in 8 banks: every such read -- three
      // per contact in the gradient loop of every Newton iteration -- took two LDS cycles instead of one.  The skew moves the odd env's
      // rows to the other 16 banks; the space comes out of the slack of this half of the union.
      float Jb_[MAXCON * JST + JB_SKEW];
    };
  };
};
typedef EnvLdsT<1> EnvLds;
static_assert(sizeof(EnvLds) == 2280 * 4, "the env block of the one-contact-per-lane instantiations (JB_SKEW above counts on 2280 dwords = 8 mod 32)");
static_assert(sizeof(ContactArraysT<1>) <= sizeof(DynScratch), "the contact arrays must not reach the collision staging area");
static_assert(sizeof(ContactArraysT<1>) + (G * JST + JB_SKEW) * sizeof(float) <= sizeof(DynScratch) + sizeof(ColScratchT<1>), "the skewed Jacobian rows must fit the union");
static_assert(EPB * sizeof(EnvLds) + sizeof(ModelTab) + K16_MAX_VERT * 16 <= 40960, "four workgroups per CU: 160 KB of LDS / 4 (hull vertices included)");
static_assert(EPB * sizeof(EnvLdsT<3>) + sizeof(ModelTab) + K16_MAX_VERT * 16 <= 81920, "the list instantiation (three contacts per lane): two workgroups per CU");

// body-lane constants needed by forward kinematics
struct BodyK {
  int jtype, qadr;
  V3 pos, axis;
  Q4 quat;
};

// forward kinematics of one env group: local joint transforms, then POINTER JUMPING over the parent links -- in every
// round a body composes the (partially composed) transform of its current ancestor pointer and inherits that body's
// pointer, so after r rounds it holds the product over 2^r ancestors: 4 rounds for any tree of up to 16 bodies instead of
// a dependent walk as long as the chain (10 links for a Panda finger).  `parents` packs the 16 parent indices, 4 bits each;
// the ancestor's transform and pointer are gathered lane to lane (ds_bpermute), so a round is one crossbar trip and no LDS fence.
// `row4` = byte offset of the group's first lane in the wave (64 x group).
// SKIPFREE: free-joint bodies are left out (neither read nor written): in the two-wave instantiation the closing FK runs on the
// collision wave while the main wave is still integrating the free bodies' quaternions, and writes their poses itself.
template <bool SKIPFREE = false, class ENV>
__device__ __forceinline__ void group_fk(ENV& S, int lane, int nb, uint64_t parents, const BodyK& k, int row4) {
  V3 P = v3(0, 0, 0);
  Q4 Qx = Q4{1, 0, 0, 0};
  int anc = 0;
  const bool mine = lane < nb && !(SKIPFREE && k.jtype == MIR_JNT_FREE);
  if (lane > 0 && lane < nb && mine) {
    Qx = k.quat;
    P = k.pos;
    if (k.jtype == MIR_JNT_REVOLUTE) {
      float ang = S.qpos[k.qadr], sn, cs;
      sincos_pi2(0.5f * ang, &sn, &cs);
      Qx = qmul(k.quat, Q4{cs, k.axis.x * sn, k.axis.y * sn, k.axis.z * sn});
    } else if (k.jtype == MIR_JNT_PRISMATIC) {
      P = k.pos + qrot(k.quat, S.qpos[k.qadr] * k.axis);
    } else if (k.jtype == MIR_JNT_FREE) {
      P = ld3(&S.qpos[k.qadr]);
      Qx = qnormalize(ld4(&S.qpos[k.qadr + 3]));
    }
    anc = (int)((parents >> (4 * lane)) & 15u);
  }
#pragma unroll 1
  for (int round = 0; round < 4; round++) {
    if (!__any(anc > 0)) break;
    const int src = row4 + ((anc > 0 ? anc : lane) << 2);
    const V3 pa = v3(lane_gather(src, P.x), lane_gather(src, P.y), lane_gather(src, P.z));
    const Q4 qa = Q4{lane_gather(src, Qx.w), lane_gather(src, Qx.x), lane_gather(src, Qx.y), lane_gather(src, Qx.z)};
    const int nxt = lane_gather(src, anc);
    if (anc > 0) {
      P = pa + qrot(qa, P);
      Qx = qmul(qa, Qx);
      anc = nxt;
    }
  }
  if (mine) {
    st3v(S.xpos[lane], P);
    st4v(S.xquat[lane], Qx);
  }
  WSYNC();
}

// One env's rows along a Newton direction: this lane's share of the cost decrease of the step al * s in the 1-D model, and the
// number of its rows whose sign the step changes.  With a = min(x, 0) the cost of a row is 1/2 D a^2 and its change
// 1/2 D (a1 - a0)(a1 + a0), where a1 - a0 is the step d itself while the row stays active: never a difference of squares (a step
// below the resolution of jar must yield a correctly tiny improvement, not an absorbed one).
// (the contact rows' share and the limit row's share are returned apart: where the problem separates by tree, the lane's contact
//  and its dof may belong to different trees; _c = the four pyramid rows of one contact, _l = the lane's joint-limit row)
__device__ __forceinline__ void step_rows_c(float al, const float (&jr)[4], const float (&vr)[4], float cD, float& pimc, float& crossc) {
  pimc = 0.0f;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const float x0 = jr[r], d = al * vr[r], x1 = x0 + d;
    const float a0 = fminf(x0, 0.0f), a1 = fminf(x1, 0.0f);
    pimc -= 0.5f * cD * ((x0 < 0.0f && x1 < 0.0f) ? d : a1 - a0) * (a1 + a0);
  }
  crossc = 0.0f;
#pragma unroll
  for (int r = 0; r < 4; r++) crossc += ((jr[r] < 0.0f) != (jr[r] + al * vr[r] < 0.0f)) ? 1.0f : 0.0f;
}
__device__ __forceinline__ void step_rows_l(float al, float ljar, float ljv, float lD, float lsg, float& piml, float& crossl) {
  {
    const float x0 = ljar, d = al * ljv, x1 = x0 + d;
    const float a0 = fminf(x0, 0.0f), a1 = fminf(x1, 0.0f);
    piml = -(0.5f * lD * ((x0 < 0.0f && x1 < 0.0f) ? d : a1 - a0) * (a1 + a0));
  }
  crossl = ((ljar < 0.0f) != (ljar + al * ljv < 0.0f)) && lsg != 0.0f ? 1.0f : 0.0f;
}

// ---------------------------------------------------------------------------------------------
// The step kernel.  VARIANT is a StepKind, FEAT a mask of FEAT_* bits, CPL = step_cpl(VARIANT): mir_step.h describes every kind and
// holds the table of their properties, from which the attributes below, the launch (launch_feat) and the body's switches come.
// One pass of the body as a device function: STEP_XR48's step loop (mir_step_kernel) calls it once per step of the call.  The other
// instantiations keep the body as the kernel's own (the same text, mir_step_body.inc), so that their code is what it was.
template <int VARIANT, int FEAT, int CPL = 1>
__device__ __attribute__((always_inline)) inline void mir_step_pass(StepArgs a) {
#include "mir_step_body.inc"
}

template <int VARIANT, int FEAT, int CPL = 1>
__global__ __launch_bounds__(step_block(VARIANT))
__attribute__((amdgpu_waves_per_eu(step_wpe_min(VARIANT), step_wpe_max(VARIANT)))) void mir_step_kernel(StepArgs a) {
  if constexpr (VARIANT == STEP_XR48) {
    // The STEP LOOP of the three-contacts-per-lane tier (mir_rollout_exact): workgroup g serves list entries 4g .. 4g + 3 (and leaves at
    // once when 4g is past the list's device count) through the steps of the call from the earliest start among them.  Every pass is
    // the whole step of one step index -- the env's state rows go through HBM between two passes, as between two launches, so a pass is
    // the single-step launch's arithmetic -- and an env takes the passes from its own start step until the end of the call or its
    // hand-off to the wave kernel (StepArgs::xr_*).  A pass in which no env of the workgroup has a step to take is skipped; once none
    // ever will, the workgroup leaves.  The two waves meet at a barrier between two passes (the LDS of one pass is the next one's).
    const int n = *a.xr_count;
    const int base = (int)blockIdx.x * EPB;
    if (base >= n) return;
    int ent[EPB];
#pragma unroll
    for (int g = 0; g < EPB; g++) ent[g] = base + g < n ? a.env_list[base + g] : -1;
    const long as = a.act_step, rs = a.rows_step;
    for (int s = 0; s < a.n_steps; s++) {
      bool take = false, later = false;  // (workgroup-uniform: every thread reads the same four words)
#pragma unroll
      for (int g = 0; g < EPB; g++) {
        if (ent[g] < 0) continue;
        const int st = __hip_atomic_load(&a.xr_start[ent[g]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        take = take || st <= s;
        later = later || (st > s && st < XR_TIER2);
      }
      if (!take && !later) return;
      if (!take) continue;
      StepArgs b = a;
      b.xr_step = s;
      b.action = a.action + (size_t)s * as;
      b.rows = a.rows + (size_t)s * rs;
      mir_step_pass<VARIANT, FEAT, CPL>(b);
      __syncthreads();
    }
  } else {
#include "mir_step_body.inc"
  }
}

}  // namespace

#if defined(MIR_STEP_CONVEX_TU) && !defined(MIR_STEP_PACKED_TU)
// debug aid: the lane-private convex narrowphase on n pairs given directly, one thread per pair.
//   in  (n, 22): type1, size1[3], pos1[3], quat1[4] (wxyz), type2, size2[3], pos2[3], quat2[4]
//   out (n, 8):  hit (0/1), pos[3], dist, normal[3]
namespace {
__global__ void k_debug_convex(const float* __restrict__ in, float* __restrict__ out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* r = in + (size_t)i * 22;
  const M3 R1 = q2m(qnormalize(Q4{r[7], r[8], r[9], r[10]})), R2 = q2m(qnormalize(Q4{r[18], r[19], r[20], r[21]}));
  const ShapeD A = {(int)r[0], v3(r[1], r[2], r[3]), v3(r[4], r[5], r[6]), mcol(R1, 0), mcol(R1, 1), mcol(R1, 2), nullptr, 0};
  const ShapeD B = {(int)r[11], v3(r[12], r[13], r[14]), v3(r[15], r[16], r[17]), mcol(R2, 0), mcol(R2, 1), mcol(R2, 2), nullptr, 0};
  f4 pt = {0, 0, 0, 0};
  V3 nrm = v3(0, 0, 0);
  const bool hit = convex_pair(A, B, pt, nrm);
  float* o = out + (size_t)i * 8;
  o[0] = hit ? 1.0f : 0.0f; o[1] = pt.x; o[2] = pt.y; o[3] = pt.z; o[4] = pt.w; o[5] = nrm.x; o[6] = nrm.y; o[7] = nrm.z;
}
}  // namespace
extern "C" int mir_launch_debug_convex(const float* in, float* out, int n, hipStream_t stream) {
  hipLaunchKernelGGL(k_debug_convex, dim3((n + 63) / 64), dim3(64), 0, stream, in, out, n);
  return (int)hipGetLastError();
}

#endif

// launcher used by the C ABI (mir_api.hip).  The instantiations with the convex narrowphase live in their own translation unit
// (mir_step_convex.hip = this file compiled with MIR_STEP_CONVEX_TU and WITHOUT -fno-signed-zeros: together with
// -ffp-contract=on that flag miscompiles the support-mapping selects of mir_convex.h -- box pairs lose contacts -- while the
// planes-and-boxes kernels gain 1 % from it).
// Each of the two sources is compiled twice, and every kind is instantiated in ONE of the two objects: the kinds of the contact-rich
// steps (step_packed, mir_step.h) in the MIR_STEP_PACKED_TU object, which is built with the SLP vectoriser on, all others in the
// object built with -fno-slp-vectorize (Makefile: STEP16FLAGS / STEP16PACKED).  The entry points below hand a kind to its object.
#ifdef MIR_STEP_PACKED_TU
constexpr bool kPackedTU = true;
#else
constexpr bool kPackedTU = false;
#endif
template <int KIND, int FEAT>
static int launch_kind(const StepArgs& a, int blocks, hipStream_t stream) {
  if constexpr (step_packed(KIND) == kPackedTU) {
    hipLaunchKernelGGL((mir_step_kernel<KIND, FEAT, step_cpl(KIND)>), dim3(blocks), dim3(step_block(KIND)), 0, stream, a);
    return (int)hipGetLastError();
  } else {
    return (int)hipErrorInvalidValue;  // (not instantiated in this object: the entry points never send it here)
  }
}
// THE dispatch: kind -> instantiation, for the FEAT mask of the caller's translation unit.  A kind that a mask does not carry is an
// error.  (STEP_POST has no collision code in it: one instantiation, FEAT_PLAIN, serves every scene; STEP_FULL stays generic.)
template <int FEAT>
static int launch_feat(const StepArgs& a, int kind, int blocks, hipStream_t stream) {
  switch (kind) {
    case STEP_POST: if constexpr (FEAT == FEAT_PLAIN) return launch_kind<STEP_POST, FEAT>(a, blocks, stream); else break;
    case STEP_PRE: return launch_kind<STEP_PRE, FEAT>(a, blocks, stream);
    case STEP_ROTATED: return launch_kind<STEP_ROTATED, FEAT>(a, blocks, stream);
    case STEP_LIST48: return launch_kind<STEP_LIST48, FEAT>(a, blocks, stream);
    case STEP_HEAVY48: return launch_kind<STEP_HEAVY48, FEAT>(a, blocks, stream);
    case STEP_POST48: return launch_kind<STEP_POST48, FEAT>(a, blocks, stream);
    case STEP_PRE48: return launch_kind<STEP_PRE48, FEAT>(a, blocks, stream);
    case STEP_ROTATED_LIST: return launch_kind<STEP_ROTATED_LIST, FEAT>(a, blocks, stream);
    case STEP_XR16: return launch_kind<STEP_XR16, FEAT>(a, blocks, stream);
    case STEP_XR48: return launch_kind<STEP_XR48, FEAT>(a, blocks, stream);
    case STEP_SINGLE: return launch_kind<STEP_SINGLE, FEAT>(a, blocks, stream);
    case STEP_LOOP: return launch_kind<STEP_LOOP, FEAT>(a, blocks, stream);
    case STEP_FULL: if constexpr ((FEAT & FEAT_SPEC) == 0) return launch_kind<STEP_FULL, FEAT>(a, blocks, stream); else break;
    case STEP_SENSE48: if constexpr ((FEAT & FEAT_SPEC) == 0) return launch_kind<STEP_SENSE48, FEAT>(a, blocks, stream); else break;  // (off the hot path: generic sizes)
  }
  return (int)hipErrorInvalidValue;
}
#ifdef MIR_STEP_CONVEX_TU
#ifdef MIR_STEP_PACKED_TU
extern "C" __attribute__((visibility("hidden"))) int mir_launch_step_convex_packed(const StepArgs* args, int kind, hipStream_t stream) {
  const StepArgs& a = *args;
#else
extern "C" __attribute__((visibility("hidden"))) int mir_launch_step_convex_packed(const StepArgs* args, int kind, hipStream_t stream);
extern "C" __attribute__((visibility("hidden"))) int mir_launch_step_convex(const StepArgs* args, int kind, hipStream_t stream) {
  const StepArgs& a = *args;
  if (step_packed(kind)) return mir_launch_step_convex_packed(args, kind, stream);
#endif
  const int blocks = (a.B + EPB - 1) / EPB;
  // the headline scene's instantiation (FEAT_SPEC: mir_create found SpecPick::matches); the everything-variant stays generic
  if ((a.features & FEAT_SPEC) && kind != STEP_FULL && kind != STEP_SENSE48) return launch_feat<FEAT_CONVEX | FEAT_SPEC>(a, kind, blocks, stream);
  if (a.features & FEAT_SAP) return launch_feat<FEAT_CONVEX | FEAT_SAP>(a, kind, blocks, stream);  // sweep-and-prune scenes carry the convex code too
  return launch_feat<FEAT_CONVEX>(a, kind, blocks, stream);
}
#elif defined(MIR_STEP_PACKED_TU)
extern "C" __attribute__((visibility("hidden"))) int mir_launch_step_plain_packed(const StepArgs* args, int kind, hipStream_t stream) {
  return launch_feat<FEAT_PLAIN>(*args, kind, (args->B + EPB - 1) / EPB, stream);
}
#else
extern "C" __attribute__((visibility("hidden"))) int mir_launch_step_convex(const StepArgs* args, int kind, hipStream_t stream);
extern "C" __attribute__((visibility("hidden"))) int mir_launch_step_plain_packed(const StepArgs* args, int kind, hipStream_t stream);
extern "C" int mir_launch_step(const StepArgs* args, hipStream_t stream) {
  const StepArgs& a = *args;
  const int blocks = (a.B + EPB - 1) / EPB;
  // a whole step (STEP_FULL asked for) takes the leanest instantiation that has everything the arguments use
  int kind = a.kind;
  if (kind == STEP_FULL) {
#ifdef MIR_PROFILE_SINGLE
    const bool prof_blocks_single = false;
#else
    const bool prof_blocks_single = a.prof != nullptr;
#endif
    const bool single = a.mode == 0 && a.n_steps == 1 && !a.act_step && !a.rows_step && !a.ar.episode_len && !prof_blocks_single && !a.out_M && !a.out_bias &&
                        !a.out_qas && !a.out_qacc && !a.out_xpos && !a.out_xquat;
    const bool plain_loop = a.mode == 0 && !a.prof && !a.out_M && !a.out_bias && !a.out_qas && !a.out_qacc && !a.out_xpos && !a.out_xquat && !a.agent_pos &&
                            !a.env_state && !a.reward && !a.terminated && !a.term_host && !a.done_ticket;
    kind = single ? STEP_SINGLE : (plain_loop ? STEP_LOOP : STEP_FULL);
  }
  if (a.features && !step_post_only(kind)) return mir_launch_step_convex(&a, kind, stream);
  if (step_packed(kind)) return mir_launch_step_plain_packed(&a, kind, stream);
  return launch_feat<FEAT_PLAIN>(a, kind, blocks, stream);
}
#endif
