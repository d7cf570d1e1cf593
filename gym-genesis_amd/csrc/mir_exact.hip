// mir_exact.hip — EXACT CONTACTS on the host side: the switch (mir_set_exact_contacts), the launches and waits that complete a step for
// its deferred envs (split_lists, exact_finish; called by mir_step_begin / mir_step_end in mir_api.hip), the counters, and the
// device-resident rollout that keeps every contact point.  WHICH route a step takes is decided in mir_route.h.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "mir_host.h"
#include "mir_step64.h"

using namespace mir_host;

/* A step of an overflow run whose predecessor's first-half launch has said which envs are above the one-contact-per-lane capacity NOW
 * (x.res.next_host, tagged x.phase.rt_tag, in the order of perm_host[x.phase.rt_perm]): the order of this step's launches -- those envs first, padded to
 * whole workgroups with others, then the rest -- into perm_host[*buf]; *nh = how many go to the three-contacts-per-lane list. */
int mir_host::split_lists(MirScene* h, int* buf, int* nh_out) {
  ExactRoute& x = h->xc;
  const size_t B = (size_t)h->B, nwg = (B + 3) / 4;
  const uint32_t want4 = 0x01010101u * (uint8_t)x.phase.rt_tag, tagm4 = 0x1f1f1f1fu;
  const int32_t* const pp = x.phase.rt_perm >= 0 ? x.res.perm_host[x.phase.rt_perm] : nullptr;
  const volatile uint32_t* w = x.res.next_host;
  // (straight into the pinned order, word by word as they arrive: the envs above the capacity from the front, the others from the back)
  const int nxt = x.phase.rt_perm == 0 ? 1 : 0;
  int32_t* const out = x.res.perm_host[nxt];
  size_t nh = 0, lo = B, g = 0;
  int rc = spin_until(h, x.res.ovf_stream, "mir_step_begin: side stream (exact contacts)",
                      "mir_step_begin: the first-half launch finished without saying which envs are above 16 points", true, [&]() {
    for (; g < nwg; g++) {
      const uint32_t v = w[g];
      if (((v >> 1) & tagm4) != want4) return false;
      partition_word(v, g, pp, B, 1u, out, nh, lo);
    }
    return true;
  });
  if (rc != MIR_OK) return rc;
  // (whole workgroups: the first of the others join the list of the bigger instantiation, which steps an env with few contacts to the same
  //  bits -- they sit right behind it in the array already)
  while ((nh & 3) && nh < B) nh++;
  __atomic_thread_fence(__ATOMIC_RELEASE);
  *buf = nxt;
  *nh_out = (int)nh;
  return MIR_OK;
}

/* exact contacts: the n envs of ovf_list_host were deferred by the launch(es) of the pending mir_step_begin (their state rows are
 * those of the step's start).  They are stepped here by the LIST INSTANTIATION of the 16-lane kernel (STEP_LIST48, mir_step.h: three
 * contacts per lane, 48 points, four envs per workgroup) -- one launch that takes the action and the output pointers of the pending
 * step, stores state, observations and the terminated byte of list entry k into ovf_term_host[k], and then writes the envs' scratch
 * rows for the NEXT step (which also say whether they are deferred again).  An env beyond THAT kernel's capacity (more than 48 points,
 * or more than 16 candidate pairs: its byte comes back with bit 7 set, nothing stored) goes on a second list and takes the route every
 * deferred env of a scene without the list instantiation takes: the wave-per-env kernel in list mode (the same scene compiled for it,
 * 64 candidates, reading and writing the 16-lane kernel's rows) followed by the action-independent half of the 16-lane kernel over that list.  MIR_EXACT_WAVE=1
 * (read by mir_set_exact_contacts), or a scene without the split closing FK, sends every deferred env that way.
 * The launches go on a stream of the library's own, BESIDE the launch that deferred these envs (which is still running its second
 * half: the host is here because that launch's terminated bytes -- early bytes -- have arrived): that launch stores nothing for
 * them, and everything queued before it on the step's stream has finished, or it would not be running.  The step's stream then
 * waits for an event recorded behind them, so that whatever the caller queues after mir_step_end -- the next step, a
 * policy network reading the observations -- comes after them. */
static int exact_wait(MirScene* h, const uint8_t* term, const int32_t* list, int n, uint8_t* terminated_host, int32_t* again, int* n_again) {
  const uint8_t want = (uint8_t)h->tag;
  int k = 0;
  return spin_until(h, h->pending_stream, "mir_step_end: stream (exact contacts)",
                    "mir_step_end: the launch for the deferred envs finished without delivering its terminated bytes", true, [&]() {
    for (; k < n; k++) {
      const uint8_t b = __atomic_load_n(term + k, __ATOMIC_RELAXED);
      if ((uint8_t)((b >> 1) & 0x1fu) != want) return false;
      if ((b & 0x80u) && again) again[(*n_again)++] = list[k];
      else if (terminated_host) terminated_host[list[k]] = b & 1u;
    }
    return true;
  });
}

int mir_host::exact_finish(MirScene* h, int n, uint8_t* terminated_host) {
  ExactRoute& x = h->xc;
  DeviceGuard guard(h->device);
  // (not beside a step that was launched as two kernels -- a fused launch, or the second half alone, followed by the first half of the
  //  next step for ALL envs: that second kernel writes the scratch rows of the deferred envs too, from their old state, and must come
  //  BEFORE the one below that writes them from the new state: stream order does that)
  void* const side = (x.res.ovf_stream && (x.pend.rotated || x.pend.big)) ? x.res.ovf_stream : h->pending_stream;  // (pend_big: behind the first-half launch, which is there)
  const size_t B = (size_t)h->B;
  int32_t* const list2_host = reinterpret_cast<int32_t*>(x.res.ovf_term_host + (B + 63) / 64 * 64);
  int32_t* const list2_dev = reinterpret_cast<int32_t*>(x.res.ovf_term_dev + (B + 63) / 64 * 64);
  uint8_t* const term2_host = reinterpret_cast<uint8_t*>(list2_host + B);
  uint8_t* const term2_dev = reinterpret_cast<uint8_t*>(list2_dev + B);
  const int32_t* wlist_host = x.res.ovf_list_host;
  const int32_t* wlist_dev = x.res.ovf_list_dev;
  const uint8_t* wterm_host = x.res.ovf_term_host;
  uint8_t* wterm_dev = x.res.ovf_term_dev;
  int nw = n;  // envs for the wave-per-env kernel
  // (the envs a heavy step defers were beyond the three-contacts-per-lane capacity already: straight to the wave-per-env kernel.  Those
  //  of a two-launch step are envs whose big row the launch before could not write: the list launch like those of a light step)
  if (!x.pend.heavy && x.cfg.exact_big) {
    memset(x.res.ovf_term_host, 0, (size_t)n);  // (tags come round every 31 steps: a byte of an older step must not pass for this one's)
    __atomic_thread_fence(__ATOMIC_RELEASE);
    Outs o;
    o.action = x.pend.action;
    o.agent_pos = (float*)x.pend.out[0]; o.env_state = (float*)x.pend.out[1]; o.reward = (float*)x.pend.out[2]; o.terminated = (uint8_t*)x.pend.out[3];
    o.term_host = x.res.ovf_term_dev; o.term_tag = h->tag;
    o.kind = STEP_LIST48; o.env_list = x.res.ovf_list_dev; o.nlist = n;
    o.prof = h->dbg_prof_list;
    h->dbg_prof_list = nullptr;
    int rc = launch(h, o, side);
    if (rc != MIR_OK) return rc;
    x.stats.big_envs += (unsigned long long)n;
    nw = 0;
    rc = exact_wait(h, x.res.ovf_term_host, x.res.ovf_list_host, n, terminated_host, list2_host, &nw);
    if (rc != MIR_OK) return rc;
    wlist_host = list2_host; wlist_dev = list2_dev; wterm_host = term2_host; wterm_dev = term2_dev;
  }
  if (nw) {
    memset(const_cast<uint8_t*>(wterm_host), 0, (size_t)nw);
    __atomic_thread_fence(__ATOMIC_RELEASE);
    StepArgs64 a;
    memset(&a, 0, sizeof a);
    a.model = h->dm64;
    a.qpos = h->qpos; a.qvel = h->qvel; a.target = h->target; a.qacc_ws = h->qacc_ws;
    a.diag = h->diag_on ? h->diag : nullptr;
    a.bad_count = h->early_stats;
    a.B = nw; a.nu = h->hm64.nu; a.convex = h->hm64.has_convex;
    a.action = x.pend.action;
    a.agent_pos = (float*)x.pend.out[0]; a.env_state = (float*)x.pend.out[1]; a.reward = (float*)x.pend.out[2]; a.terminated = (uint8_t*)x.pend.out[3];
    a.term_host = wterm_dev; a.term_tag = h->tag;
    a.mode = 0; a.n_steps = 1;
    a.env_list = wlist_dev; a.lay16_qst = h->hm.qstride;
    x.stats.wave_envs += (unsigned long long)nw;
    int rc = mir_launch_step64(&a, (hipStream_t)side);
    if (rc != 0) return hip_fail((hipError_t)rc, "wave kernel launch (exact contacts)");
    h->poses_current = 0;  // (these envs' link poses were not written)
    if (h->pre_valid) {  // (split step: the scratch rows of the coming step, for the envs that have only now reached its starting state)
      Outs p;
      p.kind = STEP_PRE; p.diag = false; p.env_list = wlist_dev; p.nlist = nw;
      rc = launch(h, p, side);
      if (rc != MIR_OK) return rc;
    }
  }
  if (side != h->pending_stream) {
    HIPCHK(hipEventRecord((hipEvent_t)x.res.ovf_event, (hipStream_t)side));
    HIPCHK(hipStreamWaitEvent((hipStream_t)h->pending_stream, (hipEvent_t)x.res.ovf_event, 0));
    x.res.ovf_event_live = 1;
    x.res.ovf_waited_stream = h->pending_stream;
  }
  if (nw) return exact_wait(h, wterm_host, wlist_host, nw, terminated_host, nullptr, nullptr);
  return MIR_OK;
}

void mir_host::exact_destroy(MirScene* h) {  // (mir_destroy, under its device guard)
  ExactRes& r = h->xc.res;
  if (r.pre_big) (void)hipFree(r.pre_big);
  if (r.xr_stats) (void)hipFree(r.xr_stats);
  if (r.main_event) (void)hipEventDestroy((hipEvent_t)r.main_event);
  if (r.light_event) (void)hipEventDestroy((hipEvent_t)r.light_event);
  if (r.next_host) (void)hipHostFree(r.next_host);
  if (r.ovf_list_host) (void)hipHostFree(r.ovf_list_host);
  if (r.ovf_event) (void)hipEventDestroy((hipEvent_t)r.ovf_event);
  if (r.ovf_stream) (void)hipStreamDestroy((hipStream_t)r.ovf_stream);
}

extern "C" {

int mir_set_exact_contacts(MirHandle h, const MirSceneSpec* spec, int32_t on) {
  if (check(h)) return MIR_E_INVALID;
  ExactRoute& x = h->xc;
  if (h->pending) return set_err(MIR_E_INVALID, "mir_set_exact_contacts: a step is pending");
  // (a scratch row whose head says "above 16 points, the contacts are elsewhere" means something to the launches of this mode only: the
  //  next step starts from the state, not from the rows)
  h->pre_valid = 0;
  x.phase.bigmode = 0;
  if (!on) { x.on = 0; return MIR_OK; }
  if (h->kernel != 16) return set_err(MIR_E_INVALID, "mir_set_exact_contacts: the scene already runs on the wave-per-env kernel (48 contact points, never thinned below that)");
  if (h->sync_mode != 3 || !h->term_wstride) return set_err(MIR_E_INVALID, "mir_set_exact_contacts: needs the tagged terminated bytes (sync mode 3)");
  if (!spec) return set_err(MIR_E_INVALID, "mir_set_exact_contacts: the scene's spec is needed once (it is compiled for the wave kernel)");
  if (!x.res.ovf_list_host) {
    // the same scene for the wave-per-env kernel, with that kernel's contact capacity
    MirSceneSpec* s2 = new (std::nothrow) MirSceneSpec(*spec);
    if (!s2) return set_err(MIR_E_INVALID, "out of host memory");
    s2->opt.max_contacts = MIR_MAX_CONTACT;
    HostConsts hc;
    char err[256] = "";
    const int rc = mir_compile_model64(s2, &h->hm64, &hc, err);
    delete s2;
    if (rc != MIR_OK) return set_err(rc, "mir_set_exact_contacts: %s", err);
    if (h->hm64.nv != h->hm.nv || h->hm64.nq != h->hm.nq || h->hm64.nu != h->hm.nu || h->hm64.agent_dim != h->agent_dim || h->hm64.env_dim != h->env_dim)
      return set_err(MIR_E_INVALID, "mir_set_exact_contacts: the spec is not the one this scene was created from");
    DeviceGuard guard(h->device);
    HIPCHK(hipMemcpy(h->dm64, &h->hm64, sizeof(DevModel64), hipMemcpyHostToDevice));
    // [list of the deferred envs (B x i32) | their terminated bytes (B, padded to 64)] twice: the envs the list instantiation could not
    // hold either go on the second list (exact_finish)
    // ... and two permutations of the envs for the launches of a heavy phase (B x i32 each, see mir_step_end)
    const size_t B = (size_t)h->B, bytes = 2 * (B * sizeof(int32_t) + ((B + 63) / 64) * 64) + 2 * ((B + 15) / 16 * 16) * sizeof(int32_t);
    HIPCHK(hipHostMalloc((void**)&x.res.ovf_list_host, bytes, hipHostMallocMapped | hipHostMallocCoherent));
    memset(x.res.ovf_list_host, 0, bytes);
    HIPCHK(hipHostGetDevicePointer((void**)&x.res.ovf_list_dev, x.res.ovf_list_host, 0));
    x.res.ovf_term_host = reinterpret_cast<uint8_t*>(x.res.ovf_list_host + B);
    x.res.ovf_term_dev = reinterpret_cast<uint8_t*>(x.res.ovf_list_dev + B);
    {
      const size_t half = B * sizeof(int32_t) + ((B + 63) / 64) * 64, pn = (B + 15) / 16 * 16;
      for (int i = 0; i < 2; i++) {
        x.res.perm_host[i] = reinterpret_cast<int32_t*>(reinterpret_cast<uint8_t*>(x.res.ovf_list_host) + 2 * half) + i * pn;
        x.res.perm_dev[i] = reinterpret_cast<int32_t*>(reinterpret_cast<uint8_t*>(x.res.ovf_list_dev) + 2 * half) + i * pn;
      }
      x.phase.perm_next = -1; x.pend.perm = -1;
    }
    if (!getenv("MIR_EXACT_ONE_STREAM")) {  // (the side stream of exact_finish; MIR_EXACT_ONE_STREAM=1: everything on the step's stream)
      int lo = 0, hi = 0;
      (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
      hipStream_t st = nullptr;
      hipEvent_t ev = nullptr;
      HIPCHK(hipStreamCreateWithPriority(&st, hipStreamNonBlocking, hi));
      HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
      x.res.ovf_stream = st; x.res.ovf_event = ev;
    }
  }
  // the list instantiation of the 16-lane kernel takes the deferred envs where the scene has the split closing forward kinematics (every
  // free body a childless child of the world: the reference's scenes); MIR_EXACT_WAVE=1: the wave-per-env kernel takes them all
  x.cfg.exact_big = (h->hm.fk_free_leaf != 0 && !(getenv("MIR_EXACT_WAVE") && atoi(getenv("MIR_EXACT_WAVE")) != 0)) ? 1 : 0;
  // (1, the default: when the caller spent at least MIR_EXACT_BIG_GAP microseconds -- 40 -- between the last mir_step_end and this
  //  mir_step_begin: the two launches of such a step take a third more GPU time than the heavy phase's one -- rows through HBM, less
  //  overlap of the two waves -- which a loop with nothing between its steps pays in full; 2: whenever the rows are there; 0: never)
  x.cfg.big_on = (x.cfg.exact_big && on != 2 && x.res.ovf_stream) ? (getenv("MIR_EXACT_BIG") ? atoi(getenv("MIR_EXACT_BIG")) : 1) : 0;
  x.cfg.big_gap_us = getenv("MIR_EXACT_BIG_GAP") ? atof(getenv("MIR_EXACT_BIG_GAP")) : 40.0;
  x.cfg.big_lists = !(getenv("MIR_EXACT_BIG_LISTS") && atoi(getenv("MIR_EXACT_BIG_LISTS")) == 0);  // (0: the second half always as one launch for the whole batch)
  x.cfg.big_side = !(getenv("MIR_EXACT_BIG_SIDE") && atoi(getenv("MIR_EXACT_BIG_SIDE")) == 0);  // (0, a test switch: the first-half launch on the step's stream)
  x.phase.t_end_us = 0.0;
  x.phase.bigmode = 0;
  if (x.cfg.big_on && !x.res.main_event) {
    DeviceGuard guard(h->device);
    hipEvent_t ev = nullptr, ev2 = nullptr;
    HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&ev2, hipEventDisableTiming));
    x.res.main_event = ev; x.res.light_event = ev2;
    const size_t nb = (((size_t)h->B + 3) / 4 * sizeof(uint32_t) + 63) / 64 * 64;
    HIPCHK(hipHostMalloc((void**)&x.res.next_host, nb, hipHostMallocMapped | hipHostMallocCoherent));
    memset(x.res.next_host, 0, nb);
    HIPCHK(hipHostGetDevicePointer((void**)&x.res.next_dev, x.res.next_host, 0));
  }
  x.phase.rt_ok = 0;
  if (!x.res.xr_stats) {  // (mir_rollout_exact's lists and counters: see mir_scene.h)
    DeviceGuard guard(h->device);
    const size_t B = (size_t)h->B, bytes = 4 * sizeof(unsigned long long) + 16 * sizeof(int32_t) + 3 * B * sizeof(int32_t);
    HIPCHK(hipMalloc((void**)&x.res.xr_stats, bytes));
    HIPCHK(hipMemset(x.res.xr_stats, 0, bytes));
    x.res.xr_count = reinterpret_cast<int32_t*>(x.res.xr_stats + 4);
    x.res.xr_list = x.res.xr_count + 16;
    x.res.xr_list2 = x.res.xr_list + B;
    x.res.xr_start = x.res.xr_list2 + B;
  }
  if (x.cfg.big_on && !x.res.pre_big) {
    DeviceGuard guard(h->device);
    HIPCHK(hipMalloc((void**)&x.res.pre_big, (size_t)h->B * K48_STRIDE * sizeof(float)));
    HIPCHK(hipMemset(x.res.pre_big, 0, (size_t)h->B * K48_STRIDE * sizeof(float)));
  }
  x.on = on == 2 ? 2 : 1;
  x.phase.heavy = 0;
  x.phase.perm_next = -1; x.pend.perm = -1;
  x.cfg.heavy_sort = !(getenv("MIR_EXACT_HEAVY_SORT") && atoi(getenv("MIR_EXACT_HEAVY_SORT")) == 0);
  x.cfg.heavy_enter = (h->B + 15) / 16; x.cfg.heavy_leave = (h->B + 31) / 32;  // (6 % / 3 % of the batch)
  if (const char* e = getenv("MIR_EXACT_HEAVY")) {
    int a = 0, b = 0;
    const int k = sscanf(e, "%d,%d", &a, &b);
    if (k >= 1) { x.cfg.heavy_enter = a; x.cfg.heavy_leave = k >= 2 ? b : a / 2; }
  }
  if (on == 2) x.cfg.heavy_enter = 0;  // (the twin of the tests: every env on the list instantiation, every step)
  return MIR_OK;
}

int mir_get_exact_contacts(MirHandle h) { return check(h) ? MIR_E_INVALID : h->xc.on; }

int mir_get_exact_stats(MirHandle h, uint64_t* out4, int32_t reset) {
  if (check(h) || !out4) return set_err(MIR_E_INVALID, "mir_get_exact_stats: null argument");
  ExactStats& st = h->xc.stats;
  out4[0] = st.steps; out4[1] = st.ovf_steps; out4[2] = st.ovf_envs; out4[3] = st.ovf_max;
  if (reset) st = ExactStats{};  // (the route counters of mir_get_exact_route too)
  return MIR_OK;
}

int mir_get_exact_route(MirHandle h, uint64_t* out4) {
  if (check(h) || !out4) return set_err(MIR_E_INVALID, "mir_get_exact_route: null argument");
  const ExactStats& st = h->xc.stats;
  out4[0] = st.big_envs; out4[1] = st.wave_envs; out4[2] = st.heavy_steps; out4[3] = st.big_steps;
  return MIR_OK;
}

}  // extern "C"

/* Device-resident K-step rollout that keeps every contact point (mirigid.h: mir_rollout_exact).  A fixed chain on the caller's stream:
 *   memset of the two list counters;
 *   the one-wave step loop with hand-off (STEP_XR16) for the whole batch -- an env stays on it until its first step above the
 *     one-contact-per-lane capacity, then stores its state of that step's start and appends itself to list 1 (exact == 2: every env at
 *     step 0, the twin route of the tests);
 *   the three-contacts-per-lane step loop (STEP_XR48) over list 1 -- fixed grid, a workgroup past the list's device count exits at
 *     once -- each env from its own start step to the end of the call, which hands an env beyond 48 points or 16 candidate pairs on to
 *     list 2 (scenes whose host-closed route has no list instantiation: list 1 is list 2);
 *   the wave-per-env kernel in list mode over list 2, each env resuming at its own step (the 16-lane layout in and out);
 *   a one-thread kernel that folds list 1's count into the statistics.
 * No host read, no pinned memory, no host wait.  Every kernel of the chain runs the same step body as the route of mir_step_begin /
 * mir_step_end, so the bits are that route's (see mirigid.h for the one exception). */
__global__ void k_xr_close(const int32_t* count, unsigned long long* stats) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const unsigned long long n = (unsigned long long)count[0];
    if (n > stats[2]) stats[2] = n;
  }
}

static int rollout_exact(MirScene* h, const float* actions, int32_t n_steps, float* rows, int32_t row_stride, const AutoResetArgs& ar, void* stream, const char* who) {
  ExactRoute& x = h->xc;
  if (h->pending) {  // (a step left open: closed first, as mir_reset does)
    int rc = mir_step_end(h, nullptr);
    if (rc != MIR_OK) return rc;
  }
  if (int rc = check_mask(h)) return rc;
  if (!x.res.xr_stats) return set_err(MIR_E_INVALID, "%s: exact contacts were never switched on", who);
  if (n_steps >= XR_TIER2) return set_err(MIR_E_INVALID, "%s: n_steps must be below 2^20", who);
  DeviceGuard guard(h->device);
  // (the side-stream launches of an earlier host-closed overflow step own the state and the scratch rows until ovf_event: mir_step_begin)
  if (x.res.ovf_event_live && x.res.ovf_waited_stream != stream) {
    HIPCHK(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)x.res.ovf_event, 0));
    x.res.ovf_waited_stream = stream;
  }
  h->pre_valid = 0;
  h->poses_current = 0;
  h->state_version++;
  x.res.xr_calls++;
  const hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipMemsetAsync(x.res.xr_count, 0, 2 * sizeof(int32_t), st));
  StepArgs a;
  memset(&a, 0, sizeof a);
  a.model = h->dm;
  a.qpos = h->qpos; a.qvel = h->qvel; a.target = h->target; a.qacc_ws = h->qacc_ws;
  a.diag = h->diag_on ? h->diag : nullptr;
  a.early_stats = h->early_stats; a.no_early_mask = 1;
  a.term_wstride = h->term_wstride;
  a.B = h->B; a.qst = h->hm.qstride; a.nu = h->hm.nu;
  a.features = (h->hm.has_convex ? FEAT_CONVEX : 0) | (h->hm.use_sap ? FEAT_CONVEX | FEAT_SAP : 0) | (h->spec_pick ? FEAT_SPEC : 0);
  a.row_stride = row_stride; a.mode = 0;
  a.ar = ar;
  a.exact = x.on;
  // (without the list instantiation the hand-off of (1) goes to list 2 directly: the step index it records carries no tier bit, which
  //  only STEP_XR48 reads)
  a.xr_list = x.cfg.exact_big ? x.res.xr_list : x.res.xr_list2; a.xr_count = x.cfg.exact_big ? x.res.xr_count : x.res.xr_count + 1;
  a.xr_list2 = x.res.xr_list2; a.xr_count2 = x.res.xr_count + 1;
  a.xr_start = x.res.xr_start; a.xr_stats = x.res.xr_stats;
  const long as = (long)h->B * h->nu, rs = (long)h->B * row_stride;
  // (1) the whole batch on the one-wave step loop, every env until its hand-off
  a.kind = STEP_XR16; a.action = actions; a.rows = rows; a.n_steps = n_steps; a.act_step = as; a.rows_step = rs;
  int rc = mir_launch_step(&a, st);
  if (rc != 0) return hip_fail((hipError_t)rc, who);
  // (2) list 1 on the three-contacts-per-lane step loop, each env from its own step (scenes whose host-closed route sends the deferred
  //     envs to the wave-per-env kernel instead -- no split closing FK, or MIR_EXACT_WAVE -- hand them straight to list 2 in (1))
  if (x.cfg.exact_big) {
    a.kind = STEP_XR48; a.env_list = x.res.xr_list; a.n_steps = n_steps; a.action = actions; a.rows = rows; a.act_step = as; a.rows_step = rs;
    rc = mir_launch_step(&a, st);
    if (rc != 0) return hip_fail((hipError_t)rc, who);
  }
  // (3) list 2 on the wave-per-env kernel, each env from its own step to the end of the call
  StepArgs64 w;
  memset(&w, 0, sizeof w);
  w.model = h->dm64;
  w.qpos = h->qpos; w.qvel = h->qvel; w.target = h->target; w.qacc_ws = h->qacc_ws;
  w.diag = h->diag_on ? h->diag : nullptr;
  w.bad_count = h->early_stats;
  w.B = h->B; w.nu = h->hm64.nu; w.convex = h->hm64.has_convex;
  w.action = actions; w.rows = rows; w.row_stride = row_stride; w.act_step = as; w.rows_step = rs; w.ar = ar;
  w.mode = 0; w.n_steps = n_steps;
  w.env_list = x.res.xr_list2; w.lay16_qst = h->hm.qstride;
  w.list_count = x.res.xr_count + 1; w.env_start = x.res.xr_start; w.xr_stats = x.res.xr_stats;
  rc = mir_launch_step64(&w, st);
  if (rc != 0) return hip_fail((hipError_t)rc, who);
  hipLaunchKernelGGL(k_xr_close, dim3(1), dim3(64), 0, st, x.res.xr_count, x.res.xr_stats);
  HIPCHK(hipGetLastError());
  return MIR_OK;
}

extern "C" {

int mir_rollout_exact(MirHandle h, const float* actions, int32_t n_steps, float* rows, int32_t row_stride, void* stream) {
  if (check(h) || !actions || !rows) return set_err(MIR_E_INVALID, "mir_rollout_exact: null argument");
  if (h->kernel != 16) return set_err(MIR_E_INVALID, "mir_rollout_exact: the scene runs on the wave-per-env kernel (48 points, nothing to switch): use mir_rollout");
  if (row_stride < h->agent_dim + h->env_dim + 2) return set_err(MIR_E_INVALID, "mir_rollout_exact: row_stride too small");
  if (!h->xc.on) return mir_rollout(h, actions, n_steps, rows, row_stride, stream);
  if (n_steps <= 0) return MIR_OK;
  return rollout_exact(h, actions, n_steps, rows, row_stride, AutoResetArgs{nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0}, stream, "mir_rollout_exact");
}

int mir_rollout_autoreset_exact(MirHandle h, const float* actions, int32_t n_steps, float* rows, int32_t row_stride, int32_t* episode_len,
                                int32_t max_len, const float* spawn_pool, int32_t pool_len, int32_t* cursor, const float* obj_quat,
                                const float* arm_qpos, void* stream) {
  if (check(h) || !actions || !rows) return set_err(MIR_E_INVALID, "mir_rollout_autoreset_exact: null argument");
  if (!episode_len || !spawn_pool || !cursor || !obj_quat || !arm_qpos || pool_len <= 0) return set_err(MIR_E_INVALID, "mir_rollout_autoreset_exact: null argument");
  if (h->kernel != 16) return set_err(MIR_E_INVALID, "mir_rollout_autoreset_exact: the scene runs on the wave-per-env kernel (48 points, nothing to switch): use mir_rollout_autoreset");
  if (row_stride < h->agent_dim + h->env_dim + 3) return set_err(MIR_E_INVALID, "mir_rollout_autoreset_exact: row_stride too small (needs the truncated column)");
  if (!h->xc.on) return mir_rollout_autoreset(h, actions, n_steps, rows, row_stride, episode_len, max_len, spawn_pool, pool_len, cursor, obj_quat, arm_qpos, stream);
  if (n_steps <= 0) return MIR_OK;
  return rollout_exact(h, actions, n_steps, rows, row_stride, AutoResetArgs{episode_len, cursor, spawn_pool, obj_quat, arm_qpos, pool_len, max_len}, stream,
                       "mir_rollout_autoreset_exact");
}

int mir_get_rollout_exact_stats(MirHandle h, uint64_t* out4, int32_t reset) {
  if (check(h) || !out4) return set_err(MIR_E_INVALID, "mir_get_rollout_exact_stats: null argument");
  ExactRes& x = h->xc.res;
  unsigned long long dev[4] = {0, 0, 0, 0};
  if (x.xr_stats) {  // (synchronises the device: the counters are written by the launches)
    DeviceGuard guard(h->device);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(dev, x.xr_stats, sizeof dev, hipMemcpyDeviceToHost));
    if (reset) HIPCHK(hipMemset(x.xr_stats, 0, sizeof dev));
  }
  out4[0] = x.xr_calls; out4[1] = dev[0]; out4[2] = dev[1]; out4[3] = dev[2];
  if (reset) x.xr_calls = 0;
  return MIR_OK;
}

}  // extern "C"
