"""Device-resident rollouts that keep every contact point (mir_rollout_exact / mir_rollout_autoreset_exact).

Each test compares the new entry points with the host-closed route they must reproduce bit for bit: K x (step_begin; step_end) with
exact contacts on (and mir_autoreset behind each step for the episode loop), or, with the switch off, mir_rollout itself."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

from gym_genesis.backend import models
from gym_genesis.backend.lib import MirError, MirScene

pytestmark = pytest.mark.gpu

HOME = np.array(models.FRANKA_HOME, dtype=np.float32)
RS = 9 + 11 + 3  # [agent | env_state | reward | terminated | truncated]


def _scene(n, exact=None):
    sc = MirScene(models.franka_cube_pick_scene().build(), n)
    if exact is not None:
        sc.set_exact_contacts(exact)
    return sc


def _bufs(sc):
    return (sc.empty(sc.agent_dim), sc.empty(sc.env_dim), sc.empty(), sc.empty(dtype=torch.uint8))


def _row_of(bufs):
    a, e, r, t = bufs
    return torch.cat([a, e, r[:, None], t[:, None].float()], 1)


DIST = 9 + 10  # the row's eef - cube distance column


def _assert_rows(got, want, what, dist=DIST):
    """A packed row against the host-closed step's outputs: bit for bit, but for the distance column, where the packed-row and the
    observation outputs of the same step kernel differ by up to one ulp with exact contacts off too (mir_rollout against step_fused:
    test_rows_and_observations_of_the_same_steps_without_the_switch pins that)."""
    keep = torch.ones(got.shape[-1], dtype=torch.bool, device=got.device)
    keep[dist] = False
    assert torch.equal(got[:, keep], want[:, keep]), what
    g, w = got[:, dist], want[:, dist]
    inf = torch.full_like(w, float("inf"))
    assert bool(((g == w) | (g == torch.nextafter(w, inf)) | (g == torch.nextafter(w, -inf))).all()), what


def _grasp(n, seed=5):
    """tests/golden/grasp_targets.json tiled to n envs, cubes moved by up to 2 mm (as the exact-contact tests do)"""
    G_ = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "grasp_targets.json")))
    T = np.array(G_["targets"], np.float32)
    pos4 = np.array([[x, y, 0.02] for x, y in G_["cube_xy"]], np.float32)
    acts4 = np.repeat(T.transpose(1, 0, 2), G_["steps_per_stage"], axis=0)
    pos = np.tile(pos4, (n // 4, 1))
    pos[:, :2] += np.random.default_rng(seed).uniform(-0.002, 0.002, (n, 2)).astype(np.float32)
    return pos, np.tile(acts4, (1, n // 4, 1))


def _reset(scs, pos):
    n = pos.shape[0]
    quat, arm = np.tile(np.array([0, 0, 0, 1], np.float32), (n, 1)), np.tile(HOME, (n, 1))
    for s in scs:
        s.reset(pos, quat, arm)


def _same_state(a, b):
    return all(torch.equal(x, y) for x, y in zip(a.get_state(), b.get_state()))


def _calls(T, K):
    t = 0
    while t < T:
        k = min(K, T - t)
        yield t, k
        t += k


def test_without_overflow_equals_the_thinned_rollout():
    """Random actions, 4096 envs: no env goes above 16 points, so rollout_exact (switch on) is mir_rollout (switch off) bit for bit,
    and nothing is handed off."""
    n = 4096
    a, b = _scene(n, True), _scene(n)
    rng = np.random.default_rng(0)
    _reset((a, b), np.stack([rng.uniform(0.45, 0.8, n), rng.uniform(-0.25, 0.25, n), np.full(n, 0.02)], 1).astype(np.float32))
    a.rollout_exact_stats(reset=True)
    acts = torch.as_tensor(rng.uniform(-1, 1, (64, n, 9)).astype(np.float32), device=a.device)
    ra, rb = torch.zeros((16, n, RS - 1), device=a.device), torch.zeros((16, n, RS - 1), device=a.device)
    for t in range(0, 64, 16):
        a.rollout_exact(acts[t:t + 16].contiguous(), ra)
        b.rollout(acts[t:t + 16].contiguous(), rb)
        assert torch.equal(ra, rb), t
    assert _same_state(a, b)
    st = a.rollout_exact_stats()
    assert st["calls"] == 4 and st["list_env_steps"] == 0 and st["wave_env_steps"] == 0 and st["max_handed"] == 0, st


def test_scripted_grasp_equals_the_host_closed_route():
    """The scripted grasp, 1024 envs, 200 steps as twelve calls of 16 and one of 8: every row and the final state equal the host-closed
    route's bit for bit; the workload hands envs off inside calls, and some of them come back to 16 points or fewer."""
    n = 1024
    pos, acts_np = _grasp(n)
    a, b = _scene(n, True), _scene(n, True)
    b.set_diag(True)
    _reset((a, b), pos)
    a.rollout_exact_stats(reset=True)
    acts = torch.as_tensor(acts_np[:200], device=a.device)
    bufs = _bufs(b)
    mid_handoff = back_under = False
    for t0, k in _calls(200, 16):
        rows = torch.zeros((k, n, RS - 1), device=a.device)
        a.rollout_exact(acts[t0:t0 + k].contiguous(), rows)
        pts = []
        for j in range(k):
            b.step_begin(acts[t0 + j], *bufs)
            b.step_end()
            _assert_rows(rows[j], _row_of(bufs), f"step {t0 + j}")
            pts.append(b.get_diag(points=True)[3].clone())
        P = torch.stack(pts)  # (k, n) candidate points of each step
        over = P > 16
        first = torch.where(over.any(0), over.float().argmax(0), torch.full((n,), k, device=P.device))
        mid_handoff |= bool(((first > 0) & (first < k)).any())
        after = torch.arange(k, device=P.device)[:, None] > first[None, :]
        back_under |= bool((after & ~over).any())
        assert _same_state(a, b), f"call at step {t0}"
    st = a.rollout_exact_stats()
    assert st["list_env_steps"] > 0 and st["calls"] == 13, st
    assert mid_handoff and back_under


def _autoreset_args(n, pool_len, seed=3):
    rng = np.random.default_rng(seed)
    dev = torch.device("cuda")
    pool = np.stack([np.stack([rng.uniform(0.45, 0.8, n), rng.uniform(-0.25, 0.25, n), np.full(n, 0.02)], 1) for _ in range(pool_len)])
    return dict(spawn_pool=torch.as_tensor(pool.astype(np.float32), device=dev).contiguous(),
                obj_quat=torch.as_tensor(np.tile(np.array([0, 0, 0, 1], np.float32), (n, 1)), device=dev),
                arm_qpos=torch.as_tensor(np.tile(HOME, (n, 1)), device=dev))


def test_episode_loop_equals_the_host_closed_steps_with_autoreset():
    """rollout_autoreset_exact == K x (step_begin; step_end; mir_autoreset) with exact contacts on: the scripted grasp, max_len 37 (no
    divisor of the call length), pool 8 -- envs handed off are re-spawned inside a call.  Rows (truncated column included),
    episode lengths, cursors and the state, bit for bit."""
    n, T, K, L = 256, 160, 16, 37
    pos, acts_np = _grasp(n)
    a, b = _scene(n, True), _scene(n, True)
    b.set_diag(True)
    _reset((a, b), pos)
    ar = _autoreset_args(n, 8)
    respawned_after_handoff = False
    dev = a.device
    el_a, cur_a = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    el_b, cur_b = el_a.clone(), cur_a.clone()
    trunc, done = torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
    acts = torch.as_tensor(acts_np[:T], device=dev)
    bufs = _bufs(b)
    a.rollout_exact_stats(reset=True)
    for t0, k in _calls(T, K):
        rows = torch.zeros((k, n, RS), device=dev)
        a.rollout_autoreset_exact(acts[t0:t0 + k].contiguous(), rows, el_a, L, ar["spawn_pool"], cur_a, ar["obj_quat"], ar["arm_qpos"])
        handed = torch.zeros(n, dtype=torch.bool, device=dev)
        for j in range(k):
            b.step_begin(acts[t0 + j], *bufs)
            b.step_end()
            handed |= b.get_diag(points=True)[3] > 16   # (the envs the call has handed off by this step)
            b.autoreset(bufs[3], el_b, L, ar["spawn_pool"], cur_b, ar["obj_quat"], ar["arm_qpos"], trunc, done)
            if j < k - 1:
                respawned_after_handoff |= bool((handed & (done != 0)).any())
            want = torch.cat([_row_of(bufs), trunc[:, None].float()], 1)
            _assert_rows(rows[j], want, f"step {t0 + j}")
        assert torch.equal(el_a, el_b) and torch.equal(cur_a, cur_b), t0
        assert _same_state(a, b), t0
    assert int(cur_a.min()) >= 3 and respawned_after_handoff
    assert a.rollout_exact_stats()["list_env_steps"] > 0


def _comb(cap):
    """two rigid combs of eleven small boxes, one lying on the floor, the other resting on it tooth on tooth: 22 touching pairs (the
    scene of the exact-contact tests' candidate-pair case, restated)"""
    from gym_genesis.backend import spec as S

    sb = S.SceneBuilder()
    sb.add_geom(0, S.GEOM_PLANE)
    for name, z in (("a", 0.02), ("b", 0.0595)):
        sb.add_body(name, 0, pos=(0.0, 0.0, z), jtype=S.JNT_FREE, mass=0.55, inertia=S.box_inertia(0.55, (0.27, 0.02, 0.02)))
        for i in range(11):
            sb.add_geom(name, S.GEOM_BOX, size=(0.02, 0.02, 0.02), pos=(0.05 * (i - 5), 0.0, 0.0))
    sb.task = dict(eef_body=1, obj_body=2, grip_dof=(), reward_z=0.1)
    sb.opt["max_contacts"] = cap
    return sb.build()


def test_wave_tail_equals_the_wave_kernel_scene():
    """More candidate pairs than lanes: the envs go to the wave-per-env kernel's tail, and rollout_exact on the 16-capacity scene equals
    rollout on the 48-capacity wave-kernel scene bit for bit."""
    n = 64
    sc, wave = MirScene(_comb(16), n), MirScene(_comb(48), n)
    assert sc.kernel == 16 and wave.kernel == 64
    sc.set_exact_contacts(True)
    rng = np.random.default_rng(2)
    q = np.zeros((n, 14), np.float32)
    q[:, 2], q[:, 9] = 0.0199, 0.0595
    q[:, 7:9] = rng.uniform(-0.003, 0.003, (n, 2))
    q[:, 3], q[:, 10] = 1.0, 1.0
    for s_ in (sc, wave):
        s_.set_state(qpos=q, qvel=np.zeros((n, 12), np.float32), warmstart=np.zeros((n, 12), np.float32))
    sc.rollout_exact_stats(reset=True)
    assert sc.nu == 0
    nothing = torch.zeros(1, device=sc.device)  # (no actuator: the action blocks are empty, but the address must not be null)
    rd = sc.agent_dim + sc.env_dim + 2
    r1, r2 = torch.zeros((10, n, rd), device=sc.device), torch.zeros((10, n, rd), device=sc.device)
    for _ in range(2):
        assert sc.lib.mir_rollout_exact(sc.h, nothing.data_ptr(), 10, r1.data_ptr(), rd, None) == 0
        assert wave.lib.mir_rollout(wave.h, nothing.data_ptr(), 10, r2.data_ptr(), rd, None) == 0
        assert torch.equal(r1, r2)
    q1, v1, _, w1 = sc.get_state()
    q2, v2, _, w2 = wave.get_state()
    assert torch.equal(q1, q2[:, :q1.shape[1]]) and torch.equal(v1[:, :12], v2[:, :12]) and torch.equal(w1[:, :12], w2[:, :12])
    assert sc.rollout_exact_stats()["wave_env_steps"] == 20 * n


def test_twin_route_all_envs_on_the_list_instantiation():
    """set_exact_contacts("all"): every env starts on the three-contacts-per-lane instantiation at step 0; K x (begin; end) under "all"."""
    n = 256
    pos, acts_np = _grasp(n)
    a, b = _scene(n, "all"), _scene(n, "all")
    _reset((a, b), pos)
    acts = torch.as_tensor(acts_np[60:124], device=a.device)
    bufs = _bufs(b)
    a.rollout_exact_stats(reset=True)
    for t0, k in _calls(64, 16):
        rows = torch.zeros((k, n, RS - 1), device=a.device)
        a.rollout_exact(acts[t0:t0 + k].contiguous(), rows)
        for j in range(k):
            b.step_begin(acts[t0 + j], *bufs)
            b.step_end()
            _assert_rows(rows[j], _row_of(bufs), t0 + j)
    assert _same_state(a, b)
    assert a.rollout_exact_stats()["list_env_steps"] == 64 * n


def test_api():
    n = 64
    sc = _scene(n, True)
    pos, acts_np = _grasp(n)
    _reset((sc,), pos)
    A = torch.as_tensor(acts_np, device=sc.device)
    acts = A[:16].contiguous()
    rows = torch.zeros((16, n, RS - 1), device=sc.device)
    # K = 0: nothing happens
    v = sc.lib.mir_get_state_version(sc.h)
    assert sc.lib.mir_rollout_exact(sc.h, acts.data_ptr(), 0, rows.data_ptr(), RS - 1, None) == 0
    assert sc.lib.mir_get_state_version(sc.h) == v
    # null arguments, a short row stride
    assert sc.lib.mir_rollout_exact(sc.h, None, 4, rows.data_ptr(), RS - 1, None) != 0
    assert sc.lib.mir_rollout_exact(sc.h, acts.data_ptr(), 4, None, RS - 1, None) != 0
    with pytest.raises(MirError):
        sc.rollout_exact(acts, torch.zeros((16, n, 8), device=sc.device))
    with pytest.raises(MirError):
        sc.rollout_autoreset_exact(acts, rows, torch.zeros(n, dtype=torch.int32, device=sc.device), 10, torch.zeros((4, n, 3), device=sc.device),
                                   torch.zeros(n, dtype=torch.int32, device=sc.device), torch.zeros((n, 4), device=sc.device),
                                   torch.zeros((n, 9), device=sc.device))  # (no truncated column)
    # a wave-kernel scene is refused
    w = MirScene(models.franka_cube_stack_scene().build(), 4)
    assert w.kernel == 64
    with pytest.raises(MirError):
        w.rollout_exact(torch.zeros((2, 4, w.nu), device=w.device), torch.zeros((2, 4, w.agent_dim + w.env_dim + 2), device=w.device))
    # a pending step is closed first: begin, then rollout_exact == begin; end; rollout_exact
    a, b = _scene(n, True), _scene(n, True)
    _reset((a, b), pos)
    ba, bb = _bufs(a), _bufs(b)
    for t in range(90):  # (into the grasp)
        for s_, bu in ((a, ba), (b, bb)):
            s_.step_begin(A[t], *bu)
            s_.step_end()
    acts2 = A[90:106].contiguous()
    a.step_begin(A[90], *ba)
    b.step_begin(A[90], *bb)
    b.step_end()
    ra, rb = rows.clone(), rows.clone()
    a.rollout_exact(acts2, ra)
    b.rollout_exact(acts2, rb)
    assert torch.equal(ra, rb) and _same_state(a, b)
    # a host-closed overflow step on stream A, rollout_exact at once on stream B == the same on one stream
    c, d = _scene(n, True), _scene(n, True)
    _reset((c, d), pos)
    bc, bd = _bufs(c), _bufs(d)
    for t in range(100):
        for s_, bu in ((c, bc), (d, bd)):
            s_.step_begin(A[t], *bu)
            s_.step_end()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    c.exact_stats(reset=True)
    t = 100
    while True:   # (host-closed steps on stream A up to the first one that defers envs: their launches go to the library's side stream)
        with torch.cuda.stream(sa):
            c.step_begin(A[t], *bc)
            c.step_end()
        d.step_begin(A[t], *bd)
        d.step_end()
        t += 1
        if c.exact_stats()["overflow_steps"] > 0 or t == 200:
            break
    assert c.exact_stats()["overflow_steps"] == 1, t
    rc_, rd_ = rows.clone(), rows.clone()
    sb.wait_stream(sa)   # (the caller orders its own streams; what the library owns -- its side stream -- rollout_exact waits for itself)
    with torch.cuda.stream(sb):
        c.rollout_exact(acts2, rc_)
    d.rollout_exact(acts2, rd_)
    torch.cuda.synchronize()
    assert torch.equal(rc_, rd_) and _same_state(c, d)


def test_task_level_keep_exact_contacts():
    """enable_autoreset(keep_exact_contacts=True) keeps exact contacts without a warning and its rollout_autoreset() is the host-closed
    loop with autoreset; enable_autoreset() with no keyword still warns and switches them off."""
    from gym_genesis.env import GenesisEnv

    n, K = 64, 16
    env = GenesisEnv(task="cube_pick", robot="franka", num_envs=n, enable_pixels=False, exact_contacts=True)
    env.reset(seed=4)
    task = env._env
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        task.enable_autoreset(max_episode_steps=37, pool_len=8, keep_exact_contacts=True)
    assert task.exact_contacts and task._mir.exact_contacts
    twin = _scene(n, True)
    twin.set_state(*task._mir.get_state())
    el, cur = task._episode_len.clone(), task._cursor.clone()
    pos, acts_np = _grasp(n)
    acts = torch.as_tensor(acts_np[80:80 + 2 * K], device=twin.device)
    bufs = _bufs(twin)
    trunc, done = torch.zeros(n, dtype=torch.uint8, device=twin.device), torch.zeros(n, dtype=torch.uint8, device=twin.device)
    for t0 in (0, K):
        rows = torch.zeros((K, n, RS), device=twin.device)
        task.rollout_autoreset(acts[t0:t0 + K].contiguous(), rows)
        for j in range(K):
            twin.step_begin(acts[t0 + j], *bufs)
            twin.step_end()
            twin.autoreset(bufs[3], el, 37, task._spawn_pool, cur, task._quat, task._home, trunc, done)
            _assert_rows(rows[j], torch.cat([_row_of(bufs), trunc[:, None].float()], 1), t0 + j)
    assert torch.equal(el, task._episode_len) and torch.equal(cur, task._cursor)
    env2 = GenesisEnv(task="cube_pick", robot="franka", num_envs=n, enable_pixels=False, exact_contacts=True)
    env2.reset(seed=4)
    with pytest.warns(UserWarning):
        env2._env.enable_autoreset()
    assert not env2._env.exact_contacts and not env2._env._mir.exact_contacts


def test_wave_tail_resumes_inside_a_call_with_the_episode_loop():
    """The wave-kernel tail entered inside a call: both combs start in the air, the lower one lands on the floor (more than 16 points:
    the three-contacts-per-lane loop takes the env) and the upper one on it (more than 16 candidate pairs: the wave kernel takes it),
    each after the first step of the call; the episode loop (max_len 20, calls of 16) re-spawns it, comb on
    comb, inside the tail.  rollout_autoreset_exact == K x (step_begin; step_end; mir_autoreset) with exact contacts on, bit for bit."""
    n, K, T, L = 64, 16, 48, 20
    a, b = MirScene(_comb(16), n), MirScene(_comb(16), n)
    for s_ in (a, b):
        s_.set_exact_contacts(True)
    b.set_diag(True)
    rng = np.random.default_rng(2)
    q = np.zeros((n, 14), np.float32)
    q[:, 2], q[:, 9] = 0.03, 0.105
    q[:, 7:9] = rng.uniform(-0.003, 0.003, (n, 2))
    q[:, 3], q[:, 10] = 1.0, 1.0
    for s_ in (a, b):
        s_.set_state(qpos=q, qvel=np.zeros((n, 12), np.float32), warmstart=np.zeros((n, 12), np.float32))
    dev = a.device
    P = 4
    pool = np.zeros((P, n, 6), np.float32)
    pool[:, :, 2], pool[:, :, 5] = 0.0199, 0.0595   # (re-spawned comb on comb: the env stays above 16 pairs)
    pool[:, :, 3:5] = rng.uniform(-0.003, 0.003, (P, n, 2))
    pool = torch.as_tensor(pool, device=dev)
    quat = torch.as_tensor(np.tile(np.array([0, 0, 0, 1], np.float32), (n, 2, 1)), device=dev).contiguous()
    arm = torch.zeros((n, 1), device=dev)   # (no arm: the address must not be null)
    nothing = torch.zeros(1, device=dev)
    el_a, cur_a = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    el_b, cur_b = el_a.clone(), cur_a.clone()
    trunc, done = torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
    rd = a.agent_dim + a.env_dim + 3
    bufs = _bufs(b)
    a.rollout_exact_stats(reset=True)
    first_over = None
    for t0, k in _calls(T, K):
        rows = torch.zeros((k, n, rd), device=dev)
        assert a.lib.mir_rollout_autoreset_exact(a.h, nothing.data_ptr(), k, rows.data_ptr(), rd, el_a.data_ptr(), L, pool.data_ptr(), P,
                                                 cur_a.data_ptr(), quat.data_ptr(), arm.data_ptr(), None) == 0
        for j in range(k):
            b.step_begin(None, *bufs)
            b.step_end()
            if first_over is None and bool((b.get_diag(points=True)[3] > 48).any()):   # (pair overflow reads 255)
                first_over = t0 + j
            b.autoreset(bufs[3], el_b, L, pool, cur_b, quat, arm, trunc, done)
            _assert_rows(rows[j], torch.cat([_row_of(bufs), trunc[:, None].float()], 1), f"step {t0 + j}", dist=a.agent_dim + 10)
        assert torch.equal(el_a, el_b) and torch.equal(cur_a, cur_b), t0
        assert _same_state(a, b), t0
    st = a.rollout_exact_stats()
    assert first_over is not None and first_over % K != 0, first_over   # (the tail resumes an env at a step > 0 of its call)
    assert 0 < st["wave_env_steps"] < T * n and int(cur_a.min()) >= 2, st


def test_reference_expert_actions_replayed():
    """The reference's expert (examples/franka/pick_cube_state.py) through GenesisEnv(exact_contacts=True).step at 256 envs; its
    actions replayed by rollout_exact from the same reset state in calls of 20: every row against the env's observations, and the
    final state, bit for bit."""
    import importlib.util

    from gym_genesis.env import GenesisEnv

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("pick_cube_state", os.path.join(root, "examples", "franka", "pick_cube_state.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    n = 256
    env = GenesisEnv(task="cube_pick", robot="franka", num_envs=n, enable_pixels=False, exact_contacts=True)
    mir = env._env._mir
    assert mir.exact_contacts
    obs, _ = env.reset(seed=0)
    st0 = [x.clone() for x in mir.get_state()]
    mir.exact_stats(reset=True)
    acts, want = [], []
    for stage in ex.STAGES:
        for _ in range(40):
            a_ = ex.expert_policy(env.get_robot(), obs, stage)
            obs, reward, terminated, _, _ = env.step(a_)
            acts.append(a_.clone())
            want.append(torch.cat([obs["agent_pos"], obs["environment_state"], reward[:, None].float(),
                                   torch.as_tensor(terminated, device=reward.device)[:, None].float()], 1).clone())
    assert mir.exact_stats()["overflow_env_steps"] > 0
    T = len(acts)
    A = torch.stack(acts).contiguous()
    tw = _scene(n, True)
    tw.set_state(*st0)
    tw.rollout_exact_stats(reset=True)
    for t0, k in _calls(T, 20):
        rows = torch.zeros((k, n, RS - 1), device=tw.device)
        tw.rollout_exact(A[t0:t0 + k].contiguous(), rows)
        for j in range(k):
            _assert_rows(rows[j], want[t0 + j], f"step {t0 + j}")
    assert _same_state(tw, mir)
    assert tw.rollout_exact_stats()["list_env_steps"] > 0


def test_episode_loop_teacher_forced_against_the_capacity_48_oracle():
    """The episode loop of rollout_autoreset_exact against a reference that is not the library: the capacity-48 float64 oracle
    (oracle/orc.py) steps the scripted grasp; TimeLimit, terminated-or-truncated and the re-spawn from the pre-drawn pool are restated
    here from the header's words (mirigid.h, mir_autoreset), the re-spawned state from the oracle's own reset.  64 envs, max_len 25,
    calls of one step, the device started from the oracle's state every step: terminated, truncated, episode_len and cursor agree
    bit for bit (envs within 2e-6 m of the reward height left out of the masks), the one-step joint state within the float32 yardstick."""
    import orc

    n, L, P, T = 64, 25, 8, 100
    nt = min(16, len(os.sched_getaffinity(0)))
    sb = models.franka_cube_pick_scene()
    sb.opt["max_contacts"] = 48
    spec48 = sb.build()
    o, o_spawn = orc.Oracle(spec48, n), orc.Oracle(spec48, n)
    sc = _scene(n, True)
    sc.set_diag(True)
    pos, acts_np = _grasp(n)
    quat_np, arm_np = np.tile(np.array([0, 0, 0, 1], np.float32), (n, 1)), np.tile(HOME, (n, 1))
    o.reset(pos, quat_np, arm_np)
    sc.reset(pos, quat_np, arm_np)
    ar = _autoreset_args(n, P)
    pool_np = ar["spawn_pool"].cpu().numpy()
    dev = sc.device
    el, cur = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    el_h, cur_h = np.zeros(n, np.int64), np.zeros(n, np.int64)
    acts = torch.as_tensor(acts_np[50:50 + T], device=dev)
    rows = torch.zeros((1, n, RS), device=dev)
    errs, excluded = [], 0
    for t in range(T):
        q, v = o.state()
        ws = o.read_all(orc.F_QACC_WS, o.nv)
        sc.set_state(qpos=q.astype(np.float32), qvel=v.astype(np.float32), warmstart=ws.astype(np.float32))
        sc.rollout_autoreset_exact(acts[t:t + 1].contiguous(), rows, el, L, ar["spawn_pool"], cur, ar["obj_quat"], ar["arm_qpos"])
        o.step_batch(acts_np[50 + t], nt)
        qo = o.state()[0]
        term = o.get_obs_all()[3].astype(bool)
        # the episode rules, restated: one more step; terminated, or truncated at max_len; either ends the episode, whose env then
        # starts over from draw `cursor % pool_len` of the pool with the arm at home, at rest, and the cursor moves on
        ln = el_h + 1
        trunc = ~term & (ln >= L)
        done = term | trunc
        clear = np.abs(qo[:, 11] - 0.1) > 2e-6
        excluded += int((~clear).sum())
        r = rows[0].cpu().numpy()
        assert np.array_equal(r[clear, 21] != 0, term[clear]), t
        assert np.array_equal(r[clear, 22] != 0, trunc[clear]), t
        ncon_dev = sc.get_diag()[0].cpu().numpy()
        same = (ncon_dev == o.counts_all()[0]) & ~done
        errs.append(np.abs(sc.get_state()[0].cpu().numpy() - qo).max(1)[same])
        if done.any():
            o_spawn.reset(pool_np[cur_h % P, np.arange(n)], quat_np, arm_np)
            for f, nn in ((orc.F_QPOS, o.nq), (orc.F_QVEL, o.nv), (orc.F_QACC_WS, o.nv), (orc.F_TARGET, o.nv)):
                x, y = o.read_all(f, nn), o_spawn.read_all(f, nn)
                x[done] = y[done]
                o.write_all(f, x)
        el_h = np.where(done, 0, ln)
        cur_h = cur_h + done
        if clear.all():
            assert np.array_equal(el.cpu().numpy(), el_h) and np.array_equal(cur.cpu().numpy(), cur_h), t
        else:   # (an env at the threshold may end its episode on one side only: the others must agree)
            el_h[~clear] = el.cpu().numpy()[~clear]
            cur_h[~clear] = cur.cpu().numpy()[~clear]
            assert np.array_equal(el.cpu().numpy()[clear], el_h[clear]) and np.array_equal(cur.cpu().numpy()[clear], cur_h[clear]), t
    e = np.concatenate(errs)
    assert int(cur_h.min()) >= 3 and excluded < 20, (cur_h.min(), excluded)
    assert np.quantile(e, 0.99) < 2e-5 and np.median(e) < 2e-6, (np.quantile(e, 0.99), np.median(e))


def test_rows_and_observations_of_the_same_steps_without_the_switch():
    """What _assert_rows allows, pinned with exact contacts off: mir_rollout's packed rows against step_fused's observations of the
    same steps agree bit for bit but for the distance column, which differs by at most one ulp (and does differ on this workload)."""
    n = 1024
    pos, acts_np = _grasp(n)
    a, b = _scene(n), _scene(n)
    _reset((a, b), pos)
    acts = torch.as_tensor(acts_np[:16], device=a.device)
    rows = torch.zeros((16, n, RS - 1), device=a.device)
    a.rollout(acts, rows)
    bufs = _bufs(b)
    differs = False
    for j in range(16):
        b.step_fused(acts[j], *bufs)
        _assert_rows(rows[j], _row_of(bufs), j)
        differs |= not torch.equal(rows[j][:, DIST], _row_of(bufs)[:, DIST])
    assert differs
