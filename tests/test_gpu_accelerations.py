"""Link accelerations, Jdot qvel and IMU readings on the GPU (include/mirigid.h: mir_link_accelerations; views: get_links_acc,
get_links_ang_acc, get_jacobian_dot_qvel, get_acc; sensors: IMU).

States are SET (set_state), not stepped to: the GPU, the float64 oracle and its float32 port hold the same float32 bits, and all three
get the same seeded qacc.  B = 5 envs, the Franka pick scene (16-lane model, qpos rows of 16 floats) and the five-cube stack scene
(wave-kernel model, rows of 64); the hand, both fingers (the longest path) and every cube (a free root, a path of one), a local point on
the hand and on the first cube, sensor axes that are not the links'.

  * parity: acc, bias_acc, imu against the float64 reference of tests/acc_ref.py; metric = max absolute error per output over the
    batch; the GPU is allowed 4 x the same error of the float32 port (acc_ref in float32 on the poses of the oracle's float32 build) on
    the same states -- the rule and margin of tests/test_gpu_kinematics.py.  Both figures are printed;
  * identities between the outputs of this launch and those of mir_link_kinematics, evaluated in float64 from the float32 outputs, held
    to 4 x what the float32 port's outputs leave of the same identity;
  * rows, clamped tail pairs, every element written, nullable outputs; the default qacc; a cube at rest;
  * through GenesisEnv; a read is invisible; the error returns.
The MIR_E_CAPACITY case "a path of more than 16 bodies" is left out for the reason given in tests/test_gpu_kinematics.py: the scene
compilers refuse such a scene before it exists.  The other MIR_E_CAPACITY return, rows x links at 2^31, is checked.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import acc_ref
import kin_ref
import orc
from gym_genesis.backend import models
from gym_genesis.backend.spec import MirAccQuery, make_acc_query

pytestmark = pytest.mark.gpu

B = 5
OUTS = ("acc", "bias_acc", "imu")
ALL = dict(acc=True, bias_acc=True, imu=True)
_cache = {}


def _queried(sb, name):
    """hand, both fingers (the longest path), every cube; a non-zero local point on the hand and on the first cube; sensor axes turned
    against the link's on the hand, a finger and the first cube (one of them given unnormalised: the library normalises)"""
    cubes = ["cube"] if name == "pick" else list(models.STACK_CUBES)
    links = [sb.body_index(n) for n in ["hand", "left_finger", "right_finger"] + cubes]
    lps = np.zeros((len(links), 3))
    lps[0], lps[3] = (0.0, 0.01, 0.1), (0.02, -0.02, 0.02)
    qo = np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (len(links), 1))
    qo[0], qo[1], qo[3] = (0.5, 0.5, -0.5, 0.5), (0.6, 0.0, 1.6, 0.0), (0.9238795, 0.0, 0.0, 0.3826834)
    return links, lps, qo


def _setup(name):
    """scene with a seeded random state and qacc, the float64 reference and the float32 port of the queried links, computed once"""
    if name in _cache:
        return _cache[name]
    from gym_genesis.backend.lib import MirScene

    sb = models.franka_cube_pick_scene() if name == "pick" else models.franka_cube_stack_scene()
    spec = sb.build()
    model = kin_ref.Model(spec)
    sc = MirScene(spec, B)
    assert sc.kernel == (16 if name == "pick" else 64)
    q, v = kin_ref.random_state(spec, model, B, seed=41 if name == "pick" else 42)
    qacc = np.random.default_rng(43 if name == "pick" else 44).uniform(-2.0, 2.0, (B, model.nv)).astype(np.float32)
    sc.set_state(qpos=q, qvel=v)
    o64, port = orc.Oracle(spec, B), orc.Oracle(spec, B, f32=True if name == "pick" else "big")
    for o in (o64, port):
        o.write_all(orc.F_QPOS, q.astype(np.float64))
        o.write_all(orc.F_QVEL, v.astype(np.float64))
    links, lps, qo = _queried(sb, name)
    ref = acc_ref.oracle_accelerations(o64, model, links, qacc, lps, qo)
    prt = acc_ref.oracle_accelerations(port, model, links, qacc, lps, qo, dtype=np.float32)
    yard = {k: float(np.abs(prt[k].astype(np.float64) - ref[k]).max()) for k in OUTS}
    qacc_d = torch.as_tensor(qacc, device=sc.device)
    _cache[name] = dict(sb=sb, spec=spec, model=model, sc=sc, q=q, v=v, qacc=qacc, qacc_d=qacc_d, o64=o64, port=port, links=links, lps=lps, qo=qo,
                        ref=ref, prt=prt, yard=yard, full=sc.link_accelerations(links, lps, qo, qacc=qacc_d, **ALL))
    return _cache[name]


@pytest.mark.parametrize("name", ["pick", "stack"])
def test_parity_with_the_float64_reference(name):
    s = _setup(name)
    got = {k: x.cpu().numpy().astype(np.float64) for k, x in s["full"].items()}
    assert all(got[k].shape == (B, len(s["links"]), 6) for k in OUTS)
    e = {k: float(np.abs(got[k] - s["ref"][k]).max()) for k in OUTS}
    yard = s["yard"]
    print(f"\n[accelerations, {name}] max |x - x64| over {B} envs x {len(s['links'])} links:  "
          + "   ".join(f"{k}: GPU {e[k]:.3e} port {yard[k]:.3e} allowed {4 * yard[k]:.3e}" for k in OUTS))
    for k in OUTS:
        assert e[k] <= 4.0 * yard[k], (name, k, e[k], yard[k])
    assert float(np.abs(s["ref"]["bias_acc"]).max()) > 0.5 and float(np.abs(s["ref"]["acc"] - s["ref"]["bias_acc"]).max()) > 0.5
    # bias_acc is the same bits with another qacc and with none
    sc = s["sc"]
    alone = sc.link_accelerations(s["links"], s["lps"], s["qo"], acc=False, bias_acc=True)
    other = sc.link_accelerations(s["links"], s["lps"], s["qo"], qacc=-3.0 * s["qacc_d"], acc=True, bias_acc=True)
    assert torch.equal(alone["bias_acc"], s["full"]["bias_acc"]) and torch.equal(other["bias_acc"], s["full"]["bias_acc"])
    assert not torch.equal(other["acc"], s["full"]["acc"])


def _sensor_axes(quat, qo):
    """R_link R(quat_offset) in float64 from link quaternions (R,L,4) and offsets (L,4)"""
    out = np.zeros(quat.shape[:2] + (3, 3))
    for r in range(quat.shape[0]):
        for i in range(quat.shape[1]):
            out[r, i] = kin_ref.quat_to_mat(quat[r, i] / np.linalg.norm(quat[r, i])) @ kin_ref.quat_to_mat(qo[i] / np.linalg.norm(qo[i]))
    return out


def _residuals(acc, bias, imu, kin, qacc, qo):
    """what float32 outputs leave of the two identities, evaluated in float64: acc - bias_acc - J qacc, imu[3:] - R_s^T vel[3:]"""
    acc, bias, imu, qacc = (np.asarray(x).astype(np.float64) for x in (acc, bias, imu, qacc))
    jac, vel, quat = (np.asarray(kin[k]).astype(np.float64) for k in ("jac", "vel", "quat"))
    r1 = acc - bias - np.einsum("blkd,bd->blk", jac, qacc)
    r2 = imu[:, :, 3:] - np.einsum("blji,blj->bli", _sensor_axes(quat, qo), vel[:, :, 3:])
    return float(np.abs(r1).max()), float(np.abs(r2).max())


@pytest.mark.parametrize("name", ["pick", "stack"])
def test_identities_with_the_outputs_of_link_kinematics(name):
    s = _setup(name)
    sc, full = s["sc"], s["full"]
    kin = {k: x.cpu().numpy() for k, x in sc.link_kinematics(s["links"], s["lps"]).items()}
    g1, g2 = _residuals(full["acc"].cpu().numpy(), full["bias_acc"].cpu().numpy(), full["imu"].cpu().numpy(), kin, s["qacc"], s["qo"])
    pk = kin_ref.oracle_kinematics(s["port"], s["model"], s["links"], s["lps"], dtype=np.float32)
    p1, p2 = _residuals(s["prt"]["acc"], s["prt"]["bias_acc"], s["prt"]["imu"], pk, s["qacc"], s["qo"])
    print(f"\n[accelerations, {name}] |acc - bias_acc - jac @ qacc|: GPU {g1:.3e} port {p1:.3e} allowed {4 * p1:.3e}   "
          f"|imu_gyro - R_s^T vel_ang|: GPU {g2:.3e} port {p2:.3e} allowed {4 * p2:.3e}")
    assert g1 <= 4.0 * p1 and g2 <= 4.0 * p2, (name, g1, p1, g2, p2)


def _raw(sc, links, lps, qo, idx, want, qacc=None, h=None, q=None, n_rows=None):
    """mir_link_accelerations into ONE NaN-filled allocation that holds acc | bias_acc | imu side by side -> (rc, the three views); an
    output that is not in `want` is not passed, and must stay NaN like everything else the call does not own"""
    q = make_acc_query(links, lps, qo) if q is None else q
    R, L = (sc.num_envs if idx is None else len(idx)), len(links)
    buf = torch.full((3, R, L, 6), float("nan"), device=sc.device)
    out = dict(zip(OUTS, buf))
    it = None if idx is None else torch.tensor(idx, dtype=torch.long, device=sc.device)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    arg = lambda k: p(out[k]) if k in want else None  # noqa: E731
    rc = sc.lib.mir_link_accelerations(sc.h if h is None else h, None if q == "null" else C.byref(q), p(it), R if n_rows is None else n_rows, p(qacc),
                                       arg("acc"), arg("bias_acc"), arg("imu"), sc._stream())
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("name", ["pick", "stack"])
def test_rows_tail_pairs_every_element_written_and_nullable_outputs(name):
    s = _setup(name)
    sc, full, links, lps, qo, qd = s["sc"], s["full"], s["links"], s["lps"], s["qo"], s["qacc_d"]
    for idx in ([4, 0, 0, 3], [4, 3, 2, 1, 0], [2]):   # repeats, reversed, a subset
        rows = sc.link_accelerations(links, lps, qo, env_idx=torch.tensor(idx, device=sc.device), qacc=qd[idx].contiguous(), **ALL)
        for k in OUTS:
            assert rows[k].shape == (len(idx), len(links), 6) and torch.equal(rows[k], full[k][idx]), (name, k, idx)
    # L = 1: five pairs (a wave with one pair and three clamped ones), and one pair alone
    for li in (1, 3):
        one = sc.link_accelerations([links[li]], lps[li], qo[li], qacc=qd, **ALL)
        solo = sc.link_accelerations([links[li]], lps[li], qo[li], env_idx=torch.tensor([2], device=sc.device), qacc=qd[2:3].contiguous(), **ALL)
        for k in OUTS:
            assert torch.equal(one[k][:, 0], full[k][:, li]) and torch.equal(solo[k][0, 0], full[k][2, li]), (name, k, li)
    # R L = 3 x 3 = 9 pairs, not a multiple of four; NaN-filled outputs are fully written
    rc, out = _raw(sc, links[:3], lps[:3], qo[:3], [4, 0, 0], OUTS, qacc=qd[[4, 0, 0]].contiguous())
    assert rc == 0
    for k in OUTS:
        assert torch.isfinite(out[k]).all() and torch.equal(out[k], full[k][[4, 0, 0]][:, :3]), (name, k)
    rc, out = _raw(sc, links, lps, qo, None, OUTS, qacc=qd)
    assert rc == 0 and all(torch.equal(out[k], full[k]) for k in OUTS)
    # an output that is not asked for is untouched, the ones asked for are the same bits
    for want in (("bias_acc",), ("acc",), ("imu",), ("acc", "imu")):
        rc, out = _raw(sc, links, lps, qo, None, want, qacc=qd)
        assert rc == 0
        for k in OUTS:
            assert torch.equal(out[k], full[k]) if k in want else bool(torch.isnan(out[k]).all()), (name, want, k)
    rc, out = _raw(sc, links, lps, qo, None, ("bias_acc",))                 # bias_acc needs no qacc
    assert rc == 0 and torch.equal(out["bias_acc"], full["bias_acc"])
    rc, out = _raw(sc, links, lps, qo, None, (), qacc=qd)                   # nothing asked for
    assert rc == 0 and all(torch.isnan(out[k]).all() for k in OUTS)
    rc, out = _raw(sc, links, lps, qo, [0], OUTS, qacc=qd, n_rows=0)        # no rows
    assert rc == 0 and all(torch.isnan(out[k]).all() for k in OUTS)
    # an index outside the batch is clamped
    rows = sc.link_accelerations(links, lps, qo, env_idx=torch.tensor([-3, B + 7], device=sc.device), qacc=qd[[0, B - 1]].contiguous(), **ALL)
    assert all(torch.equal(rows[k], full[k][[0, B - 1]]) for k in OUTS)


@pytest.mark.parametrize("name", ["pick", "stack"])
def test_default_qacc_is_the_one_forward_reports(name):
    s = _setup(name)
    sc, links, lps, qo = s["sc"], s["links"], s["lps"], s["qo"]
    before = [x.clone() for x in sc.get_state()]
    bits = lambda t: t.contiguous().view(torch.int32)  # noqa: E731  (bit for bit, whatever the values)
    qf = sc.forward()[3]
    given = sc.link_accelerations(links, lps, qo, qacc=qf, **ALL)
    default = sc.link_accelerations(links, lps, qo, **ALL)
    for k in OUTS:
        assert torch.equal(bits(default[k]), bits(given[k])), (name, k)
    idx = [3, 3, 0]
    rows = sc.link_accelerations(links, lps, qo, env_idx=torch.tensor(idx, device=sc.device), **ALL)
    for k in OUTS:
        assert torch.equal(bits(rows[k]), bits(given[k][idx])), (name, k)
    assert float((given["acc"] - given["bias_acc"]).abs().max()) > 0.0
    sc.set_state(*before)   # (the shared scene goes back to the state the other tests compare)


def test_a_cube_at_rest_reads_plus_g_up_and_no_acceleration():
    """The tolerance is read from the run: the acceleration of the cube's point is a + wdot x r + w x (w x r) with (a, wdot) the cube's six
    qacc and w its angular velocity after settling, so |acc| <= |a| + |wdot| |r| + |w|^2 |r|, plus the float32 rounding of 9.81 through
    two rotations (8 x 2^-24 x 9.81 = 5e-6)."""
    from gym_genesis.backend.lib import MirScene

    sb = models.franka_cube_pick_scene()
    sc = MirScene(sb.build(), B)
    rng = np.random.RandomState(0)
    pos = np.stack([rng.uniform(0.45, 0.80, B), rng.uniform(-0.25, 0.25, B), np.full(B, 0.02)], 1).astype(np.float32)
    sc.reset(pos, np.tile(np.array([0, 0, 0, 1], np.float32), (B, 1)), np.tile(np.array(models.FRANKA_HOME, np.float32), (B, 1)))
    sc.step(100)
    cube = sb.body_index("cube")
    lp = np.array([0.02, -0.02, 0.02])
    qacc = sc.forward()[3]
    qv = sc.get_state()[1]
    a, wdot, w = (x.cpu().numpy().astype(np.float64) for x in (qacc[:, 9:12], qacc[:, 12:15], qv[:, 12:15]))
    nr = float(np.linalg.norm(lp))
    tol = np.linalg.norm(a, axis=1) + np.linalg.norm(wdot, axis=1) * nr + (w * w).sum(1) * nr + 5e-6
    r = sc.link_accelerations([cube], lp, env_idx=None, **ALL)
    quat = sc.link_kinematics([cube], pos=False, vel=False, jac=False)["quat"].cpu().numpy().astype(np.float64)
    acc, imu = r["acc"].cpu().numpy().astype(np.float64)[:, 0], r["imu"].cpu().numpy().astype(np.float64)[:, 0]
    g = np.array(list(sc.spec.opt.gravity))
    up = np.stack([kin_ref.quat_to_mat(quat[e, 0]) @ imu[e, :3] for e in range(B)])   # the accelerometer's reading in world axes
    e_acc, e_imu = np.linalg.norm(acc[:, :3], axis=1), np.linalg.norm(up + g[None, :], axis=1)
    print(f"\n[accelerations, cube at rest] settled |qacc| tolerance {tol.max():.3e}: |acc| {e_acc.max():.3e}, |imu_world - (-g)| {e_imu.max():.3e}, imu z {up[:, 2].min():.6f}")
    assert tol.max() < 0.05, "the cube has settled"
    assert (e_acc <= tol).all() and (e_imu <= tol).all()
    assert (np.abs(up[:, 2] - 9.81) <= tol).all() and -g[2] == 9.81


def _grasp(n):
    import test_gpu_contact_forces as cf

    return cf._grasp(n)


def test_through_genesis_env_against_the_reference_on_the_state_read_back():
    from gym_genesis.env import GenesisEnv
    from gym_genesis.tasks.sensors import IMU

    n = 8
    _, acts = _grasp(n)
    env = GenesisEnv(task="cube_pick", robot="franka", num_envs=n, enable_pixels=False)
    env.reset(seed=2)
    task = env._env
    mir, robot, cube = task._mir, task.franka, task.cube
    hand = robot.get_link("hand")
    imu = task.scene.add_sensor(IMU(entity=robot, link="hand", pos_offset=(0.0, 0.0, 0.05), euler_offset=(0.0, 90.0, 0.0)))
    spec = mir.spec
    model = kin_ref.Model(spec)
    o64, port = orc.Oracle(spec, n), orc.Oracle(spec, n, f32=True)
    A = torch.as_tensor(acts, device=mir.device)
    keys = ("links_acc", "ang_acc", "jdot_qvel", "imu_lin", "imu_gyro", "cube_acc")
    worst, yard = dict.fromkeys(keys, 0.0), dict.fromkeys(keys, 0.0)
    rl = list(robot.link_idx)
    for t in range(12):
        env.step(A[20 * t % acts.shape[0]])
        if t % 4 != 3:
            continue
        la, aa, jd, rd, ca = robot.get_links_acc(), robot.get_links_ang_acc(), robot.get_jacobian_dot_qvel(hand, local_point=(0.0, 0.01, 0.1)), imu.read(), cube.get_links_acc()
        assert la.shape == (n, robot.n_links, 3) and aa.shape == (n, robot.n_links, 3) and jd.shape == (n, 6) and ca.shape == (n, 1, 3)
        assert rd.lin_acc.shape == (n, 3) and rd.ang_vel.shape == (n, 3) and hand.get_acc().shape == (n, 3)
        # rows: the same bits as the full read (the default qacc is gathered to the rows)
        sub = [5, 0, 5]
        assert torch.equal(robot.get_links_acc(links_idx_local=[9, 0], envs_idx=sub), la[sub][:, [9, 0]])
        assert torch.equal(imu.read(envs_idx=torch.tensor(sub)).lin_acc, rd.lin_acc[sub]) and torch.equal(hand.get_acc(envs_idx=sub), la[sub][:, rl.index(hand.idx)])
        assert torch.equal(robot.get_jacobian_dot_qvel(hand, local_point=(0.0, 0.01, 0.1), envs_idx=sub), jd[sub])
        q, v = (x.cpu().numpy().astype(np.float64) for x in mir.get_state()[:2])
        qacc = mir.forward()[3].cpu().numpy().astype(np.float64)
        for o in (o64, port):
            o.write_all(orc.F_QPOS, q)
            o.write_all(orc.F_QVEL, v)
        res = []
        for o, dt in ((o64, np.float64), (port, np.float32)):
            every = acc_ref.oracle_accelerations(o, model, rl + [cube.root], qacc, dtype=dt)
            hj = acc_ref.oracle_accelerations(o, model, [hand.idx], qacc, (0.0, 0.01, 0.1), dtype=dt)
            hi = acc_ref.oracle_accelerations(o, model, [hand.idx], qacc, imu.pos_offset, imu.quat_offset, dtype=dt)
            res.append(dict(links_acc=every["acc"][:, :-1, :3], ang_acc=every["acc"][:, :-1, 3:], jdot_qvel=hj["bias_acc"][:, 0], imu_lin=hi["imu"][:, 0, :3],
                            imu_gyro=hi["imu"][:, 0, 3:], cube_acc=every["acc"][:, -1:, :3]))
        got = dict(links_acc=la, ang_acc=aa, jdot_qvel=jd, imu_lin=rd.lin_acc, imu_gyro=rd.ang_vel, cube_acc=ca)
        for k in keys:
            worst[k] = max(worst[k], float(np.abs(got[k].cpu().numpy().astype(np.float64) - res[0][k]).max()))
            yard[k] = max(yard[k], float(np.abs(res[1][k].astype(np.float64) - res[0][k]).max()))
    print("\n[accelerations, GenesisEnv, 3 reads x 8 envs] " + "   ".join(f"{k}: GPU {worst[k]:.3e} port {yard[k]:.3e} allowed {4 * yard[k]:.3e}" for k in keys))
    for k in keys:
        assert worst[k] <= 4.0 * yard[k], (k, worst[k], yard[k])


def _same(mirs, v0, where):
    for x, y in zip(mirs[0].get_state(), mirs[1].get_state()):   # qpos, qvel, targets, warm start
        assert torch.equal(x, y), where
    assert mirs[0].state_version - v0[0] == mirs[1].state_version - v0[1], where


@pytest.mark.parametrize("default_qacc", [False, True])
def test_a_read_is_invisible_on_the_env_step_path(default_qacc):
    """Two GenesisEnv twins on the rotated env.step path.  A caller's qacc: the one that reads after every step against the one that never
    does.  qacc=None: the one that reads against one that calls a bare forward() at the same points."""
    from gym_genesis.env import GenesisEnv

    n = 8
    _, acts = _grasp(n)
    envs = [GenesisEnv(task="cube_pick", robot="franka", num_envs=n, enable_pixels=False) for _ in range(2)]
    for e in envs:
        e.reset(seed=3)
    mirs = [e._env._mir for e in envs]
    links = list(range(1, mirs[0].nbody))
    A = torch.as_tensor(acts, device=mirs[0].device)
    qacc = torch.as_tensor(np.random.default_rng(8).uniform(-1, 1, (n, mirs[0].nv)).astype(np.float32), device=mirs[0].device)
    v0 = [m.state_version for m in mirs]
    for t in range(30):
        res = [e.step(A[8 * t % acts.shape[0]]) for e in envs]
        if default_qacc:
            mirs[0].link_accelerations(links, (0.01, 0.0, 0.02), **ALL)
            mirs[1].forward()
        else:
            mirs[0].link_accelerations(links, (0.01, 0.0, 0.02), qacc=qacc, **ALL)
        for k in ("agent_pos", "environment_state"):
            assert torch.equal(res[0][0][k], res[1][0][k]), (t, k)
        assert torch.equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])
        _same(mirs, v0, t)
    assert mirs[0].link_accelerations_launches == 30 and mirs[1].__dict__.get("link_accelerations_launches", 0) == 0


@pytest.mark.parametrize("default_qacc", [False, True])
def test_a_read_is_invisible_on_the_wave_kernel(default_qacc):
    """K steps, a read, K steps against 2K steps (against K steps, a bare forward(), K steps with qacc=None) on the five-cube stack scene:
    state, warm start, state version and the observation buffers of every step."""
    from gym_genesis.backend.lib import MirScene

    K = 6
    sb = models.franka_cube_stack_scene()
    spec = sb.build()
    mirs = [MirScene(spec, B) for _ in range(2)]
    assert mirs[0].kernel == 64
    rng = np.random.RandomState(0)
    pos = np.zeros((B, 5, 3), np.float32)
    pos[:, :, 0] = np.array([-0.3, -0.15, 0.0, 0.15, 0.3]) + rng.uniform(-0.03, 0.03, (B, 5))
    pos[:, :, 1] = rng.uniform(-0.2, 0.2, (B, 5))
    pos[:, :, 2] = models.STACK_CUBE_Z
    quat = np.tile(np.array([0, 0, 0, 1], np.float32), (B, 5, 1))
    home = np.tile(np.array(models.FRANKA_HOME, np.float32), (B, 1))
    acts = (home + rng.uniform(-0.5, 0.5, (2 * K, B, 9))).astype(np.float32)
    links = list(range(1, spec.nbody))
    qacc = torch.as_tensor(np.random.default_rng(9).uniform(-1, 1, (B, mirs[0].nv)).astype(np.float32), device=mirs[0].device)
    bufs = [(m.empty(m.agent_dim), m.empty(m.env_dim), m.empty(), m.empty(dtype=torch.uint8)) for m in mirs]
    for m in mirs:
        m.reset(pos, quat, home)
    v0 = [m.state_version for m in mirs]
    for t in range(2 * K):
        for m, b in zip(mirs, bufs):
            m.step_fused(torch.as_tensor(acts[t], device=m.device), *b)
        for x, y in zip(bufs[0], bufs[1]):
            assert torch.equal(x, y), t
        _same(mirs, v0, t)
        if t == K - 1:
            if default_qacc:
                mirs[0].link_accelerations(links, (0.01, 0.0, 0.02), **ALL)
                mirs[1].forward()
            else:
                mirs[0].link_accelerations(links, (0.01, 0.0, 0.02), qacc=qacc, **ALL)
            _same(mirs, v0, "read")


def test_errors_name_the_entry_point_and_launch_nothing():
    from gym_genesis.backend.lib import MirError

    s = _setup("pick")
    sc, links, lps, qo, qd = s["sc"], s["links"], s["lps"], s["qo"], s["qacc_d"]
    nbody = s["spec"].nbody
    good = lambda: make_acc_query(links, lps, qo)  # noqa: E731
    bad = []
    bad.append(_raw(sc, links, lps, qo, None, OUTS, qacc=qd, q="null"))
    bad.append(_raw(sc, links, lps, qo, None, OUTS, qacc=qd, h=C.c_void_p(0)))
    q = good(); q.struct_size -= 4; bad.append(_raw(sc, links, lps, qo, None, OUTS, qacc=qd, q=q))
    for nl in (0, 33, -1):
        q = good(); q.n_links = nl; bad.append(_raw(sc, links, lps, qo, None, OUTS, qacc=qd, q=q))
    for b in (nbody, 0, -2):                                                   # a link outside 1 .. nbody - 1 (0: the world)
        q = good(); q.link_body[2] = b; bad.append(_raw(sc, links, lps, qo, None, OUTS, qacc=qd, q=q))
    for x in (float("nan"), float("inf"), -float("inf")):
        q = good(); q.local_point[1][2] = x; bad.append(_raw(sc, links, lps, qo, None, OUTS, qacc=qd, q=q))
        q = good(); q.quat_offset[3][0] = x; bad.append(_raw(sc, links, lps, qo, None, OUTS, qacc=qd, q=q))
    for bit in (1, 1 << 31):
        q = good(); q.flags = bit; bad.append(_raw(sc, links, lps, qo, None, OUTS, qacc=qd, q=q))
    bad.append(_raw(sc, links, lps, qo, None, OUTS))                           # acc and imu without qacc
    bad.append(_raw(sc, links, lps, qo, None, ("acc",)))
    bad.append(_raw(sc, links, lps, qo, None, ("bias_acc", "imu")))
    bad.append(_raw(sc, links, lps, qo, [0], OUTS, qacc=qd, n_rows=-1))
    for rc, out in bad:
        assert rc == -1 and b"mir_link_accelerations" in sc.lib.mir_last_error(), rc
        assert all(torch.isnan(x).all() for x in out.values()), "a refused call launches nothing"
    rc, out = _raw(sc, links, lps, qo, [0], OUTS, qacc=qd, n_rows=2 ** 31 - 1)    # rows x links does not fit 2^31 - 1
    assert rc == -2 and b"mir_link_accelerations" in sc.lib.mir_last_error() and all(torch.isnan(x).all() for x in out.values())
    # an all-zero quat_offset is the identity, any other length is normalised
    zero = sc.link_accelerations(links, lps, np.zeros((len(links), 4)), qacc=qd, acc=False, imu=True)["imu"]
    ident = sc.link_accelerations(links, lps, None, qacc=qd, acc=False, imu=True)["imu"]
    twice = sc.link_accelerations(links, lps, 2.0 * qo, qacc=qd, acc=False, imu=True)["imu"]
    assert torch.equal(zero, ident) and float((twice - s["full"]["imu"]).abs().max()) < 1e-5
    # between mir_step_begin and mir_step_end
    bufs = (sc.empty(sc.agent_dim), sc.empty(sc.env_dim), sc.empty(), sc.empty(dtype=torch.uint8))
    before = [x.clone() for x in sc.get_state()]
    n0 = sc.__dict__.get("link_accelerations_launches", 0)
    sc.step_begin(None, *bufs)
    rc, out = _raw(sc, links, lps, qo, None, OUTS, qacc=qd)
    msg = sc.lib.mir_last_error()
    with pytest.raises(MirError, match="mir_link_accelerations.*pending"):
        sc.link_accelerations(links, qacc=qd)
    sc.step_end()
    assert rc == -1 and b"mir_link_accelerations" in msg and b"pending" in msg
    assert all(torch.isnan(x).all() for x in out.values()) and sc.__dict__.get("link_accelerations_launches", 0) == n0
    sc.set_state(*before)   # (the shared scene goes back to the state the other tests compare)
    assert C.sizeof(MirAccQuery) == sc.lib.mir_acc_query_sizeof()
    with pytest.raises(ValueError):
        sc.link_accelerations(links, qacc=qd[:2])
