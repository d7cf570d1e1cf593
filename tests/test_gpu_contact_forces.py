"""Contact force sensing on the GPU (include/mirigid.h: mir_contact_forces; views: get_links_net_contact_force / get_contacts).

  * parity with the float64 oracle, contact by contact (count, position, normal, penetration, force) and per class of links
    (tests/contact_force_ref.py), on states of the scripted grasp (tests/golden/grasp_targets.json) and of the five-cube stack scene,
    256 envs, both kernels.  Metric |F_gpu - F_orc64| / max(|F_orc64|, m_cube g); the GPU is allowed 4 x the same metric of the oracle's
    float32 port against the float64 oracle on the same states; both figures are printed.  An env whose contact set differs between
    GPU and oracle (a point at make / break within float32 rounding) is left out: at most 2 % of a scene's envs, counted and printed;
  * Newton's laws from the GPU alone (mir_contact_forces against mir_forward);
  * every point is there: states with 17 .. 48 points on the 16-lane scene report the oracle's count with the flag bit clear;
  * a read is invisible: two scenes, one read after every step, bitwise equal states and outputs over 200 steps of the grasp;
  * the views: shapes, filters, one launch per state.
"""
import json
import os

import numpy as np
import pytest
import torch

import contact_force_ref as ref
import orc
from gym_genesis.backend import models

pytestmark = pytest.mark.gpu

HOME = np.array(models.FRANKA_HOME, dtype=np.float32)
NT = max(1, min(16, len(os.sched_getaffinity(0))))
B = 256


def _spec48():
    sb = models.franka_cube_pick_scene()
    sb.opt["max_contacts"] = 48
    return sb.build()


def _grasp(n, seed=5):
    G_ = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "grasp_targets.json")))
    T = np.array(G_["targets"], np.float32)
    pos4 = np.array([[x, y, 0.02] for x, y in G_["cube_xy"]], np.float32)
    acts4 = np.repeat(T.transpose(1, 0, 2), G_["steps_per_stage"], axis=0)
    rep = n // 4
    pos = np.tile(pos4, (rep, 1))
    pos[:, :2] += np.random.default_rng(seed).uniform(-0.002, 0.002, (n, 2)).astype(np.float32)
    return pos, np.tile(acts4, (1, rep, 1))


def _bufs(sc):
    return (sc.empty(sc.agent_dim), sc.empty(sc.env_dim), sc.empty(), sc.empty(dtype=torch.uint8))


def _to_oracle(sc, o):
    """the scene's state and targets, as the device holds them, into every env of an oracle"""
    q, v, t, w = (x.cpu().numpy().astype(np.float64) for x in sc.get_state())
    tg = np.zeros((sc.num_envs, o.nv))
    tg[:, o.u_dofs] = t
    for f, x in ((orc.F_QPOS, q), (orc.F_QVEL, v), (orc.F_QACC_WS, w), (orc.F_TARGET, tg)):
        o.write_all(f, x)


def _compare(sc, spec_o, label, port_kind):
    """-> (gpu metric max, float32-port metric max, excluded envs, most contacts among the compared envs).  mu of every contact comes from
    the oracle's own rows (contact_force_ref.contact_mu), never from the GPU's list.  Envs left out are counted apart: `GPU differs`
    (its contact set is not the float64 oracle's) and `port differs` (the float32 port's is not)."""
    n = sc.num_envs
    o, port = orc.Oracle(spec_o, n), orc.Oracle(spec_o, n, f32=port_kind)
    _to_oracle(sc, o); _to_oracle(sc, port)
    out = {k: x.cpu().numpy() for k, x in sc.contact_forces().items()}
    classes = ref.body_classes(spec_o)
    cls, table = classes
    wcube = min(m for _, _, m in ref.free_bodies(spec_o)) * 9.81
    e_gpu = e_port = 0.0
    excluded = most = ex_gpu = ex_port = 0
    _compare.last = dict(compared=[], ncon=[])
    for e in range(n):
        o.forward(e); port.forward(e)
        r = ref.contact_forces(o, e, None, classes, spec_o)
        rp = ref.contact_forces(port, e, None, classes, spec_o)
        nc = int(out["n_contacts"][e])
        same = nc == r["n"] and (nc == 0 or np.abs(out["pos_normal_pen"][e, :nc, 0:3] - r["position"]).max() < 1e-4)
        same_p = rp["n"] == r["n"] and (r["n"] == 0 or np.abs(rp["position"] - r["position"]).max() < 1e-4)
        _compare.last["ncon"].append(r["n"])
        _compare.last["compared"].append(bool(same and same_p))
        if not (same and same_p):
            excluded += 1; ex_gpu += int(not same); ex_port += int(not same_p)
            continue
        most = max(most, nc)
        assert out["flags"][e] == 0
        assert (out["ids"][e, nc:] == 0).all() and (out["force"][e, nc:] == 0).all() and (out["pos_normal_pen"][e, nc:] == 0).all()
        if nc:
            ids = out["ids"][e, :nc]
            assert np.array_equal(cls[ids[:, 2]], r["cls_a"]) and np.array_equal(cls[ids[:, 3]], r["cls_b"]), (label, e, ids, r["cls_a"], r["cls_b"])
            for k in range(nc):  # the geoms belong to the links, and the larger of their frictions is the mu of the oracle's rows
                ga, gb = spec_o.geom[int(ids[k, 0])], spec_o.geom[int(ids[k, 1])]
                assert ga.body == ids[k, 2] and gb.body == ids[k, 3]
                assert abs(max(ga.friction, gb.friction) - r["mu"][k]) < 1e-6, (label, e, k, ga.friction, gb.friction, r["mu"][k])
            assert np.abs(out["pos_normal_pen"][e, :nc, 3:6] - r["normal"]).max() < 1e-4
            assert np.abs(out["pos_normal_pen"][e, :nc, 6] - r["penetration"]).max() < 1e-5
            den = np.maximum(np.linalg.norm(r["force"], axis=1), wcube)
            e_gpu = max(e_gpu, float((np.linalg.norm(out["force"][e, :nc] - r["force"], axis=1) / den).max()))
            e_port = max(e_port, float((np.linalg.norm(rp["force"] - r["force"], axis=1) / den).max()))
        cf = ref.class_sum(out["link_force"][e].astype(np.float64), cls, len(table))
        den = np.maximum(np.linalg.norm(r["class_force"], axis=1), wcube)
        e_gpu = max(e_gpu, float((np.linalg.norm(cf - r["class_force"], axis=1) / den).max()))
        e_port = max(e_port, float((np.linalg.norm(rp["class_force"] - r["class_force"], axis=1) / den).max()))
    print(f"\n[contact forces, {label}] {n} envs, most contacts in an env {most}: |F - F64| / max(|F64|, m g)  GPU {e_gpu:.3e}   float32 port {e_port:.3e}   "
          f"ratio {e_gpu / max(e_port, 1e-30):.2f}   envs left out (contact set differs) {excluded}: GPU differs {ex_gpu}, float32 port differs {ex_port}")
    return e_gpu, e_port, excluded, most


def _pick_scene(spec, checkpoints):
    """the scripted grasp, free-running with exact contacts on; yields the scene at the given steps"""
    from gym_genesis.backend.lib import MirScene

    pos, acts = _grasp(B)
    sc = MirScene(spec, B)
    if sc.kernel == 16:
        sc.set_exact_contacts(True)
    sc.reset(pos, np.tile(np.array([1, 0, 0, 0], np.float32), (B, 1)), np.tile(HOME, (B, 1)))
    bufs = _bufs(sc)
    A = torch.as_tensor(acts, device=sc.device)
    for t in range(max(checkpoints) + 1):
        sc.step_begin(A[t].contiguous(), *bufs); sc.step_end()
        if t in checkpoints:
            yield t, sc


@pytest.mark.parametrize("kernel", [16, 64])
def test_parity_with_the_oracle_on_the_scripted_grasp(franka_spec, kernel):
    spec = franka_spec if kernel == 16 else _spec48()
    G_ = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "grasp_targets.json")))
    sps = int(G_["steps_per_stage"])
    checkpoints = sorted({5, sps + sps // 2} | set(range(2 * sps + sps // 2, 5 * sps, 8)))  # (every eighth step from the closing of the fingers on)
    res = []
    for t, sc in _pick_scene(spec, checkpoints):
        assert sc.kernel == kernel
        res.append(_compare(sc, _spec48(), f"pick scene, kernel {kernel}, step {t}", "big"))
    g, p, exc, most = (np.array(x) for x in zip(*res))
    print(f"[contact forces, pick scene, kernel {kernel}] over the checkpoints: GPU {g.max():.3e}, float32 port (yardstick) {p.max():.3e}, allowed {4 * p.max():.3e}")
    assert (exc <= 0.02 * B).all(), exc
    assert most.max() > 16, "no state with more than 16 contact points among the checkpoints"
    assert g.max() <= 4.0 * p.max(), (g, p)


def test_parity_with_the_oracle_on_the_stack_scene():
    from gym_genesis.backend.lib import MirScene

    spec = models.franka_cube_stack_scene().build()
    sc = MirScene(spec, B)
    assert sc.kernel == 64
    rng = np.random.default_rng(11)
    nfree = sc.nfree
    pos = np.zeros((B, nfree, 3), np.float32)
    for j in range(nfree):  # a stack of all cubes, slightly offset, pressed together by up to 0.3 mm
        pos[:, j, 0] = 0.55 + rng.uniform(-0.003, 0.003, B)
        pos[:, j, 1] = rng.uniform(-0.003, 0.003, B)
        pos[:, j, 2] = 0.02 + 0.04 * j - 0.0001 * j
    quat = np.tile(np.array([1, 0, 0, 0], np.float32), (B, nfree, 1))
    sc.reset(pos, quat, np.tile(HOME, (B, 1)))
    sc.step(3)
    g, p, exc, most = _compare(sc, spec, "five-cube stack, wave-per-env kernel", "big")
    assert exc <= 0.02 * B and most >= 16
    assert g <= 4.0 * p, (g, p)


@pytest.mark.parametrize("kernel", [16, 64])
def test_newtons_laws_on_the_gpu_alone(franka_spec, kernel):
    spec = franka_spec if kernel == 16 else _spec48()
    G_ = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "grasp_targets.json")))
    sps = int(G_["steps_per_stage"])
    g = np.array(list(spec.opt.gravity))
    for t, sc in _pick_scene(spec, [3 * sps + sps // 2]):
        out = {k: x.cpu().numpy().astype(np.float64) for k, x in sc.contact_forces().items()}
        qacc = sc.forward()[3].cpu().numpy().astype(np.float64)
        lf = out["link_force"]
        # Every per-link sum adds at most 48 contact forces, each formed from 4 row forces on 3 directions (<= 4 x 48 terms of
        # magnitude <= Fmax = the largest contact force of the env, mu <= 1 included): float32 summation error <= terms x eps x Fmax per
        # link, and the sum over the links repeats every term once more with the opposite sign (twice that).  m (a - g) carries the
        # rounding of m a and of m g (2 eps each side, as in the CPU tier) and the solver's own stopping gradient, which the float32
        # solver holds at its floor of 16 eps x the tree's force scale; the force scale of the cube's tree is bounded by Fmax + m g.
        eps = 2.0 ** -24
        fmax = np.linalg.norm(out["force"], axis=2).max(1)
        for b, d0, mass in ref.free_bodies(spec):
            terms = 4 * 48
            bound = terms * eps * fmax + 4 * eps * mass * (np.abs(qacc[:, d0:d0 + 3]).max(1) + 9.81) + 16 * 2 * eps * (fmax + mass * 9.81) * np.sqrt(6.0)
            err = np.abs(lf[:, b] - mass * (qacc[:, d0:d0 + 3] - g)).max(1)
            print(f"\n[newton, kernel {kernel}] body {b}: max |F - m (a - g)| {err.max():.3e}, bound at that env {bound[err.argmax()]:.3e}, worst ratio {np.max(err / bound):.3f}")
            assert (err <= bound).all(), (err.max(), bound[err.argmax()])
        tot = np.abs(lf.sum(1)).max(1)
        assert (tot <= 2 * 4 * 48 * eps * np.maximum(fmax, 1e-30) + 1e-30).all(), tot.max()
        assert fmax.max() >= 0.9 * 0.25 * min(m_ for _, _, m_ in ref.free_bodies(spec)) * 9.81  # (a cube at rest: four points share its weight)


@pytest.mark.parametrize("kernel,exact", [(16, True), (16, False), (64, False)])
def test_a_read_is_invisible(franka_spec, kernel, exact):
    from gym_genesis.backend.lib import MirScene

    spec = franka_spec if kernel == 16 else _spec48()
    pos, acts = _grasp(B)
    scs = [MirScene(spec, B) for _ in range(2)]
    for sc in scs:
        if exact:
            sc.set_exact_contacts(True)
        sc.reset(pos, np.tile(np.array([1, 0, 0, 0], np.float32), (B, 1)), np.tile(HOME, (B, 1)))
    bufs = [_bufs(sc) for sc in scs]
    A = torch.as_tensor(acts, device=scs[0].device)
    v0 = [sc.state_version for sc in scs]
    reads = 0
    for t in range(200):
        for k, sc in enumerate(scs):
            sc.step_begin(A[t].contiguous(), *bufs[k]); sc.step_end()
        r = scs[0].contact_forces(contacts=(t % 2 == 0))
        reads += int(r["n_contacts"].max() > 0)
        sa, sb = scs[0].get_state(), scs[1].get_state()
        for x, y in zip(sa, sb):
            assert torch.equal(x, y), f"step {t}: state differs after a sensor read"
        for x, y in zip(bufs[0], bufs[1]):
            assert torch.equal(x, y), f"step {t}: outputs differ after a sensor read"
        assert scs[0].state_version - v0[0] == scs[1].state_version - v0[1]
    assert reads > 100


@pytest.mark.parametrize("kernel,exact", [(16, True), (16, False), (64, False)])
def test_state_version_advances_by_one_per_step_with_and_without_reads(franka_spec, kernel, exact):
    """Every step counts once, whatever launches serve it, and a read counts nothing.  (With exact contacts on, a step of an overflow
    run whose envs were all back at 16 points or fewer used to go uncounted -- one list launch that "completes a counted step" with no
    launch before it to count it; mir_step_begin counts it now.)"""
    from gym_genesis.backend.lib import MirScene

    spec = franka_spec if kernel == 16 else _spec48()
    pos, acts = _grasp(B)
    scs = [MirScene(spec, B) for _ in range(2)]
    for sc in scs:
        if exact:
            sc.set_exact_contacts(True)
        sc.reset(pos, np.tile(np.array([1, 0, 0, 0], np.float32), (B, 1)), np.tile(HOME, (B, 1)))
    bufs = [_bufs(sc) for sc in scs]
    A = torch.as_tensor(acts, device=scs[0].device)
    v0 = [sc.state_version for sc in scs]
    for t in range(200):
        for k, sc in enumerate(scs):
            sc.step_begin(A[t].contiguous(), *bufs[k]); sc.step_end()
        scs[0].contact_forces()
        assert [sc.state_version - v for sc, v in zip(scs, v0)] == [t + 1, t + 1]


def test_a_read_is_invisible_through_genesis_env_step():
    from gym_genesis.env import GenesisEnv

    _, acts = _grasp(B)
    envs = [GenesisEnv(task="cube_pick", robot="franka", num_envs=B, enable_pixels=False) for _ in range(2)]
    obs = [e.reset(seed=3)[0] for e in envs]
    robot, cube = envs[0]._env.franka, envs[0]._env.cube
    A = torch.as_tensor(acts, device=envs[0]._env._mir.device)
    for t in range(200):
        res = [e.step(A[t]) for e in envs]
        robot.get_links_net_contact_force(); cube.get_contacts(with_entity=robot)
        envs[0]._env._mir.contact_forces()
        for k in ("agent_pos", "environment_state"):
            assert torch.equal(res[0][0][k], res[1][0][k]), (t, k)
        assert torch.equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])
        sa, sb = envs[0]._env._mir.get_state(), envs[1]._env._mir.get_state()
        assert all(torch.equal(x, y) for x, y in zip(sa, sb)), t


def test_views_shapes_filters_and_one_launch_per_state():
    from gym_genesis.env import GenesisEnv

    _, acts = _grasp(B)
    env = GenesisEnv(task="cube_pick", robot="franka", num_envs=B, enable_pixels=False)
    env.reset(seed=1)
    mir, robot, cube = env._env._mir, env._env.franka, env._env.cube
    A = torch.as_tensor(acts, device=mir.device)
    for t in range(int(0.55 * acts.shape[0])):
        env.step(A[t])
    n0 = mir.contact_force_launches
    lf = robot.get_links_net_contact_force()
    c = cube.get_contacts(with_entity=robot)
    lc = cube.get_links_net_contact_force(envs_idx=[0, 3])
    assert mir.contact_force_launches == n0 + 1, "two getters on one state must share one launch"
    assert lf.shape == (B, 11, 3) and lf.dtype == torch.float32 and lf.is_cuda and lc.shape == (2, 1, 3)
    for k in ("geom_a", "geom_b", "link_a", "link_b", "penetration", "valid_mask"):
        assert c[k].shape == (B, 48), k
    for k in ("position", "force_a", "force_b"):
        assert c[k].shape == (B, 48, 3), k
    assert c["valid_mask"].dtype == torch.bool and torch.equal(c["force_a"], -c["force_b"])
    raw = {k: v.cpu().numpy() for k, v in mir.contact_sensor().items()}
    assert mir.contact_force_launches == n0 + 1
    ids = raw["ids"]
    valid = np.arange(48)[None, :] < raw["n_contacts"][:, None]
    rl = np.array(robot.link_idx)
    want = valid & (((ids[:, :, 2] == 12) & np.isin(ids[:, :, 3], rl)) | ((ids[:, :, 3] == 12) & np.isin(ids[:, :, 2], rl)))
    assert np.array_equal(c["valid_mask"].cpu().numpy(), want) and want.any()
    assert np.array_equal(c["force_b"].cpu().numpy()[want], raw["force"][want])
    assert np.array_equal(lf.cpu().numpy(), raw["link_force"][:, rl])
    q, v, tg, w = mir.get_state()
    mir.set_state(qpos=q)      # a setter in between: the next getter launches again
    cube.get_links_net_contact_force()
    assert mir.contact_force_launches == n0 + 2
    robot.control_dofs_position(robot.get_dofs_position())  # ... and so do new PD targets
    robot.get_links_net_contact_force()
    assert mir.contact_force_launches == n0 + 3
    cube.get_contacts()
    assert mir.contact_force_launches == n0 + 3


def test_grasp_semantics_both_fingers_push_on_the_held_cube_and_nothing_after_release():
    """The user's question -- "is the cube held": at the end of the reference expert's episode (examples/franka/pick_cube_state.py, the
    cube lifted) both finger links report a force on the cube, and the components along the finger axis (left finger -> right finger)
    oppose each other; after the fingers are opened and the cube has fallen, no contact joins robot and cube and the forces are exactly 0."""
    import importlib.util

    from gym_genesis.env import GenesisEnv

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sp = importlib.util.spec_from_file_location("pick_cube_state", os.path.join(root, "examples", "franka", "pick_cube_state.py"))
    ex = importlib.util.module_from_spec(sp)
    sp.loader.exec_module(ex)
    env = GenesisEnv(task="cube_pick", robot="franka", num_envs=B, enable_pixels=False)
    obs, _ = env.reset(seed=0)
    robot, cube = env.get_robot(), env._env.cube
    lifted = np.zeros(B, bool)
    for stage in ex.STAGES:
        for _ in range(40):
            a = ex.expert_policy(robot, obs, stage)
            obs, reward, terminated, truncated, info = env.step(a)
    lifted = terminated.copy()
    assert lifted.mean() > 0.5
    c = cube.get_contacts(with_entity=robot)
    lf, rf = robot.link_idx.index(10), robot.link_idx.index(11)   # left_finger, right_finger (models.py)
    axis = robot.get_link("right_finger").get_pos() - robot.get_link("left_finger").get_pos()
    axis = axis / axis.norm(dim=1, keepdim=True)
    # force ON THE CUBE from each finger: force_b where the cube is link b, force_a where it is link a
    on_cube = torch.where((c["link_b"] == 12)[:, :, None], c["force_b"], c["force_a"])
    other = torch.where(c["link_b"] == 12, c["link_a"], c["link_b"])
    fl = (on_cube * ((other == 10) & c["valid_mask"])[:, :, None]).sum(1)
    fr = (on_cube * ((other == 11) & c["valid_mask"])[:, :, None]).sum(1)
    al, ar = (fl * axis).sum(1).cpu().numpy(), (fr * axis).sum(1).cpu().numpy()
    held = torch.as_tensor(lifted)
    print(f"\n[grasp] lifted {lifted.mean():.3f}; force on the cube along the finger axis, lifted envs: left {np.median(al[lifted]):+.3f} N, right {np.median(ar[lifted]):+.3f} N (medians)")
    assert (al[lifted] > 0).all() and (ar[lifted] < 0).all(), "the left finger pushes the cube towards the right one and the other way round"
    net = robot.get_links_net_contact_force()
    assert (net[held][:, lf].norm(dim=1) > 0).all() and (net[held][:, rf].norm(dim=1) > 0).all()
    # release: fingers open, everything else stays; the cube falls out of the hand
    for _ in range(80):
        a2 = a.clone()
        a2[:, -2:] = 0.04
        obs, *_ = env.step(a2)
    c = cube.get_contacts(with_entity=robot)
    assert not bool(c["valid_mask"].any()), "no contact joins robot and cube after the release"
    assert float(c["force_a"].abs().max()) == 0.0 and float(c["force_b"].abs().max()) == 0.0
    c2 = robot.get_contacts(with_entity=cube)
    assert not bool(c2["valid_mask"].any())


def test_parity_with_the_oracle_on_the_so101_pads_on_the_cube():
    """The scene with TWO friction values (floor 1, robot and cube 5): the scripted SO-101 grasp of tests/test_gpu_so101_contact.py --
    gripper pressed on the floor, closed on the cube, dragged -- with mu per contact from the oracle's rows."""
    import test_gpu_so101_contact as so
    from gym_genesis.backend.lib import MirScene

    sb = models.so101_cube_pick_scene()
    spec = sb.build()
    sb.opt["max_contacts"] = 48
    spec48 = sb.build()
    assert ref.pair_mu_values(spec) == [1.0, 5.0]
    sc = MirScene(spec, B)
    assert sc.kernel == 16
    sc.set_exact_contacts(True)
    rng = np.random.RandomState(0)
    pos = np.stack([rng.uniform(0.2, 0.3, B), rng.uniform(-0.1, 0.1, B), np.full(B, 0.02)], 1).astype(np.float32)
    sc.reset(pos, np.tile(np.array([1, 0, 0, 0], np.float32), (B, 1)), np.zeros((B, sc.n_arm), np.float32))
    bufs = _bufs(sc)
    res, t = [], 0
    for name, q, steps in so.PICK_SCRIPT:
        a = torch.tensor(q, dtype=torch.float32, device=sc.device).repeat(B, 1)
        for k in range(steps):
            sc.step_begin(a, *bufs); sc.step_end()
            t += 1
            if name != "hover" and k % 40 == 39:
                res.append(_compare(sc, spec48, f"SO-101 pick scene, {name}, step {t}", "big"))
    g, p, exc, most = (np.array(x) for x in zip(*res))
    print(f"[contact forces, SO-101 pick scene] over the checkpoints: GPU {g.max():.3e}, float32 port (yardstick) {p.max():.3e}, allowed {4 * p.max():.3e}")
    assert (exc <= 0.02 * B).all(), exc
    assert most.max() >= 8
    assert g.max() <= 4.0 * p.max(), (g, p)


def test_every_point_is_there_above_32_points(franka_spec):
    """The third contact slot of a lane (contacts 32 .. 47): the reference expert presses both fingertips on the floor around the cube it
    holds.  From its episode, the states with the most contact points: n_contacts is the oracle's, the flag bit is clear, parity as above,
    and at least one env with more than 32 points is among the compared ones (not among those left out)."""
    import importlib.util

    from gym_genesis.env import GenesisEnv

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sp = importlib.util.spec_from_file_location("pick_cube_state", os.path.join(root, "examples", "franka", "pick_cube_state.py"))
    ex = importlib.util.module_from_spec(sp)
    sp.loader.exec_module(ex)
    env = GenesisEnv(task="cube_pick", robot="franka", num_envs=B, enable_pixels=False)
    obs, _ = env.reset(seed=0)
    mir, robot = env._env._mir, env.get_robot()
    assert mir.kernel == 16
    res, big_compared, seen = [], 0, 0
    for stage in ex.STAGES:
        for _ in range(40):
            obs, *_ = env.step(ex.expert_policy(robot, obs, stage))
            nc = mir.contact_forces(contacts=False)["n_contacts"]
            seen = max(seen, int(nc.max()))
            if int(nc.max()) > 32 and len(res) < 4:
                res.append(_compare(mir, _spec48(), f"reference expert, {stage}, most points {int(nc.max())}", "big"))
                last = _compare.last
                big_compared += sum(1 for n_, ok in zip(last["ncon"], last["compared"]) if n_ > 32 and ok)
    assert seen > 32, f"the expert's episode never exceeds 32 contact points at {B} envs (most: {seen})"
    g, p, exc, most = (np.array(x) for x in zip(*res))
    print(f"[contact forces, above 32 points] GPU {g.max():.3e}, float32 port (yardstick) {p.max():.3e}, allowed {4 * p.max():.3e}; envs above 32 points compared: {big_compared}")
    assert big_compared >= 1 and most.max() > 32
    assert (exc <= 0.02 * B).all(), exc
    assert g.max() <= 4.0 * p.max(), (g, p)


@pytest.mark.parametrize("cap", [16, 48])
def test_beyond_the_capacity_the_flag_bit_is_set(cap):
    """The two combs of tests/test_gpu_exact_contacts.py (eleven teeth resting tooth on tooth, one comb on the floor: 22 touching pairs,
    more than 16 candidate pairs and more than 48 candidate points): flag bit 0 set, n_contacts <= 48, every output finite, the links sum
    to zero -- on the 16-lane kernel's sensor instantiation (capacity 16 scene) and on the wave-per-env kernel (capacity 48 scene)."""
    from gym_genesis.backend import spec as S
    from gym_genesis.backend.lib import MirScene

    sb = S.SceneBuilder()
    sb.add_geom(0, S.GEOM_PLANE)
    for name, z in (("a", 0.02), ("b", 0.0595)):
        sb.add_body(name, 0, pos=(0.0, 0.0, z), jtype=S.JNT_FREE, mass=0.55, inertia=S.box_inertia(0.55, (0.27, 0.02, 0.02)))
        for i in range(11):
            sb.add_geom(name, S.GEOM_BOX, size=(0.02, 0.02, 0.02), pos=(0.05 * (i - 5), 0.0, 0.0))
    sb.task = dict(eef_body=1, obj_body=2, grip_dof=(), reward_z=0.1)
    sb.opt["max_contacts"] = cap
    n = 64
    sc = MirScene(sb.build(), n)
    assert sc.kernel == (16 if cap == 16 else 64)
    rng = np.random.default_rng(2)
    q = np.zeros((n, 14), np.float32)
    q[:, 2], q[:, 9] = 0.0199, 0.0595
    q[:, 7:9] = rng.uniform(-0.003, 0.003, (n, 2))
    q[:, 3], q[:, 10] = 1.0, 1.0
    sc.set_state(qpos=q, qvel=np.zeros((n, 12), np.float32), warmstart=np.zeros((n, 12), np.float32))
    before = [x.clone() for x in sc.get_state()]
    out = sc.contact_forces()
    nc, fl = out["n_contacts"].cpu().numpy(), out["flags"].cpu().numpy()
    print(f"\n[beyond the capacity, scene capacity {cap}, kernel {sc.kernel}] n_contacts {nc.min()} .. {nc.max()}, flags set in {int((fl & 1).sum())} of {n} envs")
    assert ((fl & 1) == 1).all() and (nc <= 48).all() and (nc > 16).all()
    for k in ("pos_normal_pen", "force", "link_force"):
        assert torch.isfinite(out[k]).all(), k
    lf = out["link_force"].cpu().numpy().astype(np.float64)
    fmax = np.linalg.norm(out["force"].cpu().numpy(), axis=2).max(1)
    assert (np.abs(lf.sum(1)).max(1) <= 2 * 4 * 48 * 2.0 ** -24 * fmax).all() and fmax.min() > 0
    ids = out["ids"].cpu().numpy()
    for e in range(n):
        assert (ids[e, nc[e]:] == 0).all() and (out["force"][e, nc[e]:] == 0).all()
        assert set(ids[e, :nc[e], 2:].ravel()) <= {0, 1, 2}
    for x, y in zip(before, sc.get_state()):
        assert torch.equal(x, y)


@pytest.mark.parametrize("kernel", [16, 64])
def test_a_read_is_invisible_to_mir_step(franka_spec, kernel):
    """The plain stepping route (control_dofs_position + scene.step(): mir_set_pd_targets, mir_step -- whole steps, other launch kinds
    than the begin / end path, and on the 16-lane kernel no scratch row to keep): 200 steps of the scripted grasp, a read after every
    step in one of two scenes; states bitwise equal and the state version one per step in both.  Every tenth step is three steps in one call."""
    from gym_genesis.backend.lib import MirScene

    spec = franka_spec if kernel == 16 else _spec48()
    pos, acts = _grasp(B)
    scs = [MirScene(spec, B) for _ in range(2)]
    for sc in scs:
        sc.reset(pos, np.tile(np.array([1, 0, 0, 0], np.float32), (B, 1)), np.tile(HOME, (B, 1)))
    A = torch.as_tensor(acts, device=scs[0].device)
    v0 = [sc.state_version for sc in scs]
    reads = 0
    for t in range(200):
        k = 3 if t % 10 == 9 else 1
        for sc in scs:
            sc.set_pd_targets(A[t].contiguous())
            sc.step(k)
        r = scs[0].contact_forces(link_force=(t % 2 == 0))
        reads += int(r["n_contacts"].max() > 0)
        for x, y in zip(scs[0].get_state(), scs[1].get_state()):
            assert torch.equal(x, y), f"step {t}: state differs after a sensor read"
        assert scs[0].state_version - v0[0] == scs[1].state_version - v0[1]
    for x, y in zip(scs[0].get_obs(), scs[1].get_obs()):
        assert torch.equal(x, y)
    assert reads > 100
