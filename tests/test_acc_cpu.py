"""Link accelerations, Jdot qvel and IMU readings (include/mirigid.h: mir_link_accelerations), CPU tier.

  * the float64 reference of tests/acc_ref.py equals central finite differences of kin_ref's velocity along the motion;
  * acc - bias_acc = J qacc with kin_ref's Jacobian;
  * known answers: a body at rest, one revolute joint spinning, a free body under a pure qacc;
  * the views and the IMU sensor on a test double that serves `link_accelerations` from the reference;
  * the ctypes mirror of MirAccQuery has the layout a C compiler gives the header's struct.
The first two also on the synthetic trees of tests/tree_cases.py, every moving body of each.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import acc_ref
import kin_ref
import orc
import tree_cases
from fake_scene import OracleScene
from gym_genesis.backend import models
from gym_genesis.backend.spec import MIR_MAX_BODY, MirAccQuery, make_acc_query

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LP = (0.03, -0.02, 0.05)


def _scene(name):
    if name in tree_cases.CASES:
        return tree_cases.build(name)
    sb = models.franka_cube_pick_scene() if name == "pick" else models.franka_cube_stack_scene()
    return sb, sb.build()


def _links(sb, name):
    """hand, one finger (the longest path), first and last cube; every body of a synthetic tree that has a joint on its path"""
    if name in tree_cases.CASES:
        moves = [False] * len(sb.bodies)
        for b in range(1, len(sb.bodies)):
            moves[b] = moves[sb.bodies[b]["parent"]] or sb.bodies[b]["jtype"] != kin_ref.FIXED
        return [b for b in range(1, len(sb.bodies)) if moves[b]]
    cubes = ["cube"] if name == "pick" else [models.STACK_CUBES[0], models.STACK_CUBES[-1]]
    return [sb.body_index(n) for n in ["hand", "left_finger"] + cubes]


def _state(spec, model, seed):
    q, v = kin_ref.random_state(spec, model, 1, seed=seed)
    return q[0].astype(np.float64), v[0].astype(np.float64), np.random.default_rng(seed + 100).uniform(-2.0, 2.0, model.nv)


def _path_dofs(model, link):
    return [d for b in model.path(link) for d in range(model.dofadr[b], model.dofadr[b] + {0: 0, 1: 1, 2: 1, 3: 6}[model.jtype[b]])]


@pytest.mark.parametrize("scene", ["pick", "stack", *tree_cases.CASES])
def test_the_reference_equals_central_differences_of_the_velocity_along_the_motion(scene):
    """vel(t) = kin_ref's J(q(t)) qvel(t) along qvel(t) = qvel + t qacc, q(+-h) = integrate(q, qvel +- h/2 qacc, +-h) (the mean velocity
    over the interval: q(+-h) to O(h^3)); acc = (vel(h) - vel(-h)) / 2h.
    h = 1e-5: truncation h^2 / 6 x the third derivative of vel along the motion -- measured by the run at h = 1e-3, whose error of
    < 7e-6 is all truncation, so < 7e-10 at 1e-5 -- against round-off: vel is a sum of < 20 products of float64 poses that carry < 4.4e-14
    (test_kin_cpu.py), so < 1e-12 / 2h = 5e-8 at worst, in practice the 2e-11 the free bodies show.  Both < 1e-8 between h = 3e-6 and 3e-5.
    The model term: the oracle multiplies the model's float32-rounded frame quaternions along the path without normalising (orc_fk), so
    a frame's matrix is |Q|^2 R + (1 - |Q|^2) 1 with |Q|^2 = 1 + delta: an offset d = o_j - o_{j-1} holds a part delta |d| that does not turn
    with the parent.  The reference turns all of d: its w x (w x d) and alpha x d are off by at most delta |d| (|w|^2 + |alpha|) per
    element, |w| <= S = sum |qvel_i|, |alpha| <= S^2 + A, A = sum |qacc_i| over the path; the sum of |d| over the path with the local
    point is the reach, < 2 m: 2 delta (2 S^2 + A) with delta summed over the path as in test_kin_cpu.py, x 3 for the entries of a cross
    product.  Free bodies have delta = 0 and are held to 1e-8."""
    h, bound = 1e-5, 1e-8
    sb, spec = _scene(scene)
    model = kin_ref.Model(spec)
    o = orc.Oracle(spec, 1)
    q0, v0, qacc = _state(spec, model, 3)
    links = _links(sb, scene)

    def vel(q, v):
        o.write(orc.F_QPOS, q)
        o.write(orc.F_QVEL, v)
        return kin_ref.oracle_kinematics(o, model, links, LP)["vel"][0]

    fd = (vel(acc_ref.integrate(model, q0, v0 + 0.5 * h * qacc, h), v0 + h * qacc) - vel(acc_ref.integrate(model, q0, v0 - 0.5 * h * qacc, -h), v0 - h * qacc)) / (2 * h)
    o.write(orc.F_QPOS, q0)
    o.write(orc.F_QVEL, v0)
    ref = acc_ref.oracle_accelerations(o, model, links, qacc[None], LP)["acc"][0]
    for i, link in enumerate(links):
        dofs = _path_dofs(model, link)
        S, A = np.abs(v0[dofs]).sum(), np.abs(qacc[dofs]).sum()
        delta = sum(abs(float((np.array(list(spec.body[b].quat), np.float32).astype(np.float64) ** 2).sum()) - 1.0)
                    for b in model.path(link) if model.jtype[b] != kin_ref.FREE)
        allowed = bound + 6 * delta * (2 * S * S + A)
        err = float(np.abs(fd[i] - ref[i]).max())
        print(f"\n[acc, {scene}] link {link}: max |acc - FD| {err:.3e}, bound {allowed:.3e} (delta {delta:.2e}, |acc| {np.abs(ref[i]).max():.2f})")
        assert err < allowed, (scene, link, err, allowed)
        if scene not in tree_cases.CASES:
            assert np.abs(ref[i]).max() > 0.5
    # (a synthetic tree is asked link by link, a link under one joint included, whose acceleration is one random number: the scene must move)
    assert np.median(np.abs(ref).max(-1)) > 0.5


@pytest.mark.parametrize("scene", ["pick", "stack", *tree_cases.CASES])
def test_acc_minus_bias_acc_is_the_jacobian_times_qacc(scene):
    """Both sides are sums of < 20 float64 products of magnitudes < 10: 1e-13."""
    sb, spec = _scene(scene)
    model = kin_ref.Model(spec)
    o = orc.Oracle(spec, 1)
    q0, v0, qacc = _state(spec, model, 4)
    o.write(orc.F_QPOS, q0)
    o.write(orc.F_QVEL, v0)
    links = _links(sb, scene)
    ref = acc_ref.oracle_accelerations(o, model, links, qacc[None], LP)
    J = kin_ref.oracle_kinematics(o, model, links, LP)["jac"][0]
    assert np.abs(ref["acc"][0] - ref["bias_acc"][0] - J @ qacc).max() < 1e-13
    # bias_acc does not see qacc
    again = acc_ref.oracle_accelerations(o, model, links, np.zeros((1, model.nv)), LP)
    assert np.array_equal(again["bias_acc"], ref["bias_acc"]) and np.array_equal(again["acc"], again["bias_acc"])


def _pose(o, model, link):
    xp, xq = o.read(orc.F_XPOS).reshape(-1, 3), o.read(orc.F_XQUAT).reshape(-1, 4)
    return xp, kin_ref.quat_to_mat(xq[link] / np.linalg.norm(xq[link]))


def test_known_answers_at_rest_spinning_and_a_free_body():
    sb, spec = _scene("pick")
    model = kin_ref.Model(spec)
    o = orc.Oracle(spec, 1)
    q0, _, _ = _state(spec, model, 5)
    hand, cube = sb.body_index("hand"), sb.body_index("cube")
    nv, g = model.nv, np.array(list(spec.opt.gravity))
    assert g[2] < -9.0
    zero = np.zeros((1, nv))
    # ---- at rest: imu = (-g in the sensor's axes, 0), acc = 0
    qoff = np.array([0.5, 0.5, -0.5, 0.5])
    o.write(orc.F_QPOS, q0)
    o.write(orc.F_QVEL, np.zeros(nv))
    r = acc_ref.oracle_accelerations(o, model, [hand, cube], zero, LP, [qoff, (1.0, 0.0, 0.0, 0.0)])
    xp, Rh = _pose(o, model, hand)
    Rs = Rh @ kin_ref.quat_to_mat(qoff)
    assert np.abs(r["acc"]).max() == 0.0 and np.abs(r["imu"][0, :, 3:]).max() == 0.0
    assert np.abs(r["imu"][0, 0, :3] - Rs.T @ (-g)).max() < 1e-14
    assert abs(np.linalg.norm(r["imu"][0, 0, :3]) - 9.81) < 1e-12
    # (a cube lying flat: +9.81 along its own z)
    flat = q0.copy()
    qa = model.qadr[cube]
    flat[qa + 3:qa + 7] = (1.0, 0.0, 0.0, 0.0)
    o.write(orc.F_QPOS, flat)
    r = acc_ref.oracle_accelerations(o, model, [cube], zero)
    assert np.allclose(r["imu"][0, 0], (0.0, 0.0, 9.81, 0.0, 0.0, 0.0), atol=1e-15)
    # ---- one revolute joint spinning at constant qd (the Panda's first): centripetal qd^2 x the distance to the axis, toward the axis
    qd = 1.7
    v = np.zeros(nv)
    v[0] = qd
    o.write(orc.F_QPOS, q0)
    o.write(orc.F_QVEL, v)
    r = acc_ref.oracle_accelerations(o, model, [hand], zero, LP)
    k = kin_ref.oracle_kinematics(o, model, [hand], LP)
    b1 = model.path(hand)[[model.jtype[b] for b in model.path(hand)].index(kin_ref.REVOLUTE)]
    xp, _ = _pose(o, model, hand)
    xq1 = o.read(orc.F_XQUAT).reshape(-1, 4)[b1]
    axis = kin_ref.quat_to_mat(xq1 / np.linalg.norm(xq1)) @ model.axis[b1]
    arm = k["pos"][0, 0] - xp[b1]
    perp = arm - (arm @ axis) * axis
    assert np.linalg.norm(perp) > 0.05
    # (the model term of the finite-difference test: offsets of the oracle's frames hold a part ~1e-7 that does not turn)
    assert np.abs(r["acc"][0, 0, :3] + qd * qd * perp).max() < 1e-6 * qd * qd and np.abs(r["acc"][0, 0, 3:]).max() == 0.0
    assert np.array_equal(r["acc"], r["bias_acc"])
    assert np.abs(r["imu"][0, 0, 3:] - _pose(o, model, hand)[1].T @ (qd * axis)).max() < 1e-14
    # ---- a free body under a pure qacc reproduces it: [lin + ang x r; ang]
    a = np.zeros((1, nv))
    d = model.dofadr[cube]
    a[0, d:d + 6] = (0.3, -0.2, 0.5, 1.0, -2.0, 0.7)
    o.write(orc.F_QVEL, np.zeros(nv))
    r = acc_ref.oracle_accelerations(o, model, [cube, cube], a, [(0.0, 0.0, 0.0), LP])
    assert np.array_equal(r["acc"][0, 0], a[0, d:d + 6]) and np.abs(r["bias_acc"]).max() == 0.0
    _, Rc = _pose(o, model, cube)
    assert np.abs(r["acc"][0, 1, :3] - (a[0, d:d + 3] + np.cross(a[0, d + 3:d + 6], Rc @ np.array(LP)))).max() < 1e-15
    # ... and with a spin, the point's centripetal term w x (w x r)
    w = np.array([0.4, 0.9, -1.3])
    v = np.zeros(nv)
    v[d + 3:d + 6] = w
    o.write(orc.F_QVEL, v)
    r = acc_ref.oracle_accelerations(o, model, [cube], zero, LP)
    assert np.abs(r["acc"][0, 0, :3] - np.cross(w, np.cross(w, Rc @ np.array(LP)))).max() < 1e-15


# ---- the views and the sensor on a test double ---------------------------------------------------------------------------------------
class AccScene(OracleScene):
    """OracleScene with MirScene.link_accelerations served by the reference; qacc=None: zeros stand in for forward()"""

    def link_accelerations(self, links, local_points=None, quat_offsets=None, env_idx=None, qacc=None, acc=True, bias_acc=False, imu=False):
        make_acc_query(links, local_points, quat_offsets)  # (the argument checks of the product)
        model = kin_ref.Model(self.spec)
        envs = list(range(self.num_envs)) if env_idx is None else self._np(env_idx).reshape(-1).tolist()
        self.default_qacc = qacc is None
        a = np.zeros((len(envs), self.nv)) if qacc is None else self._np(qacc)
        k = acc_ref.oracle_accelerations(self.o, model, links, a, local_points, quat_offsets, envs)
        self.launches = getattr(self, "launches", 0) + 1
        want = dict(acc=acc, bias_acc=bias_acc, imu=imu)
        return {n: torch.from_numpy(np.ascontiguousarray(v.astype(np.float32))) for n, v in k.items() if want[n]}


@pytest.fixture(scope="module")
def pick_views():
    from gym_genesis.tasks.views import EntityView, SceneView

    sb = models.franka_cube_pick_scene()
    spec = sb.build()
    B = 5
    sc = AccScene(spec, B)
    model = kin_ref.Model(spec)
    q, v = kin_ref.random_state(spec, model, B, seed=9)
    sc.o.write_all(orc.F_QPOS, q.astype(np.float64))
    sc.o.write_all(orc.F_QVEL, v.astype(np.float64))
    robot = EntityView(sc, sb, root="link0", dof_names=models.FRANKA_JOINTS)
    cube = EntityView(sc, sb, root="cube", dof_names=())
    ref = acc_ref.oracle_accelerations(sc.o, model, list(range(1, spec.nbody)), np.zeros((B, model.nv)))   # computed once, left unchanged
    return sc, sb, robot, cube, ref, B, SceneView(sc)


def test_views_shapes_names_and_rows(pick_views):
    sc, sb, robot, cube, ref, B, scene = pick_views
    hand = robot.get_link("hand")
    n = robot.n_links
    acc = robot.get_links_acc()
    assert acc.shape == (B, n, 3) and acc.dtype == torch.float32 and robot.get_links_ang_acc().shape == (B, n, 3)
    assert np.allclose(acc.numpy(), ref["acc"][:, [b - 1 for b in robot.link_idx], 0:3], atol=1e-5)
    assert cube.get_links_acc().shape == (B, 1, 3) and robot.get_links_acc(links_idx_local=[9, 0]).shape == (B, 2, 3)
    assert hand.get_acc().shape == (B, 3) and hand.get_ang_acc().shape == (B, 3)
    assert np.allclose(hand.get_acc().numpy(), ref["acc"][:, hand.idx - 1, 0:3], atol=1e-5)
    assert np.allclose(hand.get_ang_acc().numpy(), ref["acc"][:, hand.idx - 1, 3:6], atol=1e-5)
    n0 = sc.launches
    jd = robot.get_jacobian_dot_qvel(hand)
    assert jd.shape == (B, 6) and sc.launches == n0 + 1
    assert np.allclose(jd.numpy(), ref["bias_acc"][:, hand.idx - 1], atol=1e-5)
    jp = robot.get_jacobian_dot_qvel(hand, local_point=(0.0, 0.0, 0.1))
    assert torch.equal(jp[:, 3:], jd[:, 3:]) and not torch.equal(jp[:, :3], jd[:, :3])
    for idx, rows in (([4, 0, 0, 3], [4, 0, 0, 3]), (torch.tensor([2, 1]), [2, 1]), (slice(1, 4), [1, 2, 3])):
        assert torch.equal(robot.get_links_acc(envs_idx=idx), acc[rows])
        assert torch.equal(robot.get_jacobian_dot_qvel(hand, envs_idx=idx), jd[rows])
        assert torch.equal(hand.get_acc(envs_idx=idx), hand.get_acc()[rows])
    with pytest.raises(IndexError):
        robot.get_links_acc(envs_idx=[0, B])
    with pytest.raises(ValueError):
        cube.get_jacobian_dot_qvel(hand)   # a link of another entity


def test_imu_options_and_sensor(pick_views):
    from gym_genesis.tasks.sensors import IMU, ImuSensor, Raycaster, euler_to_quat

    sc, sb, robot, cube, ref, B, scene = pick_views
    with pytest.raises(ValueError, match="entity"):
        scene.add_sensor(IMU(link="hand"))          # a link name without the entity it belongs to
    with pytest.raises(ValueError):
        scene.add_sensor(IMU())                     # nothing to ride on
    with pytest.raises(TypeError):
        scene.add_sensor(object())
    assert not isinstance(scene.add_sensor(Raycaster(entity=robot, link="hand")), ImuSensor)
    imu = scene.add_sensor(IMU(entity=robot, link="hand", pos_offset=(0.0, 0.01, 0.1), euler_offset=(90.0, 0.0, 30.0)))
    assert isinstance(imu, ImuSensor) and imu.link_body == sb.body_index("hand")
    assert np.allclose(imu.quat_offset, euler_to_quat((90.0, 0.0, 30.0)))
    assert scene.add_sensor(IMU(entity=cube)).link_body == cube.root
    assert scene.add_sensor(IMU(link=robot.get_link("hand"), quat_offset=(0.0, 1.0, 0.0, 0.0))).quat_offset == (0.0, 1.0, 0.0, 0.0)
    data = imu.read()
    assert data._fields == ("lin_acc", "ang_vel") and data.lin_acc.shape == (B, 3) and data.ang_vel.shape == (B, 3) and sc.default_qacc
    model = kin_ref.Model(sc.spec)
    qacc = np.random.default_rng(1).uniform(-1, 1, (2, model.nv))
    want = acc_ref.oracle_accelerations(sc.o, model, [imu.link_body], qacc, imu.pos_offset, imu.quat_offset, envs=[3, 1])["imu"][:, 0]
    got = imu.read(envs_idx=[3, 1], qacc=torch.from_numpy(qacc))
    assert not sc.default_qacc
    assert np.allclose(got.lin_acc.numpy(), want[:, :3], atol=1e-5) and np.allclose(got.ang_vel.numpy(), want[:, 3:], atol=1e-6)


# ---- the struct ------------------------------------------------------------------------------------------------------------------
def test_ctypes_mirror_of_the_query_struct_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mirigid.h"\n'
                   'int main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(MirAccQuery), offsetof(MirAccQuery, struct_size), offsetof(MirAccQuery, n_links),\n'
                   '         offsetof(MirAccQuery, link_body), offsetof(MirAccQuery, local_point), offsetof(MirAccQuery, quat_offset), offsetof(MirAccQuery, flags), MIR_MAX_BODY);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    mine = [C.sizeof(MirAccQuery)] + [getattr(MirAccQuery, f).offset for f in ("struct_size", "n_links", "link_body", "local_point", "quat_offset", "flags")] + [MIR_MAX_BODY]
    assert got == mine, (got, mine)


def test_make_acc_query_round_trips():
    q = make_acc_query([9, 12], [[0, 0, 0.1], [0.02, 0, 0]], [[0.5, 0.5, -0.5, 0.5], [0, 0, 0, 2]])
    assert q.struct_size == C.sizeof(MirAccQuery) and q.n_links == 2 and list(q.link_body[:2]) == [9, 12] and q.flags == 0
    assert abs(q.local_point[0][2] - 0.1) < 1e-7 and abs(q.local_point[1][0] - 0.02) < 1e-7
    assert list(q.quat_offset[0]) == [0.5, 0.5, -0.5, 0.5] and list(q.quat_offset[1]) == [0.0, 0.0, 0.0, 2.0], "as given: the library normalises"
    assert list(q.link_body[2:]) == [0] * (MIR_MAX_BODY - 2) and all(list(q.quat_offset[i]) == [0.0] * 4 for i in range(2, MIR_MAX_BODY))
    q = make_acc_query([3], (0.0, 0.1, 0.2))           # one point / no offset for every link
    assert np.allclose(list(q.local_point[0]), (0.0, 0.1, 0.2)) and list(q.quat_offset[0]) == [0.0] * 4, "all-zero = identity"
    q = make_acc_query([3, 4], np.array([0.0, 0.1, 0.2]), np.array([0.0, 1.0, 0.0, 0.0]))
    assert list(q.quat_offset[1]) == [0.0, 1.0, 0.0, 0.0] and np.allclose(list(q.local_point[1]), (0.0, 0.1, 0.2))
    for bad in (dict(links=[]), dict(links=list(range(1, MIR_MAX_BODY + 2))), dict(links=[1], local_points=(0.0, 1.0)),
                dict(links=[1, 2], quat_offsets=[[1, 0, 0, 0]]), dict(links=[1], flags=1)):
        with pytest.raises(ValueError):
            make_acc_query(**bad)


def test_the_library_reports_the_same_struct_size():
    from gym_genesis.backend.lib import load_library

    lib = load_library()
    assert lib.mir_acc_query_sizeof() == C.sizeof(MirAccQuery)
