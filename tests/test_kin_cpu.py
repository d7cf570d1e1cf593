"""Link Jacobians, velocities and poses (include/mirigid.h: mir_link_kinematics), CPU tier.

  * the float64 reference of tests/kin_ref.py equals central finite differences of the oracle's forward kinematics;
  * its velocity equals the displacement of one oracle step (this pins the free joint's convention);
  * the views (get_jacobian, get_links_pos / quat / vel / ang, link.get_vel / get_ang) on a test double that serves
    `link_kinematics` from the reference;
  * the ctypes mirror of MirKinQuery has the layout a C compiler gives the header's struct.
The first two also on the synthetic trees of tests/tree_cases.py, every moving body of each.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import kin_ref
import orc
import tree_cases
from fake_scene import OracleScene
from gym_genesis.backend import models
from gym_genesis.backend.spec import MIR_MAX_BODY, MirKinQuery, make_kin_query

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scene(name):
    if name in tree_cases.CASES:
        return tree_cases.build(name)
    sb = models.franka_cube_pick_scene() if name == "pick" else models.franka_cube_stack_scene()
    return sb, sb.build()


def _links(sb, name):
    """hand, one finger, first and last cube; every body of a synthetic tree that has a joint on its path (the tests ask for a link that moves)"""
    if name in tree_cases.CASES:
        moves = [False] * len(sb.bodies)
        for b in range(1, len(sb.bodies)):
            moves[b] = moves[sb.bodies[b]["parent"]] or sb.bodies[b]["jtype"] != kin_ref.FIXED
        return [b for b in range(1, len(sb.bodies)) if moves[b]]
    cubes = ["cube"] if name == "pick" else [models.STACK_CUBES[0], models.STACK_CUBES[-1]]
    return [sb.body_index(n) for n in ["hand", "left_finger"] + cubes]


def _rotvec(qa, qb):
    """rotation vector of qa (x) qb^-1 (world axes), float64"""
    w1, x1, y1, z1 = qa
    w2, x2, y2, z2 = qb[0], -qb[1], -qb[2], -qb[3]
    d = np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                  w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])
    if d[0] < 0:
        d = -d
    s = np.linalg.norm(d[1:])
    return d[1:] * (2.0 * np.arctan2(s, d[0]) / s if s > 1e-300 else 2.0)


def _qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def _perturb(model, q, d, eps):
    """qpos moved by eps along scene dof d: a scalar dof moves its qpos entry; a free dof by the integrator's rule -- position += eps e_k,
    quaternion <- exp(eps e_k) (x) q"""
    q = q.copy()
    b = max(b for b in range(model.nbody) if model.dofadr[b] <= d and model.jtype[b] != kin_ref.FIXED)
    k, qa = d - model.dofadr[b], model.qadr[b]
    if model.jtype[b] != kin_ref.FREE:
        q[qa] += eps
    elif k < 3:
        q[qa + k] += eps
    else:
        dq = np.array([np.cos(0.5 * eps), 0.0, 0.0, 0.0])
        dq[1 + k - 3] = np.sin(0.5 * eps)
        q[qa + 3:qa + 7] = _qmul(dq, q[qa + 3:qa + 7])
    return q


def _pose(o, model, q, link, lp):
    o.write(orc.F_QPOS, q)
    o.fk()
    xp, xq = o.read(orc.F_XPOS).reshape(-1, 3), o.read(orc.F_XQUAT).reshape(-1, 4)
    ql = xq[link] / np.linalg.norm(xq[link])
    return xp[link] + kin_ref.quat_to_mat(ql) @ np.asarray(lp), ql


@pytest.mark.parametrize("scene", ["pick", "stack", *tree_cases.CASES])
def test_the_reference_jacobian_equals_central_differences_of_the_oracles_fk(scene):
    """eps = 1e-5 and the bound 1e-8 + a model term, from the errors of a central difference in float64.  Truncation: eps^2 / 6 x the
    third derivative of a pose along one dof, at most the lever arm (< 2 m with the local point) for positions and 1 for orientations:
    < 4e-11.  Round-off: the oracle's forward kinematics is a chain of < 200 float64 operations on magnitudes < 2, so a pose carries
    < 200 x 2^-53 x 2 = 4.4e-14, and the difference of two of them divided by 2 eps < 4.4e-9.  Sum < 1e-8.
    The model term: the oracle holds the model's frame quaternions rounded to float32, as the product does, and multiplies them along
    the path without normalising (orc_fk), so the "rotation" of a link's frame is q2mat of a quaternion with |Q|^2 = 1 + delta,
    |delta| <= the sum over the path of | |float32(quat_b)|^2 - 1 | (computed below from the spec), whose entries differ from those of a
    rotation by at most 2 delta.  The table's columns assume rigid frames; the derivative of the oracle's map differs from them by at
    most 3 entries x 2 delta x the lever arm (< 2 m) = 12 delta.  (The Panda's path to a finger: delta of a few 1e-7.)"""
    eps, bound = 1e-5, 1e-8
    sb, spec = _scene(scene)
    model = kin_ref.Model(spec)
    o = orc.Oracle(spec, 1)
    q0, v0 = kin_ref.random_state(spec, model, 1, seed=3)
    q0, v0 = q0[0].astype(np.float64), v0[0].astype(np.float64)
    worst = 0.0
    for link in _links(sb, scene):
        for lp in ((0.0, 0.0, 0.0), (0.03, -0.02, 0.05)):
            o.write(orc.F_QPOS, q0)
            o.write(orc.F_QVEL, v0)
            ref = kin_ref.oracle_kinematics(o, model, [link], lp)
            J = ref["jac"][0, 0]
            fd = np.zeros_like(J)
            for d in range(model.nv):
                pp, qp = _pose(o, model, _perturb(model, q0, d, eps), link, lp)
                pm, qm = _pose(o, model, _perturb(model, q0, d, -eps), link, lp)
                fd[0:3, d], fd[3:6, d] = (pp - pm) / (2 * eps), _rotvec(qp, qm) / (2 * eps)
            delta = sum(abs(float((np.array(list(spec.body[b].quat), np.float32).astype(np.float64) ** 2).sum()) - 1.0)
                        for b in model.path(link) if model.jtype[b] != kin_ref.FREE)
            err = float(np.abs(J - fd).max())
            worst = max(worst, err)
            print(f"\n[kin, {scene}] link {link}, local point {lp}: max |J - FD| {err:.3e}, bound {bound + 12 * delta:.3e} (delta {delta:.2e})")
            assert err < bound + 12 * delta, (scene, link, lp, err, delta)
            on = sorted({c for c in range(model.nv) if np.abs(J[:, c]).max() > 0})
            want = sorted(d for b in model.path(link) for d in range(model.dofadr[b], model.dofadr[b] + {0: 0, 1: 1, 2: 1, 3: 6}[model.jtype[b]]))
            assert on == want, "the non-zero columns are the dofs of the path"
    print(f"\n[kin, {scene}] analytic Jacobian against central differences (eps {eps:g}): max |J - FD| over the links {worst:.3e}")


@pytest.mark.parametrize("scene", ["pick", "stack", *tree_cases.CASES])
def test_the_reference_velocity_equals_the_displacement_of_one_oracle_step(scene):
    """One step of the oracle with dt = 1e-6 from a state in free space: the oracle updates qvel, then moves qpos with the NEW qvel (a
    free body: position += dt v, quaternion <- exp(w dt) (x) q).  So (p(q1) - p(q0)) / dt = J(q0) qvel1 + dt / 2 x the second derivative
    of p along the motion, which is at most (sum |qvel_i|)^2 x the lever arm (< 2 m; 1 for the orientation): the bound below, plus the
    round-off of the difference, 4.4e-14 / dt, and the model term of the test above, 12 delta per unit of |qvel_i|."""
    dt = float(np.float32(1e-6))   # (the oracle rounds the step to float32, the kernels' dt)
    sb, _ = _scene(scene)
    sb.opt["dt"] = dt
    sb.opt["enable_collision"] = 0
    spec = sb.build()
    model = kin_ref.Model(spec)
    o = orc.Oracle(spec, 1)
    q0, v0 = kin_ref.random_state(spec, model, 1, seed=4)
    q0, v0 = q0[0].astype(np.float64), v0[0].astype(np.float64)
    moved = []
    for link in _links(sb, scene):
        lp = (0.03, -0.02, 0.05)
        o.write(orc.F_QPOS, q0)
        o.write(orc.F_QVEL, v0)
        o.write(orc.F_QACC_WS, np.zeros(model.nv))
        p0, ql0 = _pose(o, model, q0, link, lp)
        o.step(0)
        q1, v1 = o.read(orc.F_QPOS), o.read(orc.F_QVEL)
        o.write(orc.F_QPOS, q0)
        o.write(orc.F_QVEL, v1)
        vel = kin_ref.oracle_kinematics(o, model, [link], lp)["vel"][0, 0]
        p1, ql1 = _pose(o, model, q1, link, lp)
        fd = np.concatenate([(p1 - p0) / dt, _rotvec(ql1, ql0) / dt])
        path_dofs = [d for b in model.path(link) for d in range(model.dofadr[b], model.dofadr[b] + {0: 0, 1: 1, 2: 1, 3: 6}[model.jtype[b]])]
        delta = sum(abs(float((np.array(list(spec.body[b].quat), np.float32).astype(np.float64) ** 2).sum()) - 1.0)
                    for b in model.path(link) if model.jtype[b] != kin_ref.FREE)
        bound = 0.5 * dt * np.abs(v1[path_dofs]).sum() ** 2 * 2.0 + 4.4e-14 / dt + 12 * delta * np.abs(v1[path_dofs]).sum()
        err = float(np.abs(vel - fd).max())
        print(f"\n[kin, {scene}] link {link}: |J qvel - dp / dt| {err:.3e}, bound {bound:.3e}")
        assert err < bound, (scene, link, err, bound)
        moved.append(float(np.abs(vel).max()))
        if scene not in tree_cases.CASES:
            assert np.abs(vel).max() > 0.05
    # (a synthetic tree is asked link by link, a link under one joint included, whose speed is one random number: the scene must move)
    assert max(moved) > 0.05 and np.median(moved) > 0.05


# ---- the views on a test double -------------------------------------------------------------------------------------------------
class KinScene(OracleScene):
    """OracleScene with MirScene.link_kinematics served by the reference"""

    def link_kinematics(self, links, local_points=None, env_idx=None, dof0=0, n_dofs=None, pos=True, quat=True, vel=True, jac=True):
        make_kin_query(links, local_points, dof0, self.nv - dof0 if n_dofs is None else n_dofs)  # (the argument checks of the product)
        model = kin_ref.Model(self.spec)
        envs = None if env_idx is None else self._np(env_idx).reshape(-1)
        k = kin_ref.oracle_kinematics(self.o, model, links, local_points, envs)
        nd = self.nv - dof0 if n_dofs is None else n_dofs
        k["jac"] = k["jac"][:, :, :, dof0:dof0 + nd]
        self.launches = getattr(self, "launches", 0) + 1
        want = dict(pos=pos, quat=quat, vel=vel, jac=jac)
        return {n: torch.from_numpy(np.ascontiguousarray(v.astype(np.float32))) for n, v in k.items() if want[n]}


@pytest.fixture(scope="module")
def pick_views():
    from gym_genesis.tasks.views import EntityView

    sb = models.franka_cube_pick_scene()
    spec = sb.build()
    B = 5
    sc = KinScene(spec, B)
    model = kin_ref.Model(spec)
    q, v = kin_ref.random_state(spec, model, B, seed=9)
    sc.o.write_all(orc.F_QPOS, q.astype(np.float64))
    sc.o.write_all(orc.F_QVEL, v.astype(np.float64))
    robot = EntityView(sc, sb, root="link0", dof_names=models.FRANKA_JOINTS)
    cube = EntityView(sc, sb, root="cube", dof_names=())
    ref = kin_ref.oracle_kinematics(sc.o, model, list(range(1, spec.nbody)))   # computed once, left unchanged
    return sc, sb, robot, cube, ref, B


def test_views_shapes_and_entity_columns(pick_views):
    sc, sb, robot, cube, ref, B = pick_views
    hand = robot.get_link("hand")
    J = robot.get_jacobian(hand)
    assert J.shape == (B, 6, 9) and J.dtype == torch.float32
    assert np.allclose(J.numpy(), ref["jac"][:, hand.idx - 1, :, 0:9], atol=1e-6)
    Jc = cube.get_jacobian(0)
    assert Jc.shape == (B, 6, 6)
    assert np.allclose(Jc.numpy(), ref["jac"][:, sb.body_index("cube") - 1, :, 9:15], atol=1e-6), "the cube's columns start at scene dof 9"
    assert np.array_equal(Jc.numpy()[:, 0:3, 0:3], np.tile(np.eye(3, dtype=np.float32), (B, 1, 1)))
    # a LinkView and its local index are the same link; a local point moves the linear rows only
    assert torch.equal(robot.get_jacobian(robot.link_idx.index(hand.idx)), J)
    Jp = robot.get_jacobian(hand, local_point=(0.0, 0.0, 0.1))
    assert torch.equal(Jp[:, 3:6], J[:, 3:6]) and not torch.equal(Jp[:, 0:3], J[:, 0:3])
    n = robot.n_links
    assert robot.get_links_pos().shape == (B, n, 3) and robot.get_links_quat().shape == (B, n, 4)
    assert robot.get_links_vel().shape == (B, n, 3) and robot.get_links_ang().shape == (B, n, 3)
    assert cube.get_links_vel().shape == (B, 1, 3) and robot.get_links_vel(links_idx_local=[9, 0]).shape == (B, 2, 3)
    assert np.allclose(robot.get_links_vel(links_idx_local=[9, 0]).numpy(), ref["vel"][:, [robot.link_idx[9] - 1, robot.link_idx[0] - 1], 0:3], atol=1e-6)
    assert hand.get_vel().shape == (B, 3) and hand.get_ang().shape == (B, 3)
    assert np.allclose(hand.get_vel().numpy(), ref["vel"][:, hand.idx - 1, 0:3], atol=1e-6)
    assert np.allclose(hand.get_ang().numpy(), ref["vel"][:, hand.idx - 1, 3:6], atol=1e-6)
    # the cube's velocity is its qvel (free joint: world linear velocity of the origin, world angular velocity)
    qv = sc.get_state()[1].numpy()
    assert np.allclose(cube.get_links_vel().numpy()[:, 0], qv[:, 9:12], atol=1e-6) and np.allclose(cube.get_links_ang().numpy()[:, 0], qv[:, 12:15], atol=1e-6)
    # poses agree with the route the existing getters take
    assert np.allclose(robot.get_links_pos().numpy(), sc.get_links()[0].numpy()[:, robot.link_idx], atol=1e-6)


def test_views_pair_of_results_from_one_launch(pick_views):
    sc, sb, robot, cube, ref, B = pick_views
    n0 = getattr(sc, "launches", 0)
    k = robot.links_kinematics(quat=False)
    assert sc.launches == n0 + 1 and set(k) == {"pos", "vel", "ang"}
    assert k["pos"].shape == (B, robot.n_links, 3) and k["ang"].shape == (B, robot.n_links, 3)


def test_views_envs_idx_as_list_tensor_and_slice(pick_views):
    sc, sb, robot, cube, ref, B = pick_views
    hand = robot.get_link("hand")
    full = robot.get_jacobian(hand)
    for idx, rows in (([4, 0, 0, 3], [4, 0, 0, 3]), (torch.tensor([2, 1]), [2, 1]), (slice(1, 4), [1, 2, 3]), (np.arange(B), list(range(B)))):
        J = robot.get_jacobian(hand, envs_idx=idx)
        assert J.shape == (len(rows), 6, 9) and torch.equal(J, full[rows])
        assert torch.equal(hand.get_vel(envs_idx=idx), hand.get_vel()[rows])
        assert torch.equal(cube.get_links_ang(envs_idx=idx), cube.get_links_ang()[rows])


def test_views_refuse_a_bad_link_or_env(pick_views):
    sc, sb, robot, cube, ref, B = pick_views
    with pytest.raises(IndexError):
        robot.get_jacobian(robot.n_links)
    with pytest.raises(IndexError):
        cube.get_links_vel(links_idx_local=[1])
    with pytest.raises(ValueError):
        cube.get_jacobian(robot.get_link("hand"))   # a link of another entity
    with pytest.raises(IndexError):
        robot.get_jacobian(0, envs_idx=[0, B])
    with pytest.raises(IndexError):
        robot.get_link("hand").get_vel(envs_idx=[-B - 1])
    with pytest.raises(ValueError):
        robot.get_jacobian(0, local_point=(0.0, 1.0))


# ---- the struct ------------------------------------------------------------------------------------------------------------------
def test_ctypes_mirror_of_the_query_struct_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mirigid.h"\n'
                   'int main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(MirKinQuery), offsetof(MirKinQuery, struct_size), offsetof(MirKinQuery, n_links),\n'
                   '         offsetof(MirKinQuery, link_body), offsetof(MirKinQuery, local_point), offsetof(MirKinQuery, dof0), offsetof(MirKinQuery, n_dofs), MIR_MAX_BODY);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    mine = [C.sizeof(MirKinQuery)] + [getattr(MirKinQuery, f).offset for f in ("struct_size", "n_links", "link_body", "local_point", "dof0", "n_dofs")] + [MIR_MAX_BODY]
    assert got == mine, (got, mine)
    q = make_kin_query([9, 12], [[0, 0, 0.1], [0.02, 0, 0]], dof0=9, n_dofs=6)
    assert q.struct_size == C.sizeof(MirKinQuery) and q.n_links == 2 and list(q.link_body[:2]) == [9, 12]
    assert abs(q.local_point[0][2] - 0.1) < 1e-7 and abs(q.local_point[1][0] - 0.02) < 1e-7 and (q.dof0, q.n_dofs) == (9, 6)
    with pytest.raises(ValueError):
        make_kin_query([])
    with pytest.raises(ValueError):
        make_kin_query(list(range(1, MIR_MAX_BODY + 2)))


def test_the_library_reports_the_same_struct_size():
    from gym_genesis.backend.lib import load_library

    lib = load_library()
    assert lib.mir_kin_query_sizeof() == C.sizeof(MirKinQuery)
