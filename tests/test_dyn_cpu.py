"""Rigid-body dynamics queries (include/mirigid.h: mir_dynamics), CPU tier.

The float64 reference of tests/dyn_ref.py (the oracle's M, qfrc_bias, qfrc_act) is pinned from first principles:
  * gravity = bias at qvel = 0 equals central differences of the potential energy V(q) = -sum_b m_b g . xipos_b over every scalar dof
    (free dofs perturbed by the integrator's rule, as tests/test_kin_cpu.py does);
  * 1/2 qvel^T (M - diag(armature)) qvel equals the sum of the bodies' kinetic energies, 1/2 m |v_com|^2 + 1/2 w^T (R I R^T) w, from
    the velocities of tests/kin_ref.py at the centres of mass.  kin_ref gives the linear velocity of any point of a link, its angular
    velocity and its orientation, so the rotational term is covered for every body (full 3 x 3 body inertias, from the spec);
  * entries of M that couple different kinematic trees are exact zeros; M is symmetric;
  * make_dyn_query validation and the struct's layout;
  * the EntityView methods on a test double that serves `dynamics` from the reference.
The first three also on the synthetic trees of tests/tree_cases.py.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import dyn_ref
import kin_ref
import orc
import tree_cases
from fake_scene import OracleScene
from gym_genesis.backend import models
from gym_genesis.backend.spec import MIR_MAX_DOF, MirDynQuery, make_dyn_query

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scene(name):
    if name in tree_cases.CASES:
        return tree_cases.build(name)
    sb = models.franka_cube_pick_scene() if name == "pick" else models.franka_cube_stack_scene()
    return sb, sb.build()


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


def _f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def _masses(spec):
    return np.array([float(_f32(spec.body[b].mass)) if b else 0.0 for b in range(spec.nbody)])


def _delta(spec, model):
    """sum over the jointed bodies of | |float32(quat_b)|^2 - 1 |: how far the oracle's un-normalised frame products are from rotations
    (tests/test_kin_cpu.py derives the term)"""
    return sum(abs(float((_f32(list(spec.body[b].quat)) ** 2).sum()) - 1.0) for b in range(1, spec.nbody) if model.jtype[b] != kin_ref.FREE)


def _potential(o, spec, q, mass, g):
    o.write(orc.F_QPOS, q)
    o.fk()
    xi = o.read(orc.F_XIPOS).reshape(-1, 3)
    return -float((mass[:, None] * xi * g[None, :]).sum())


@pytest.mark.parametrize("scene", ["pick", "stack", *tree_cases.CASES])
def test_gravity_force_equals_central_differences_of_the_potential_energy(scene):
    """eps = 3e-5.  Truncation: eps^2 / 6 x the third derivative of V along one dof, at most W = sum m |g| x the lever arm (< 2 m):
    1.5e-10 W.  Round-off: V is a sum of < 32 terms, each from a forward-kinematics chain of < 200 float64 operations, on magnitudes
    < W: 200 x 2^-53 x W = 2.2e-14 W per evaluation, 2 evaluations divided by 2 eps: 7.4e-10 W.  Together < 1e-9 W.  The model term:
    the oracle's frames are products of float32-rounded quaternions that are not normalised (orc_fk), so its rotation matrices are
    rotations to within 2 delta per entry; the Newton-Euler recursion treats the motion subspaces as rigid, the differenced potential
    follows the oracle's map: 3 entries x 2 delta x W = 6 delta W (12 delta x the lever arm in tests/test_kin_cpu.py)."""
    eps = 3e-5
    sb, spec = _scene(scene)
    model = kin_ref.Model(spec)
    o = orc.Oracle(spec, 1)
    q0, v0 = kin_ref.random_state(spec, model, 1, seed=5)
    ref = dyn_ref.oracle_dynamics(o, q0, v0)
    q0 = q0[0].astype(np.float64)
    mass, g = _masses(spec), _f32(list(spec.opt.gravity))
    W = float(mass.sum() * np.linalg.norm(g) * 2.0)
    bound = (1e-9 + 6.0 * _delta(spec, model)) * W
    fd = np.array([(_potential(o, spec, _perturb(model, q0, d, eps), mass, g) - _potential(o, spec, _perturb(model, q0, d, -eps), mass, g)) / (2 * eps)
                   for d in range(model.nv)])
    err = float(np.abs(ref["gravity"][0] - fd).max())
    print(f"\n[dyn, {scene}] max |gravity - dV/dq| {err:.3e}, bound {bound:.3e} (W {W:.1f}, largest force {np.abs(fd).max():.2f})")
    assert err < bound, (scene, err, bound)
    assert np.abs(fd).max() > 1.0
    # a free body's holding force is its weight, upwards; nothing else
    for b in range(1, spec.nbody):
        if model.jtype[b] == kin_ref.FREE and not any(model.parent[c] == b for c in range(spec.nbody)):
            d = model.dofadr[b]
            assert np.allclose(ref["gravity"][0, d:d + 3], -mass[b] * g, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("scene", ["pick", "stack", *tree_cases.CASES])
def test_kinetic_energy_of_the_mass_matrix_equals_the_sum_over_the_bodies(scene):
    """Both sides are float64 sums of < 1000 products: round-off < 1e-12 T.  The model term: kin_ref normalises a link's quaternion,
    the oracle's inertias and subspaces use the un-normalised product (rotation entries within 2 delta): the rotated inertia and the
    lever arms differ by a relative 4 delta, bounded with T itself."""
    sb, spec = _scene(scene)
    model = kin_ref.Model(spec)
    o = orc.Oracle(spec, 1)
    q0, v0 = kin_ref.random_state(spec, model, 1, seed=6)
    ref = dyn_ref.oracle_dynamics(o, q0, v0)
    arm = np.array([float(_f32(spec.dof[i].armature)) for i in range(model.nv)])
    v = v0[0].astype(np.float64)
    T_M = 0.5 * v @ (ref["mass"][0] - np.diag(arm)) @ v
    bodies = list(range(1, spec.nbody))
    lps = np.array([_f32(list(spec.body[b].ipos)) for b in bodies])
    k = kin_ref.oracle_kinematics(o, model, bodies, lps)
    T = 0.0
    for i, b in enumerate(bodies):
        ib = _f32(list(spec.body[b].inertia))
        I = np.array([[ib[0], ib[3], ib[4]], [ib[3], ib[1], ib[5]], [ib[4], ib[5], ib[2]]])
        R = kin_ref.quat_to_mat(k["quat"][0, i])
        vc, w = k["vel"][0, i, 0:3], k["vel"][0, i, 3:6]
        T += 0.5 * _masses(spec)[b] * vc @ vc + 0.5 * w @ (R @ I @ R.T) @ w
    bound = (1e-12 + 4.0 * _delta(spec, model)) * T
    print(f"\n[dyn, {scene}] kinetic energy: 1/2 v'Mv {T_M:.9f}, sum over bodies {T:.9f}, difference {abs(T - T_M):.3e}, bound {bound:.3e}")
    assert abs(T - T_M) < bound and T > 0.1


@pytest.mark.parametrize("scene", ["pick", "stack", *tree_cases.CASES])
def test_cross_tree_blocks_are_exact_zeros_and_m_is_symmetric(scene):
    sb, spec = _scene(scene)
    model = kin_ref.Model(spec)
    o = orc.Oracle(spec, 2)
    q, v = kin_ref.random_state(spec, model, 2, seed=7)
    M = dyn_ref.oracle_dynamics(o, q, v)["mass"]
    root = [0] * spec.nbody
    for b in range(1, spec.nbody):
        root[b] = b if model.parent[b] == 0 else root[model.parent[b]]
    tree = np.array([root[max(b for b in range(spec.nbody) if model.dofadr[b] <= d and model.jtype[b] != kin_ref.FIXED)] for d in range(model.nv)])
    cross = tree[:, None] != tree[None, :]
    if len(set(tree)) == 1:   # (a synthetic scene of one tree: no cross block, and M is dense where a path is shared)
        assert scene in tree_cases.CASES and scene != "many" and not cross.any()
    else:
        assert cross.any() and (M[:, cross] == 0.0).all()
    assert np.array_equal(M, M.transpose(0, 2, 1))
    assert (np.linalg.eigvalsh(M) > 0).all()


# ---- the struct ------------------------------------------------------------------------------------------------------------------
def test_make_dyn_query_validation_and_struct_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mirigid.h"\n'
                   'int main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %d\\n", sizeof(MirDynQuery), offsetof(MirDynQuery, struct_size), offsetof(MirDynQuery, dof0),\n'
                   '         offsetof(MirDynQuery, n_dofs), offsetof(MirDynQuery, flags), MIR_MAX_DOF);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    mine = [C.sizeof(MirDynQuery)] + [getattr(MirDynQuery, f).offset for f in ("struct_size", "dof0", "n_dofs", "flags")] + [MIR_MAX_DOF]
    assert got == mine, (got, mine)
    q = make_dyn_query(9, 6)
    assert (q.struct_size, q.dof0, q.n_dofs, q.flags) == (C.sizeof(MirDynQuery), 9, 6, 0)
    assert make_dyn_query().n_dofs == 0
    for bad in ((-1, 2, 0), (0, -1, 0), (MIR_MAX_DOF, 1, 0), (0, MIR_MAX_DOF + 1, 0), (0, 3, 1), (0, 3, 1 << 31)):
        with pytest.raises(ValueError):
            make_dyn_query(*bad)


def test_the_library_reports_the_same_struct_size():
    from gym_genesis.backend.lib import load_library

    assert load_library().mir_dyn_query_sizeof() == C.sizeof(MirDynQuery)


# ---- the views on a test double -------------------------------------------------------------------------------------------------
class DynScene(OracleScene):
    """OracleScene with MirScene.dynamics served by the reference (on a second oracle, so that the scene's own state stays put)"""

    def dynamics(self, env_idx=None, dof0=0, n_dofs=None, qpos=None, qvel=None, qacc=None, mass=True, bias=True, gravity=False, tau=False,
                 ctrl_force=False):
        nd = self.nv - dof0 if n_dofs is None else n_dofs
        make_dyn_query(dof0, nd)  # (the argument checks of the product)
        envs = np.arange(self.num_envs) if env_idx is None else self._np(env_idx).reshape(-1)
        q0, v0 = self.o.state()
        t0 = self.o.read_all(orc.F_TARGET, self.nv)
        q = q0[envs] if qpos is None else self._np(qpos).astype(np.float64)
        v = v0[envs] if qvel is None else self._np(qvel).astype(np.float64)
        o2 = orc.Oracle(self.spec, len(envs))
        o2.write_all(orc.F_TARGET, t0[envs])
        r = dyn_ref.oracle_dynamics(o2, q, v, qacc=None if qacc is None else self._np(qacc))
        self.dyn_launches = getattr(self, "dyn_launches", 0) + 1
        self.last_qacc = None if qacc is None else self._np(qacc).copy()
        want = dict(mass=mass, bias=bias, gravity=gravity, tau=tau, ctrl_force=ctrl_force)
        w = slice(dof0, dof0 + nd)
        return {n: torch.from_numpy(np.ascontiguousarray((r[n][:, w, w] if n == "mass" else r[n][:, w]).astype(np.float32))) for n in dyn_ref.OUTS if want[n]}


@pytest.fixture(scope="module")
def pick_views():
    from gym_genesis.tasks.views import EntityView

    sb = models.franka_cube_pick_scene()
    spec = sb.build()
    B = 5
    sc = DynScene(spec, B)
    model = kin_ref.Model(spec)
    q, v = kin_ref.random_state(spec, model, B, seed=9)
    tgt, qacc = dyn_ref.random_targets_and_acc(spec, q, v, seed=10)
    sc.o.write_all(orc.F_QPOS, q.astype(np.float64))
    sc.o.write_all(orc.F_QVEL, v.astype(np.float64))
    sc.o.set_targets(tgt)
    robot = EntityView(sc, sb, root="link0", dof_names=models.FRANKA_JOINTS)
    cube = EntityView(sc, sb, root="cube", dof_names=())
    ref = dyn_ref.oracle_dynamics(orc.Oracle(spec, B), q, v, targets=tgt, qacc=qacc)   # computed once, left unchanged
    return sc, robot, cube, ref, B, q, v, qacc


def test_views_shapes_and_entity_windows(pick_views):
    sc, robot, cube, ref, B, q, v, qacc = pick_views
    M = robot.get_mass_mat()
    assert M.shape == (B, 9, 9) and M.dtype == torch.float32
    assert np.allclose(M.numpy(), ref["mass"][:, 0:9, 0:9], rtol=1e-6, atol=1e-7)
    Mc = cube.get_mass_mat()
    assert Mc.shape == (B, 6, 6) and np.allclose(Mc.numpy(), ref["mass"][:, 9:15, 9:15], rtol=1e-6, atol=1e-9)
    m = float(np.float32(sc.spec.body[cube.root].mass))
    assert np.allclose(Mc.numpy()[:, 0:3, 0:3], m * np.eye(3), rtol=1e-6, atol=0)
    for fn, key in ((robot.get_dofs_bias_force, "bias"), (robot.get_dofs_gravity_force, "gravity"), (robot.get_dofs_control_force, "ctrl_force")):
        x = fn()
        assert x.shape == (B, 9) and np.allclose(x.numpy(), ref[key][:, 0:9], rtol=1e-6, atol=1e-6), key
        y = fn(dofs_idx_local=[8, 0, 3])
        assert y.shape == (B, 3) and torch.equal(y, x[:, [8, 0, 3]]), key
        z = fn(envs_idx=[4, 0, 0])
        assert z.shape == (3, 9) and torch.equal(z, x[[4, 0, 0]]), key
    assert cube.get_dofs_control_force().shape == (B, 6) and not cube.get_dofs_control_force().any(), "the cube has no actuators"
    assert np.allclose(cube.get_dofs_gravity_force().numpy()[:, 2], m * 9.81, rtol=1e-6)
    assert torch.equal(robot.get_mass_mat(envs_idx=torch.tensor([2, 1])), M[[2, 1]])
    with pytest.raises(NotImplementedError, match="decompose"):
        robot.get_mass_mat(decompose=True)
    with pytest.raises(IndexError):
        robot.get_dofs_bias_force(envs_idx=[0, B])


def test_views_inverse_dynamics_over_the_entitys_dofs(pick_views):
    sc, robot, cube, ref, B, q, v, qacc = pick_views
    # the robot's accelerations, the cube at zero acceleration: the cube's tree does not reach the robot's rows
    tau = robot.inverse_dynamics(qacc[:, 0:9])
    assert tau.shape == (B, 9)
    assert sc.last_qacc.shape == (B, 15) and np.array_equal(sc.last_qacc[:, 0:9], qacc[:, 0:9]) and not sc.last_qacc[:, 9:].any()
    want = np.einsum("bij,bj->bi", ref["mass"][:, 0:9, 0:9], qacc[:, 0:9].astype(np.float64)) + ref["bias"][:, 0:9]
    assert np.allclose(tau.numpy(), want, rtol=1e-6, atol=1e-5)
    assert torch.equal(robot.inverse_dynamics(qacc[:, 0:9], dofs_idx_local=[1, 2]), tau[:, [1, 2]])
    assert torch.equal(robot.inverse_dynamics(qacc[[3, 1], 0:9], envs_idx=[3, 1]), tau[[3, 1]])
    # zero acceleration: the bias force; the state's own values as overrides: the same numbers
    zero = robot.inverse_dynamics(np.zeros((B, 9), np.float32))
    assert torch.equal(zero, robot.get_dofs_bias_force())
    same = robot.inverse_dynamics(qacc[:, 0:9], qpos=q[:, 0:9], qvel=v[:, 0:9])
    assert torch.equal(same, tau)
    # at rest the bias is the gravity force
    rest = robot.inverse_dynamics(np.zeros((B, 9), np.float32), qvel=np.zeros((B, 9), np.float32))
    assert np.allclose(rest.numpy(), ref["gravity"][:, 0:9], rtol=1e-6, atol=1e-5)
    ct = cube.inverse_dynamics(qacc[:, 9:15])
    assert ct.shape == (B, 6)
    with pytest.raises(ValueError):
        robot.inverse_dynamics(qacc[:, 0:8])
    with pytest.raises(NotImplementedError):
        cube.inverse_dynamics(qacc[:, 9:15], qpos=q[:, 9:15])
