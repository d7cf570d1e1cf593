"""Operational-space dynamics (include/mirigid.h: mir_task_dynamics), CPU tier.

The float64 reference of tests/task_ref.py (the oracle's M and J, combined) is pinned from first principles:
  * M minv = I;
  * a free cube queried at its centre of mass: lambda = diag(m 1, R I_body R^T), the closed form of the spec;
  * J jbar = I at damping = 0; dynamic consistency J M^-1 (I - jbar J)^T = 0;
  * lambda with damping is the float64 inverse of lambda_inv + d^2 I;
  * the NaN rule: Franka link3 (three dofs on its path) is NaN at damping = 0 and finite at damping = 0.1, the hand is finite at 0;
  * the float32 port agrees with the float64 reference to float32 accuracy;
  * make_task_query validation and the struct's layout;
  * the EntityView methods on a test double that serves `task_dynamics` from the reference; forward_dynamics / inverse_dynamics
    round trip.
M minv = I, the consistency of J-bar (or the NaN rule) and the float32 port also on the synthetic trees of tests/tree_cases.py.
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
import task_ref
import tree_cases
from gym_genesis.backend import models
from gym_genesis.backend.spec import MIR_MAX_BODY, MIR_MAX_DOF, MirTaskQuery, make_task_query
from test_dyn_cpu import DynScene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 4
LP_HAND, LP_CUBE = (0.01, -0.02, 0.05), (0.015, -0.01, 0.02)


@pytest.fixture(scope="module")
def pick():
    sb = models.franka_cube_pick_scene()
    spec = sb.build()
    model = kin_ref.Model(spec)
    q, v = kin_ref.random_state(spec, model, B, seed=11)
    hand, link3, cube = sb.body_index("hand"), sb.body_index("link3"), sb.body_index("cube")
    x = np.random.default_rng(12).uniform(-2, 2, (B, model.nv))
    M, J = task_ref.oracle_mass_and_jacobian(spec, model, q, [hand, cube, link3, cube], [LP_HAND, LP_CUBE, (0, 0, 0), (0, 0, 0)])
    ref = task_ref.combine(M, J, x, 0.0)   # computed once, left unchanged
    return dict(sb=sb, spec=spec, model=model, q=q, v=v, x=x, M=M, J=J, ref=ref, hand=hand, link3=link3, cube=cube)


def test_minv_is_the_inverse_and_respects_the_trees(pick):
    M, ref = pick["M"], pick["ref"]
    nv = M.shape[1]
    err = np.abs(M @ ref["minv"] - np.eye(nv)).max()
    # cond(M) < 1e5 here (armature 0.1 against arm inertias of a few kg m^2, cube inertias of 1e-6): 1e5 x 2^-52 x a few
    assert err < 1e-9, err
    assert (ref["minv"][:, 0:9, 9:15] == 0).all() and (ref["minv"][:, 9:15, 0:9] == 0).all()
    assert np.array_equal(ref["minv"], ref["minv"].transpose(0, 2, 1))
    assert np.abs(np.einsum("bij,bj->bi", M, ref["solve"]) - pick["x"]).max() < 1e-9


def test_free_cube_at_its_centre_of_mass_has_the_closed_form_inertia(pick):
    spec, ref, cube = pick["spec"], pick["ref"], pick["cube"]
    m = float(np.float32(spec.body[cube].mass))
    ib = np.asarray(list(spec.body[cube].inertia), np.float32).astype(np.float64)
    I = np.array([[ib[0], ib[3], ib[4]], [ib[3], ib[1], ib[5]], [ib[4], ib[5], ib[2]]])
    assert not np.any(np.asarray(list(spec.body[cube].ipos))), "the cube's centre of mass is its origin"
    qa = pick["model"].qadr[cube]
    for b in range(B):
        R = kin_ref.quat_to_mat(pick["q"][b, qa + 3:qa + 7].astype(np.float64) / np.linalg.norm(pick["q"][b, qa + 3:qa + 7].astype(np.float64)))
        want = np.zeros((6, 6))
        want[0:3, 0:3], want[3:6, 3:6] = m * np.eye(3), R @ I @ R.T
        got = ref["lambda"][b, 3]
        assert np.allclose(got, want, rtol=1e-9, atol=1e-12 * m), (b, np.abs(got - want).max())
    # away from the centre of mass the linear and angular parts couple
    assert np.abs(ref["lambda"][:, 1, 0:3, 3:6]).max() > 1e-6


def test_jbar_is_a_dynamically_consistent_inverse(pick):
    M, J, ref = pick["M"], pick["J"], pick["ref"]
    minv = ref["minv"]
    for l in (0, 1, 3):
        Jl, jb = J[:, l], ref["jbar"][:, l]
        assert np.isfinite(jb).all()
        scale = np.abs(Jl).max() * np.abs(jb).max()
        assert np.abs(Jl @ jb - np.eye(6)).max() < 1e-8 * max(1.0, scale), l
        N = np.eye(M.shape[1]) - jb @ Jl
        cons = Jl @ minv @ N.transpose(0, 2, 1)
        assert np.abs(cons).max() < 1e-8 * np.abs(Jl @ minv).max() * max(1.0, np.abs(N).max()), (l, np.abs(cons).max())
        assert np.allclose(ref["lambda_inv"][:, l], Jl @ minv @ Jl.transpose(0, 2, 1), rtol=1e-10, atol=1e-12)


def test_damped_lambda_is_the_inverse_of_lambda_inv_plus_d2(pick):
    d = 0.1
    damped = task_ref.combine(pick["M"], pick["J"], None, d)
    assert np.array_equal(damped["lambda_inv"], pick["ref"]["lambda_inv"])
    for l in range(4):
        A = damped["lambda_inv"][:, l] + d * d * np.eye(6)
        assert np.isfinite(damped["lambda"][:, l]).all()
        assert np.allclose(damped["lambda"][:, l], np.linalg.inv(A), rtol=1e-8, atol=1e-10), l
        assert np.allclose(damped["jbar"][:, l], pick["ref"]["minv"] @ pick["J"][:, l].transpose(0, 2, 1) @ np.linalg.inv(A), rtol=1e-8, atol=1e-10)


def test_nan_rule(pick):
    ref = pick["ref"]
    assert np.isnan(ref["lambda"][:, 2]).all() and np.isnan(ref["jbar"][:, 2]).all(), "link3 has three dofs on its path"
    assert np.isfinite(ref["lambda_inv"]).all()
    assert (ref["relpivot"][:, 2] < 1e-6).all(), ref["relpivot"][:, 2]
    assert np.isfinite(ref["lambda"][:, 0]).all() and np.isfinite(ref["jbar"][:, 0]).all(), "the hand has seven"
    assert (ref["relpivot"][:, [0, 1, 3]] > task_ref.PIVOT).all()
    damped = task_ref.combine(pick["M"], pick["J"], None, 0.1)
    assert np.isfinite(damped["lambda"]).all() and np.isfinite(damped["jbar"]).all()
    assert (damped["relpivot"] > task_ref.PIVOT).all()
    # the rule itself, on a matrix whose pivots are known: diag(1, 1, 1, 1, 1, p)
    for p, ok in ((2e-5, True), (1e-5, False), (0.0, False), (-1.0, False)):
        A = np.diag([1.0, 1, 1, 1, 1, p])[None]
        assert (task_ref.relative_pivots(A)[0] > task_ref.PIVOT) == ok, p


def test_float32_port_agrees_with_the_reference_to_float32_accuracy(pick):
    """cond(M) ~ 1e4 and cond(lambda_inv) up to ~1e4 at the hand: a float32 walk is expected within cond x 2^-24 x a few, relative to the
    largest entry; 2e-2 is two orders above that and two below a wrong formula."""
    hand, cube = pick["hand"], pick["cube"]
    port = task_ref.oracle_task_dynamics(pick["spec"], pick["model"], pick["q"], [hand, cube], [LP_HAND, LP_CUBE], x=pick["x"], damping=0.05, f32=True)
    ref = task_ref.oracle_task_dynamics(pick["spec"], pick["model"], pick["q"], [hand, cube], [LP_HAND, LP_CUBE], x=pick["x"], damping=0.05)
    for k in task_ref.OUTS:
        if k in ("minv", "solve"):
            assert np.abs(port[k] - ref[k]).max() < 2e-2 * np.abs(ref[k]).max(), k
        else:
            for l in range(2):
                assert np.abs(port[k][:, l] - ref[k][:, l]).max() < 2e-2 * np.abs(ref[k][:, l]).max(), (k, l)
    assert not np.array_equal(port["minv"], ref["minv"])


# ---- the same pins on the synthetic trees of tests/tree_cases.py --------------------------------------------------------------------------
LP_TREE = (0.03, -0.02, 0.05)
_trees = {}


def _tree(name):
    """state at seed 3, x, and per case the two deepest links with >= 6 dofs on their path (bushy has none: its deepest two)"""
    if name not in _trees:
        sb, spec = tree_cases.build(name)
        model = kin_ref.Model(spec)
        q, v = kin_ref.random_state(spec, model, B, seed=3)
        x = np.random.default_rng(12).uniform(-2, 2, (B, model.nv))
        links = tree_cases.links_on_long_paths(model)[:2] or [model.nbody - 1, model.nbody - 2]
        M, J = task_ref.oracle_mass_and_jacobian(spec, model, q, links, LP_TREE)
        _trees[name] = dict(spec=spec, model=model, q=q, x=x, links=links, M=M, J=J, ref=task_ref.combine(M, J, x, 0.0))   # computed once, left unchanged
    return _trees[name]


@pytest.mark.parametrize("name", tree_cases.CASES)
def test_trees_minv_is_the_inverse_and_respects_the_trees(name):
    """The pick bar is the absolute 1e-9 for cond(M) < 1e5 and entries of M^-1 up to 3e5.  Here it is relative to the float64 magnitudes:
    |M minv - I| <= cond(M) x 2^-52 x a few, so 16 cond(M) 2^-52 (`many` holds a 4 cm cube beside 3 kg bodies: cond(M) ~ 3e6)."""
    t = _tree(name)
    M, ref, model = t["M"], t["ref"], t["model"]
    nv = model.nv
    bar = 16.0 * np.linalg.cond(M).max() * 2.0 ** -52
    err = np.abs(M @ ref["minv"] - np.eye(nv)).max()
    print(f"\n[task, {name}] max |M minv - I| {err:.3e}, bar {bar:.3e} (cond {np.linalg.cond(M).max():.3g})")
    assert err < bar, (err, bar)
    root = [0] * model.nbody
    for b in range(1, model.nbody):
        root[b] = b if model.parent[b] == 0 else root[model.parent[b]]
    tree = np.array([root[max(b for b in range(model.nbody) if model.dofadr[b] <= d and model.jtype[b] != kin_ref.FIXED)] for d in range(nv)])
    cross = tree[:, None] != tree[None, :]
    assert cross.any() == (name == "many") and (ref["minv"][:, cross] == 0).all()
    assert np.array_equal(ref["minv"], ref["minv"].transpose(0, 2, 1))
    scale = np.abs(ref["solve"]).max()
    assert np.abs(np.einsum("bij,bj->bi", M, ref["solve"]) - t["x"]).max() < bar * max(1.0, scale)


@pytest.mark.parametrize("name", tree_cases.CASES)
def test_trees_jbar_is_a_dynamically_consistent_inverse_or_nan(name):
    t = _tree(name)
    M, J, ref = t["M"], t["J"], t["ref"]
    minv = ref["minv"]
    assert np.isfinite(ref["lambda_inv"]).all()
    for l in range(2):
        Jl, jb = J[:, l], ref["jbar"][:, l]
        assert np.allclose(ref["lambda_inv"][:, l], Jl @ minv @ Jl.transpose(0, 2, 1), rtol=1e-10, atol=1e-12)
        if name == "bushy":   # four dofs on every path: the rule of the header, on links other than the Panda's link3
            assert np.isnan(jb).all() and np.isnan(ref["lambda"][:, l]).all() and (ref["relpivot"][:, l] < 1e-6).all()
            continue
        assert np.isfinite(jb).all() and (ref["relpivot"][:, l] > 1e-4).all(), ref["relpivot"][:, l]
        scale = np.abs(Jl).max() * np.abs(jb).max()
        assert np.abs(Jl @ jb - np.eye(6)).max() < 1e-8 * max(1.0, scale), l
        N = np.eye(M.shape[1]) - jb @ Jl
        cons = Jl @ minv @ N.transpose(0, 2, 1)
        assert np.abs(cons).max() < 1e-8 * np.abs(Jl @ minv).max() * max(1.0, np.abs(N).max()), (l, np.abs(cons).max())
    damped = task_ref.combine(M, J, None, 0.05)
    assert np.isfinite(damped["lambda"]).all() and np.isfinite(damped["jbar"]).all() and (damped["relpivot"] > 1e-4).all()


@pytest.mark.parametrize("name", tree_cases.CASES)
def test_trees_float32_port_agrees_with_the_reference_to_float32_accuracy(name):
    """The bar of the pick test, 2e-2 of the largest entry; minv and solve per tree (tests/tree_metrics.py), never pooled: in `many`
    the cube's rotational block of M^-1 is 3e5, the chain's a few."""
    import tree_metrics

    t = _tree(name)
    f32 = "big" if name == "many" else True
    port = task_ref.oracle_task_dynamics(t["spec"], t["model"], t["q"], t["links"], LP_TREE, x=t["x"], damping=0.05, f32=f32)
    ref = task_ref.oracle_task_dynamics(t["spec"], t["model"], t["q"], t["links"], LP_TREE, x=t["x"], damping=0.05)
    for label, idx in tree_metrics.dof_groups(t["model"]):
        for lb, jdx in tree_metrics.dof_groups(t["model"]):
            if label[0] == lb[0]:
                blk = lambda a: a[:, idx[:, None], jdx[None, :]]  # noqa: E731
                assert np.abs(blk(port["minv"]) - blk(ref["minv"])).max() <= 2e-2 * np.abs(blk(ref["minv"])).max(), (label, lb)
        assert np.abs(port["solve"][:, idx] - ref["solve"][:, idx]).max() < 2e-2 * np.abs(ref["solve"][:, idx]).max(), label
    for k in ("lambda_inv", "lambda", "jbar"):
        if name == "bushy" and k != "lambda_inv":
            continue   # (damping 0.05 leaves that 6 x 6 at a relative pivot of ~1e-4: conditioning, not the formulas)
        for l in range(2):
            assert np.abs(port[k][:, l] - ref[k][:, l]).max() < 2e-2 * np.abs(ref[k][:, l]).max(), (k, l)
    assert not np.array_equal(port["minv"], ref["minv"])


# ---- the struct ------------------------------------------------------------------------------------------------------------------
def test_make_task_query_validation_and_struct_layout(tmp_path):
    fields = ("struct_size", "n_links", "link_body", "local_point", "dof0", "n_dofs", "damping", "flags")
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mirigid.h"\nint main(void) {\n  printf("%zu", sizeof(MirTaskQuery));\n'
                   + "".join(f'  printf(" %zu", offsetof(MirTaskQuery, {f}));\n' for f in fields) + '  printf(" %d\\n", MIR_MAX_BODY);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    mine = [C.sizeof(MirTaskQuery)] + [getattr(MirTaskQuery, f).offset for f in fields] + [MIR_MAX_BODY]
    assert got == mine, (got, mine)
    q = make_task_query([8, 11], [[1, 2, 3], [4, 5, 6]], 9, 6, 0.25)
    assert (q.struct_size, q.n_links, q.dof0, q.n_dofs, q.damping, q.flags) == (C.sizeof(MirTaskQuery), 2, 9, 6, 0.25, 0)
    assert list(q.link_body[:2]) == [8, 11] and list(q.local_point[1]) == [4.0, 5.0, 6.0]
    assert list(make_task_query([3], (1, 2, 3)).local_point[0]) == [1.0, 2.0, 3.0]
    empty = make_task_query()
    assert (empty.n_links, empty.n_dofs, empty.damping) == (0, 0, 0.0)
    bad = [dict(links=[1] * (MIR_MAX_BODY + 1)), dict(links=[0]), dict(links=[-1]), dict(dof0=-1), dict(n_dofs=-1), dict(dof0=MIR_MAX_DOF, n_dofs=1),
           dict(damping=-0.1), dict(damping=float("nan")), dict(damping=float("inf")), dict(flags=1), dict(flags=1 << 31),
           dict(links=[1], local_points=[float("nan"), 0, 0]), dict(links=[1, 2], local_points=[[0, 0, 0]]), dict(links=[1], local_points=[0, 0])]
    for kw in bad:
        with pytest.raises(ValueError):
            make_task_query(**kw)


def test_the_library_reports_the_same_struct_size():
    from gym_genesis.backend.lib import load_library

    assert load_library().mir_task_query_sizeof() == C.sizeof(MirTaskQuery)


# ---- the views on a test double -------------------------------------------------------------------------------------------------
class TaskScene(DynScene):
    """DynScene with MirScene.task_dynamics served by the float64 reference"""

    def task_dynamics(self, links=(), local_points=None, env_idx=None, dof0=0, n_dofs=None, qpos=None, x=None, damping=0.0, minv=False,
                      solve=False, lambda_inv=None, lambda_=None, jbar=None):
        nd = self.nv - dof0 if n_dofs is None else n_dofs
        make_task_query(links, local_points, dof0, nd, damping)   # (the argument checks of the product)
        lambda_inv, lambda_, jbar = (bool(len(links)) if w is None else bool(w) for w in (lambda_inv, lambda_, jbar))
        envs = np.arange(self.num_envs) if env_idx is None else self._np(env_idx).reshape(-1)
        q = self.o.state()[0][envs] if qpos is None else self._np(qpos).astype(np.float64)
        r = task_ref.oracle_task_dynamics(self.spec, kin_ref.Model(self.spec), q, links, local_points, x=None if x is None else self._np(x), damping=damping)
        self.task_launches = getattr(self, "task_launches", 0) + 1
        self.last_x = None if x is None else self._np(x).copy()
        w = slice(dof0, dof0 + nd)
        pick = dict(minv=lambda a: a[:, w, w], solve=lambda a: a[:, w], lambda_inv=lambda a: a, jbar=lambda a: a[:, :, w, :])
        pick["lambda"] = pick["lambda_inv"]
        want = dict(minv=minv, solve=solve, lambda_inv=lambda_inv, jbar=jbar)
        want["lambda"] = lambda_
        return {k: torch.from_numpy(np.ascontiguousarray(pick[k](r[k]).astype(np.float32))) for k in task_ref.OUTS if want[k]}


@pytest.fixture(scope="module")
def views(pick):
    from gym_genesis.tasks.views import EntityView

    sb, spec = pick["sb"], pick["spec"]
    sc = TaskScene(spec, B)
    tgt, qacc = dyn_ref.random_targets_and_acc(spec, pick["q"], pick["v"], seed=13)
    sc.o.write_all(orc.F_QPOS, pick["q"].astype(np.float64))
    sc.o.write_all(orc.F_QVEL, pick["v"].astype(np.float64))
    sc.o.set_targets(tgt)
    robot = EntityView(sc, sb, root="link0", dof_names=models.FRANKA_JOINTS)
    cube = EntityView(sc, sb, root="cube", dof_names=())
    return sc, robot, cube, qacc


def test_views_shapes_and_entity_windows(pick, views):
    sc, robot, cube, qacc = views
    ref = pick["ref"]
    Mi = robot.get_mass_mat_inv()
    assert Mi.shape == (B, 9, 9) and Mi.dtype == torch.float32 and np.allclose(Mi.numpy(), ref["minv"][:, 0:9, 0:9], rtol=1e-6, atol=1e-7)
    Mc = cube.get_mass_mat_inv()
    assert Mc.shape == (B, 6, 6) and np.allclose(Mc.numpy(), ref["minv"][:, 9:15, 9:15], rtol=1e-6)
    assert torch.equal(robot.get_mass_mat_inv(envs_idx=[3, 0, 0]), Mi[[3, 0, 0]])
    y = robot.mass_mat_solve(pick["x"][:, 0:9])
    assert y.shape == (B, 9) and sc.last_x.shape == (B, 15) and not sc.last_x[:, 9:].any()
    assert np.allclose(y.numpy(), ref["solve"][:, 0:9], rtol=1e-5, atol=1e-6)
    assert torch.equal(robot.mass_mat_solve(pick["x"][:, 0:9], qpos=pick["q"][:, 0:9]), y)
    n0 = sc.task_launches
    op = robot.operational_space(robot.get_link("hand"), local_point=LP_HAND)
    assert sc.task_launches == n0 + 1, "one launch"
    assert op["lambda_inv"].shape == (B, 6, 6) and op["lambda"].shape == (B, 6, 6) and op["jbar"].shape == (B, 9, 6)
    for k in ("lambda_inv", "lambda"):
        assert np.allclose(op[k].numpy(), ref[k][:, 0], rtol=1e-5, atol=1e-6), k
    assert np.allclose(op["jbar"].numpy(), ref["jbar"][:, 0, 0:9], rtol=1e-5, atol=1e-6)
    assert torch.equal(robot.get_operational_inertia(robot.get_link("hand"), LP_HAND), op["lambda"])
    assert torch.equal(robot.get_jacobian_dyn_inverse(robot.get_link("hand"), LP_HAND, envs_idx=[2]), op["jbar"][[2]])
    sing = robot.operational_space(robot.get_link("link3"))
    assert torch.isnan(sing["lambda"]).all() and torch.isnan(sing["jbar"]).all() and torch.isfinite(sing["lambda_inv"]).all()
    assert torch.isfinite(robot.get_operational_inertia(robot.get_link("link3"), damping=0.1)).all()
    oc = cube.operational_space(0, local_point=LP_CUBE)
    assert oc["jbar"].shape == (B, 6, 6) and np.allclose(oc["lambda"].numpy(), ref["lambda"][:, 1], rtol=1e-5, atol=1e-9)
    with pytest.raises(ValueError):
        robot.operational_space(cube.get_link("cube"))
    with pytest.raises(ValueError):
        robot.mass_mat_solve(pick["x"][:, 0:8])
    with pytest.raises(ValueError):
        robot.get_operational_inertia(robot.get_link("hand"), damping=-1.0)
    with pytest.raises(IndexError):
        robot.get_mass_mat_inv(envs_idx=[0, B])
    with pytest.raises(NotImplementedError):
        cube.mass_mat_solve(pick["x"][:, 9:15], qpos=pick["q"][:, 9:15])
    with pytest.raises(NotImplementedError, match="decompose"):
        robot.get_mass_mat(decompose=True)


def test_a_scene_without_the_entry_point_raises_not_implemented(pick):
    from gym_genesis.tasks.views import EntityView

    robot = EntityView(DynScene(pick["spec"], 1), pick["sb"], root="link0", dof_names=models.FRANKA_JOINTS)
    for call in (lambda: robot.get_mass_mat_inv(), lambda: robot.operational_space(robot.get_link("hand")), lambda: robot.mass_mat_solve(np.zeros((1, 9)))):
        with pytest.raises(NotImplementedError, match="mir_task_dynamics"):
            call()


def test_forward_dynamics_inverts_inverse_dynamics(pick, views):
    sc, robot, cube, qacc = views
    tau = robot.inverse_dynamics(qacc[:, 0:9])
    n_dyn, n_task = sc.dyn_launches, sc.task_launches
    back = robot.forward_dynamics(tau)
    assert (sc.dyn_launches, sc.task_launches) == (n_dyn + 1, n_task + 1), "two launches"
    # float32 tensors on both legs: cond(M) ~ 1e4 x 2^-24 x |qacc| <= 2 -> 1e-3
    assert back.shape == (B, 9) and np.abs(back.numpy() - qacc[:, 0:9]).max() < 2e-3
    q2, v2 = kin_ref.random_state(pick["spec"], pick["model"], B, seed=14)
    tau2 = robot.inverse_dynamics(qacc[:, 0:9], qpos=q2[:, 0:9], qvel=v2[:, 0:9])
    back2 = robot.forward_dynamics(tau2, qpos=q2[:, 0:9], qvel=v2[:, 0:9])
    assert np.abs(back2.numpy() - qacc[:, 0:9]).max() < 2e-3 and not torch.equal(tau2, tau)
    rows = robot.forward_dynamics(tau[[3, 1]], envs_idx=[3, 1])
    assert np.allclose(rows.numpy(), back.numpy()[[3, 1]], rtol=1e-6, atol=1e-6)
    cb = cube.forward_dynamics(cube.inverse_dynamics(qacc[:, 9:15]))
    assert np.abs(cb.numpy() - qacc[:, 9:15]).max() < 2e-3
