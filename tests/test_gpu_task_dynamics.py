"""Operational-space dynamics on the GPU (include/mirigid.h: mir_task_dynamics; views: get_mass_mat_inv, mass_mat_solve,
forward_dynamics, operational_space, get_operational_inertia, get_jacobian_dyn_inverse).

States are SET (set_state), not stepped to: the GPU, the float64 reference and its float32 port hold the same float32 bits.  B = 5 envs
(not a multiple of four: the last wave has clamped pairs), the Franka pick scene (16-lane model, nv = 15, the arm's tree and the cube's
in one wave) and the five-cube stack scene (wave-kernel model, nv = 39, six trees).  Links: the hand and a cube at a non-zero
local_point, and link3 -- three dofs on its path -- for the singular case.

  * parity against the float64 reference of tests/task_ref.py per (scene, output, link) -- never pooled over links: the cube's
    lambda_inv is ~1e4 times the arm's.  minv, solve, lambda_inv, jbar: max absolute error over the batch.  lambda: the residual
    max |lambda_gpu (lambda_inv_ref64 + d^2 I) - I| (the raw error of an inverse depends far more on the order of summation than the
    residual does).  Allowed: 4 x the same metric of the float32 port on the same states (the project's margin for a float32 kernel
    that sums in another order than the serial walk).  All figures printed.
    The singular rule is checked on the CPU in the setup: every non-singular case has its smallest float64 relative pivot above 1e-4,
    every singular one below 1e-6, so that float32 cannot land on the other side of the 1e-5 rule;
  * the NaN rule; rows by env index; windows, coverage, symmetry, cross-tree zeros, nullable outputs; the qpos override; agreement with
    mir_dynamics and mir_link_kinematics; through GenesisEnv; a read is invisible; the error returns.
The MIR_E_CAPACITY cases of the tree table (a tree of more than 16 bodies or 15 dofs, more than 20 trees) and a free joint below
another body are left out, as in tests/test_gpu_dynamics.py: the scene compilers refuse such scenes before they exist.  An output of
2^31 elements is reached with a row count alone (nothing is allocated: the call returns before it looks at a pointer).
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import dyn_ref
import kin_ref
import orc
import task_ref
import tree_metrics
from gym_genesis.backend import models
from gym_genesis.backend.spec import MIR_MAX_BODY, MirTaskQuery, make_task_query

pytestmark = pytest.mark.gpu

B = 5
OUTS = task_ref.OUTS
ALL = dict(minv=True, solve=True, lambda_inv=True, lambda_=True, jbar=True)
LPS = [(0.01, -0.02, 0.05), (0.015, -0.01, 0.02), (0.0, 0.0, 0.0)]   # hand, cube, link3
NAMES = ("hand", "cube", "link3")
DAMPINGS = (0.0, 0.1)
SEED = dict(pick=31, stack=32)
_cache = {}


def _residual(lam, lam_inv64, d):
    """max |lambda (lambda_inv_ref64 + d^2 I) - I| over the batch, float64 on the host"""
    return float(np.abs(lam @ (lam_inv64 + d * d * np.eye(6)) - np.eye(6)).max())


def _metrics(got, ref, d):
    """{(output, link name or None): metric} of `got` against the float64 reference; singular (row, link) pairs of the reference are
    left to the NaN test"""
    m = {("minv", None): float(np.abs(got["minv"] - ref["minv"]).max()), ("solve", None): float(np.abs(got["solve"] - ref["solve"]).max())}
    for l, nm in enumerate(NAMES):
        m[("lambda_inv", nm)] = float(np.abs(got["lambda_inv"][:, l] - ref["lambda_inv"][:, l]).max())
        if np.isnan(ref["lambda"][:, l]).all():
            continue
        m[("jbar", nm)] = float(np.abs(got["jbar"][:, l] - ref["jbar"][:, l]).max())
        m[("lambda", nm)] = _residual(got["lambda"][:, l], ref["lambda_inv"][:, l], d)
    return m


def _cpu_side(name):
    """scene, seeded state, the float64 reference and the float32 port per damping (computed once), the pivot condition"""
    sb = models.franka_cube_pick_scene() if name == "pick" else models.franka_cube_stack_scene()
    spec = sb.build()
    model = kin_ref.Model(spec)
    q, v = kin_ref.random_state(spec, model, B, seed=SEED[name])
    x = np.random.default_rng(SEED[name] + 100).uniform(-2.0, 2.0, (B, model.nv)).astype(np.float32)
    links = [sb.body_index("hand"), sb.body_index("cube" if name == "pick" else "cube_2"), sb.body_index("link3")]
    M, J = task_ref.oracle_mass_and_jacobian(spec, model, q, links, LPS)
    M32, J32 = task_ref.oracle_mass_and_jacobian(spec, model, q, links, LPS, f32=True if name == "pick" else "big")
    ref, port, yard = {}, {}, {}
    for d in DAMPINGS:
        ref[d] = task_ref.combine(M, J, x.astype(np.float64), d)
        port[d] = {k: np.asarray(a, np.float64) for k, a in task_ref.combine(M32, J32, x, d).items()}
        # (the singular rule cannot flip in float32: checked for every case, none left out)
        rp = ref[d]["relpivot"]
        sing = np.isnan(ref[d]["lambda"]).all(axis=(2, 3))
        assert (rp[~sing] > 1e-4).all() and (rp[sing] < 1e-6).all(), (name, d, rp)
        assert np.array_equal(sing, np.isnan(port[d]["lambda"]).all(axis=(2, 3)))
        assert sing[:, 2].all() == (d == 0.0) and not sing[:, 0:2].any(), "link3 alone is singular, without damping alone"
        yard[d] = _metrics(port[d], ref[d], d)
    return dict(sb=sb, spec=spec, model=model, q=q, v=v, x=x, links=links, ref=ref, port=port, yard=yard, M32=M32, J32=J32)


def _setup(name):
    if name in _cache:
        return _cache[name]
    from gym_genesis.backend.lib import MirScene

    s = _cpu_side(name)
    sc = MirScene(s["spec"], B)
    assert sc.kernel == (16 if name == "pick" else 64) and s["model"].nv == (15 if name == "pick" else 39)
    sc.set_state(qpos=s["q"], qvel=s["v"])
    s["sc"], s["x_d"] = sc, torch.as_tensor(s["x"], device=sc.device)
    s["full"] = {d: sc.task_dynamics(links=s["links"], local_points=LPS, x=s["x_d"], damping=d, **ALL) for d in DAMPINGS}
    _cache[name] = s
    return s


def _tree_of_dof(model):
    root = [0] * model.nbody
    for b in range(1, model.nbody):
        root[b] = b if model.parent[b] == 0 else root[model.parent[b]]
    return np.array([root[max(b for b in range(model.nbody) if model.dofadr[b] <= d and model.jtype[b] != kin_ref.FIXED)] for d in range(model.nv)])


@pytest.mark.parametrize("name", ["pick", "stack"])
def test_parity_with_the_float64_reference(name):
    """Figures of the first run on an MI355X: DESIGN.md, operational-space dynamics, measured errors."""
    s = _setup(name)
    nv = s["model"].nv
    bad = []
    for d in DAMPINGS:
        got = {k: a.cpu().numpy().astype(np.float64) for k, a in s["full"][d].items()}
        assert got["minv"].shape == (B, nv, nv) and got["solve"].shape == (B, nv) and got["jbar"].shape == (B, 3, nv, 6)
        assert got["lambda_inv"].shape == (B, 3, 6, 6) and got["lambda"].shape == (B, 3, 6, 6)
        e, yard = _metrics(got, s["ref"][d], d), s["yard"][d]
        assert set(e) == set(yard)
        for key in sorted(e, key=str):
            print(f"[task dynamics, {name}, damping {d}] {key[0]:>10} {str(key[1]):>5}: GPU {e[key]:.3e} port {yard[key]:.3e} allowed {4 * yard[key]:.3e}")
            if not e[key] <= 4.0 * yard[key]:
                bad.append((name, d, key, e[key], yard[key]))
        # minv and solve per kinematic tree and dof kind as well (tests/tree_metrics.py): pooled, a cube's rotational block of M^-1 (~3e5)
        # sets a yardstick of 0.07 .. 0.25 for the arm, whose entries are ~10 and whose own port error is ~1e-5
        t = f"task dynamics, {name}, damping {d}"
        bad += tree_metrics.report(f"{t}, minv", tree_metrics.matrix_blocks(s["model"], got["minv"], s["port"][d]["minv"], s["ref"][d]["minv"]))
        bad += tree_metrics.report(f"{t}, solve", tree_metrics.vector_blocks(s["model"], got["solve"], s["port"][d]["solve"], s["ref"][d]["solve"]))
    assert not bad, bad


@pytest.mark.parametrize("name", ["pick", "stack"])
def test_nan_rule(name):
    s = _setup(name)
    f0, f1 = s["full"][0.0], s["full"][0.1]
    assert torch.isnan(f0["lambda"][:, 2]).all() and torch.isnan(f0["jbar"][:, 2]).all(), "link3 has three dofs on its path"
    assert torch.isfinite(f0["lambda_inv"]).all() and torch.isfinite(f0["lambda"][:, 0:2]).all() and torch.isfinite(f0["jbar"][:, 0:2]).all()
    assert torch.isfinite(f0["minv"]).all() and torch.isfinite(f0["solve"]).all(), "nothing else is affected"
    for k in OUTS:
        assert torch.isfinite(f1[k]).all(), k
    # (link3's lambda_inv at damping 0 and everything of it at 0.1 are within their yardsticks: test_parity covers every key)
    assert ("lambda_inv", "link3") in s["yard"][0.0] and ("lambda", "link3") in s["yard"][0.1] and ("lambda", "link3") not in s["yard"][0.0]
    for k in ("minv", "solve", "lambda_inv"):
        assert torch.equal(f0[k], f1[k]), "damping reaches lambda and jbar only"


@pytest.mark.parametrize("name", ["pick", "stack"])
def test_rows_by_env_index_repeats_and_any_order(name):
    s = _setup(name)
    sc, full = s["sc"], s["full"][0.1]
    for idx in ([4, 0, 0, 3], [4, 3, 2, 1, 0], [2]):
        it = torch.tensor(idx, device=sc.device)
        rows = sc.task_dynamics(links=s["links"], local_points=LPS, env_idx=it, x=s["x_d"][idx].contiguous(), damping=0.1, **ALL)
        for k in OUTS:
            assert rows[k].shape[0] == len(idx) and torch.equal(rows[k], full[k][idx]), (name, k, idx)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _raw(sc, links, idx, dof0, nd, want, damping=0.0, qpos=None, x=None, offset=0, h=None, q=None, n_rows=None, alloc=True):
    """mir_task_dynamics into NaN-filled tensors (`offset` floats into a larger allocation: an unaligned output) -> (rc, tensors)"""
    q = make_task_query(links, LPS[:len(links)] if links else None, dof0, nd, damping) if q is None else q
    R, L = (sc.num_envs if idx is None else len(idx)), len(links)
    shapes = dict(minv=(R, nd, nd), solve=(R, nd), lambda_inv=(R, L, 6, 6), jbar=(R, L, nd, 6))
    shapes["lambda"] = shapes["lambda_inv"]
    out = {}
    for k in want:
        n = int(np.prod(shapes[k])) if alloc else 1
        out[k] = torch.full((n + offset,), float("nan"), device=sc.device)[offset:]
        out[k] = out[k].view(shapes[k]) if alloc else out[k]
    it = None if idx is None else torch.tensor(idx, dtype=torch.long, device=sc.device)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    rc = sc.lib.mir_task_dynamics(sc.h if h is None else h, None if q == "null" else C.byref(q), p(it), R if n_rows is None else n_rows, p(qpos), p(x),
                                  p(out.get("minv")), p(out.get("solve")), p(out.get("lambda_inv")), p(out.get("lambda")), p(out.get("jbar")), sc._stream())
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("name", ["pick", "stack"])
def test_windows_coverage_symmetry_and_cross_tree_zeros(name):
    s = _setup(name)
    sc, model, links = s["sc"], s["model"], s["links"]
    nv = model.nv
    for d in DAMPINGS:
        full = s["full"][d]
        rc, out = _raw(sc, links, None, 0, nv, OUTS, damping=d, x=s["x_d"])
        assert rc == 0
        for k in OUTS:
            assert torch.equal(_bits(out[k]), _bits(full[k])), k
            if d > 0:
                assert torch.isfinite(out[k]).all(), k
        Mi, Li = out["minv"], out["lambda_inv"]
        assert torch.equal(_bits(Mi), _bits(Mi.transpose(1, 2))), "minv bitwise symmetric"
        assert torch.equal(_bits(Li), _bits(Li.transpose(2, 3))), "lambda_inv bitwise symmetric"
        tree = _tree_of_dof(model)
        cross = torch.as_tensor(tree[:, None] != tree[None, :], device=sc.device)
        assert bool(cross.any()) and bool((Mi[:, cross] == 0.0).all())
        assert bool((Mi[:, ~cross].abs().amax(0) > 0).any())
    # sub-windows into NaN-filled outputs at addresses that are not 16-byte aligned: one that cuts the arm's tree, an odd one that cuts a
    # cube's six dofs, the last dof alone
    full = s["full"][0.1]
    for d0, nd, off in ((3, 4, 0), (7, 5, 1), (nv - 1, 1, 3), (9, 6, 0), (1, nv - 1, 1)):
        rc, part = _raw(sc, links, [4, 0, 0], d0, nd, OUTS, damping=0.1, x=s["x_d"][[4, 0, 0]].contiguous(), offset=off)
        assert rc == 0
        w = slice(d0, d0 + nd)
        want = dict(minv=full["minv"][[4, 0, 0]][:, w, w], solve=full["solve"][[4, 0, 0]][:, w], lambda_inv=full["lambda_inv"][[4, 0, 0]],
                    jbar=full["jbar"][[4, 0, 0]][:, :, w, :])
        want["lambda"] = full["lambda"][[4, 0, 0]]
        for k in OUTS:
            assert torch.isfinite(part[k]).all() and torch.equal(_bits(part[k]), _bits(want[k])), (name, k, d0, nd)
    # nullable outputs: each alone gives the same bits; a query without links serves minv / solve; none at all is MIR_OK without a launch
    for k in OUTS:
        rc, one = _raw(sc, links, None, 0, nv, (k,), damping=0.1, x=s["x_d"] if k == "solve" else None)
        assert rc == 0 and torch.equal(_bits(one[k]), _bits(full[k])), k
    rc, two = _raw(sc, [], None, 0, nv, ("minv", "solve"), x=s["x_d"])
    assert rc == 0 and torch.equal(_bits(two["minv"]), _bits(full["minv"])) and torch.equal(_bits(two["solve"]), _bits(full["solve"]))
    rc, none = _raw(sc, links, None, 0, nv, ())
    assert rc == 0
    rc, empty = _raw(sc, links, None, 5, 0, ("minv", "solve", "jbar"), x=s["x_d"], offset=1)   # an empty result: no launch, nothing read
    assert rc == 0
    n0 = sc.__dict__.get("task_dynamics_launches", 0)
    assert sc.task_dynamics(links=links, lambda_inv=False, lambda_=False, jbar=False) == {} and sc.task_dynamics() == {}
    assert sc.__dict__.get("task_dynamics_launches", 0) == n0


@pytest.mark.parametrize("name", ["pick", "stack"])
def test_qpos_override(name):
    from gym_genesis.backend.lib import MirScene

    s = _setup(name)
    sc, model, full = s["sc"], s["model"], s["full"][0.1]
    kw = dict(links=s["links"], local_points=LPS, damping=0.1, **ALL)
    before = [t.clone() for t in sc.get_state()]
    same = sc.task_dynamics(qpos=before[0], x=s["x_d"], **kw)
    for k in OUTS:
        assert torch.equal(_bits(same[k]), _bits(full[k])), k
    q2, v2 = kin_ref.random_state(s["spec"], model, B, seed=41)
    other = MirScene(s["spec"], B)
    other.set_state(qpos=q2, qvel=v2)
    want = other.task_dynamics(x=s["x_d"], **kw)
    got = sc.task_dynamics(qpos=torch.as_tensor(q2, device=sc.device), x=s["x_d"], **kw)
    for k in OUTS:
        assert torch.equal(_bits(got[k]), _bits(want[k])) and not torch.equal(_bits(got[k]), _bits(full[k])), k
    idx = [3, 3, 1]
    got = sc.task_dynamics(env_idx=torch.tensor(idx, device=sc.device), qpos=torch.as_tensor(q2[idx], device=sc.device), x=s["x_d"][idx].contiguous(), **kw)
    for k in OUTS:
        assert torch.equal(_bits(got[k]), _bits(want[k][idx])), k
    for a, b in zip(sc.get_state(), before):
        assert torch.equal(a, b), "an override changes nothing"
    other.close() if hasattr(other, "close") else None


@pytest.mark.parametrize("name", ["pick", "stack"])
def test_consistency_with_mir_dynamics_and_mir_link_kinematics(name):
    """minv mass = I with the mass of mir_dynamics, and J minv J^T = lambda_inv with the J of mir_link_kinematics, on the same state:
    the products in float64 on the host from the float32 results.  Each is allowed 4 x the same figure of the float32 port (its minv
    against the float32 oracle's M; its lambda_inv against J32 minv J32^T per link): the yardstick rule of the parity test."""
    s = _setup(name)
    sc, full, port = s["sc"], s["full"][0.0], s["port"][0.0]
    nv = s["model"].nv
    f64 = lambda t: t.cpu().numpy().astype(np.float64)  # noqa: E731
    mass = f64(sc.dynamics(mass=True, bias=False)["mass"])
    J = f64(sc.link_kinematics(s["links"], LPS, pos=False, quat=False, vel=False)["jac"])
    minv, M32, J32 = f64(full["minv"]), s["M32"].astype(np.float64), s["J32"].astype(np.float64)
    e = float(np.abs(minv @ mass - np.eye(nv)).max())
    y = float(np.abs(port["minv"] @ M32 - np.eye(nv)).max())
    print(f"\n[task dynamics, {name}] max |minv mass - I|: GPU {e:.3e} port {y:.3e} allowed {4 * y:.3e}")
    bad = [] if e <= 4 * y else [("minv mass", e, y)]
    for l, nm in enumerate(NAMES):
        e = float(np.abs(J[:, l] @ minv @ J[:, l].transpose(0, 2, 1) - f64(full["lambda_inv"][:, l])).max())
        y = float(np.abs(J32[:, l] @ port["minv"] @ J32[:, l].transpose(0, 2, 1) - port["lambda_inv"][:, l]).max())
        print(f"[task dynamics, {name}] max |J minv J^T - lambda_inv| at {nm}: GPU {e:.3e} port {y:.3e} allowed {4 * y:.3e}")
        if not e <= 4 * y:
            bad.append((nm, e, y))
    assert not bad, bad


def _grasp(n):
    G_ = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "grasp_targets.json")))
    T = np.array(G_["targets"], np.float32)
    return np.tile(np.repeat(T.transpose(1, 0, 2), G_["steps_per_stage"], axis=0), (1, n // 4, 1))


def test_through_genesis_env_against_the_reference_on_the_state_read_back():
    from gym_genesis.env import GenesisEnv

    n, d = 8, 0.05
    acts = _grasp(n)
    env = GenesisEnv(task="cube_pick", robot="franka", num_envs=n, enable_pixels=False)
    env.reset(seed=2)
    task = env._env
    mir, robot = task._mir, task.franka
    spec = mir.spec
    model = kin_ref.Model(spec)
    hand = robot.get_link("hand")
    o64, o32 = orc.Oracle(spec, n), orc.Oracle(spec, n, f32=True)
    A = torch.as_tensor(acts, device=mir.device)
    tau = np.random.default_rng(7).uniform(-5, 5, (n, 9)).astype(np.float32)
    keys = ("lambda_inv", "lambda", "jbar", "qacc")
    worst, yard = dict.fromkeys(keys, 0.0), dict.fromkeys(keys, 0.0)
    for t in range(20):
        env.step(A[20 * t % acts.shape[0]])
        op = robot.operational_space(hand, damping=d)
        qacc = robot.forward_dynamics(tau)
        assert op["lambda_inv"].shape == (n, 6, 6) and op["lambda"].shape == (n, 6, 6) and op["jbar"].shape == (n, 9, 6) and qacc.shape == (n, 9)
        q, v = (a.cpu().numpy() for a in mir.get_state()[:2])
        b64 = dyn_ref.oracle_dynamics(o64, q, v)["bias"]
        b32 = dyn_ref.oracle_dynamics(o32, q, v)["bias"].astype(np.float32)
        x64, x32 = np.zeros((n, 15)), np.zeros((n, 15), np.float32)
        x64[:, 0:9], x32[:, 0:9] = tau.astype(np.float64) - b64[:, 0:9], tau - b32[:, 0:9]
        ref = task_ref.oracle_task_dynamics(spec, model, q, [hand.idx], None, x=x64, damping=d)
        prt = task_ref.oracle_task_dynamics(spec, model, q, [hand.idx], None, x=x32, damping=d, f32=True)
        assert (ref["relpivot"] > 1e-4).all()
        got = {k: op[k].cpu().numpy().astype(np.float64) for k in op}
        for k, g, p, r in (("lambda_inv", got["lambda_inv"], prt["lambda_inv"][:, 0], ref["lambda_inv"][:, 0]),
                           ("jbar", got["jbar"], prt["jbar"][:, 0, 0:9], ref["jbar"][:, 0, 0:9]),
                           ("qacc", qacc.cpu().numpy().astype(np.float64), prt["solve"][:, 0:9], ref["solve"][:, 0:9])):
            worst[k], yard[k] = max(worst[k], float(np.abs(g - r).max())), max(yard[k], float(np.abs(p - r).max()))
        worst["lambda"] = max(worst["lambda"], _residual(got["lambda"], ref["lambda_inv"][:, 0], d))
        yard["lambda"] = max(yard["lambda"], _residual(prt["lambda"][:, 0], ref["lambda_inv"][:, 0], d))
    print("\n[task dynamics, GenesisEnv, 20 steps x 8 envs] " + "   ".join(f"{k}: GPU {worst[k]:.3e} port {yard[k]:.3e} allowed {4 * yard[k]:.3e}" for k in keys))
    for k in keys:
        assert worst[k] <= 4.0 * yard[k], (k, worst[k], yard[k])


def test_a_read_is_invisible():
    from gym_genesis.env import GenesisEnv

    n = 8
    acts = _grasp(n)
    envs = [GenesisEnv(task="cube_pick", robot="franka", num_envs=n, enable_pixels=False) for _ in range(2)]
    for e in envs:
        e.reset(seed=3)
    mirs = [e._env._mir for e in envs]
    sb = models.franka_cube_pick_scene()
    links = [sb.body_index("hand"), sb.body_index("cube"), sb.body_index("link3")]
    A = torch.as_tensor(acts, device=mirs[0].device)
    dev = lambda a: torch.as_tensor(a.astype(np.float32), device=mirs[0].device)  # noqa: E731
    q2, _ = kin_ref.random_state(mirs[0].spec, kin_ref.Model(mirs[0].spec), n, seed=9)
    kw = dict(links=links, local_points=LPS, qpos=dev(q2), x=dev(np.random.default_rng(8).uniform(-1, 1, (n, mirs[0].nv))), damping=0.05, **ALL)
    v0 = [m.state_version for m in mirs]
    counters = ("link_kinematics_launches", "raycast_launches", "contact_force_launches", "dynamics_launches", "link_accelerations_launches")
    for t in range(50):
        res = [e.step(A[8 * t % acts.shape[0]]) for e in envs]
        mirs[0].task_dynamics(**kw)
        for k in ("agent_pos", "environment_state"):
            assert torch.equal(res[0][0][k], res[1][0][k]), (t, k)
        assert torch.equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])
        for a, b in zip(mirs[0].get_state(), mirs[1].get_state()):   # qpos, qvel, targets, warm start
            assert torch.equal(a, b), t
        assert mirs[0].state_version - v0[0] == mirs[1].state_version - v0[1]
    K = 4
    stride = mirs[0].agent_dim + mirs[0].env_dim + 2
    rows = [torch.zeros((K, n, stride), device=m.device) for m in mirs]
    for call in range(2):
        a = A[100 + K * call:100 + K * (call + 1)].contiguous()
        for m, r in zip(mirs, rows):
            m.rollout_exact(a, r)
        mirs[0].task_dynamics(**kw)
        assert torch.equal(rows[0], rows[1]), call
        for a, b in zip(mirs[0].get_state(), mirs[1].get_state()):
            assert torch.equal(a, b), call
    assert mirs[0].task_dynamics_launches == 52
    assert [mirs[0].__dict__.get(k, 0) for k in counters] == [mirs[1].__dict__.get(k, 0) for k in counters], "the other queries' launch counters"
    assert mirs[1].__dict__.get("task_dynamics_launches", 0) == 0


def test_errors_name_the_entry_point_and_launch_nothing():
    from gym_genesis.backend.lib import MirError, MirScene

    s = _setup("pick")
    sc, nv, links = s["sc"], s["model"].nv, s["links"]
    mk = lambda: make_task_query(links, LPS, 0, nv, 0.0)  # noqa: E731
    go = lambda **kw: _raw(sc, links, None, 0, nv, OUTS, x=s["x_d"], **kw)  # noqa: E731
    bad = [go(q="null"), go(h=C.c_void_p(0))]
    q = mk(); q.struct_size -= 4; bad.append(go(q=q))
    for nl in (-1, MIR_MAX_BODY + 1):
        q = mk(); q.n_links = nl; bad.append(go(q=q))
    for b in (0, -1, sc.nbody):
        q = mk(); q.link_body[1] = b; bad.append(go(q=q))
    for val in (float("nan"), float("inf")):
        q = mk(); q.local_point[2][1] = val; bad.append(go(q=q))
    for val in (float("nan"), float("inf"), -0.5):
        q = mk(); q.damping = val; bad.append(go(q=q))
    for d0, nd in ((1, nv), (-1, 2), (0, -1), (nv + 1, 0)):
        q = mk(); q.dof0, q.n_dofs = d0, nd; bad.append(go(q=q))
    for bit in (1, 1 << 31):
        q = mk(); q.flags = bit; bad.append(go(q=q))
    bad.append(_raw(sc, links, None, 0, nv, OUTS))                                              # solve without x
    for k in ("lambda_inv", "lambda", "jbar"):                                                  # a link output without links
        bad.append(_raw(sc, [], None, 0, nv, (k,), alloc=False))
    for rc, out in bad:
        assert rc == -1 and b"mir_task_dynamics" in sc.lib.mir_last_error(), rc
        assert all(torch.isnan(a).all() for a in out.values()), "a refused call launches nothing"
    # an output of 2^31 elements, with a row count alone: each output by itself
    for k, per_row in (("minv", nv * nv), ("solve", nv), ("lambda_inv", 3 * 36), ("lambda", 3 * 36), ("jbar", 3 * nv * 6)):
        rc, out = _raw(sc, links, [0], 0, nv, (k,), x=s["x_d"], n_rows=(2 ** 31 - 1) // per_row + 1)
        assert rc == -2 and b"mir_task_dynamics" in sc.lib.mir_last_error() and torch.isnan(out[k]).all(), k
    # a link whose kinematic tree has no dofs: a body welded to the world beside a free cube
    sb = models.SceneBuilder()
    sb.add_geom(0, models.GEOM_PLANE)
    sb.add_body("post", 0, pos=(0.3, 0.0, 0.1), mass=1.0, inertia=models.box_inertia(1.0, (0.05, 0.05, 0.1)))
    sb.add_geom("post", models.GEOM_BOX, size=(0.05, 0.05, 0.1))
    models._add_cube(sb, "cube", (0.0, 0.0, 0.02))
    welded = MirScene(sb.build(), 2)
    rc, out = _raw(welded, [sb.body_index("post")], None, 0, welded.nv, ("lambda_inv",))
    assert rc == -1 and b"mir_task_dynamics" in welded.lib.mir_last_error() and b"no dofs" in welded.lib.mir_last_error()
    assert torch.isnan(out["lambda_inv"]).all()
    rc, out = _raw(welded, [sb.body_index("cube")], None, 0, welded.nv, ("lambda_inv",))
    assert rc == 0 and torch.isfinite(out["lambda_inv"]).all()
    welded.close() if hasattr(welded, "close") else None
    # between mir_step_begin and mir_step_end
    bufs = (sc.empty(sc.agent_dim), sc.empty(sc.env_dim), sc.empty(), sc.empty(dtype=torch.uint8))
    before = [a.clone() for a in sc.get_state()]
    n0 = sc.__dict__.get("task_dynamics_launches", 0)
    sc.step_begin(None, *bufs)
    rc, out = go()
    msg = sc.lib.mir_last_error()
    with pytest.raises(MirError, match="mir_task_dynamics.*pending"):
        sc.task_dynamics(minv=True)
    sc.step_end()
    assert rc == -1 and b"mir_task_dynamics" in msg and b"pending" in msg
    assert all(torch.isnan(a).all() for a in out.values()) and sc.__dict__.get("task_dynamics_launches", 0) == n0
    sc.set_state(*before)   # (the shared scene goes back to the state the other tests compare)
    assert C.sizeof(MirTaskQuery) == sc.lib.mir_task_query_sizeof()
    with pytest.raises(ValueError):
        sc.task_dynamics(solve=True)
    with pytest.raises(ValueError):
        sc.task_dynamics(lambda_=True)
