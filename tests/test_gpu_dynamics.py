"""Rigid-body dynamics queries on the GPU (include/mirigid.h: mir_dynamics; views: get_mass_mat, get_dofs_control_force,
get_dofs_bias_force, get_dofs_gravity_force, inverse_dynamics).

States are SET (set_state), not stepped to: the GPU, the float64 oracle and its float32 port hold the same float32 bits.  B = 5 envs
(not a multiple of four: the last wave has clamped pairs), the Franka pick scene (16-lane model, nv = 15) and the five-cube stack
scene (wave-kernel model, nv = 39).

  * parity: mass, bias, gravity, tau, ctrl_force against the float64 reference of tests/dyn_ref.py; metric = max absolute error per
    output over the batch; the GPU is allowed 4 x the same error of the oracle's float32 build on the same states (the margin of the
    kinematics and contact-force tests for a float32 kernel that sums in another order than the serial walk).  All figures printed;
  * rows by env index; windows, coverage, symmetry, cross-tree zeros; state overrides; agreement with mir_forward;
  * through GenesisEnv; a read is invisible; the error returns.
The MIR_E_CAPACITY cases of the tree table (a tree of more than 16 bodies or 15 dofs, more than 20 trees) are left out: the scene
compilers refuse such scenes before they exist.  R x n^2 >= 2^31 is reached with a row count alone (nothing is allocated: the call
returns before it looks at a pointer).
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
import tree_metrics
from gym_genesis.backend import models
from gym_genesis.backend.spec import MirDynQuery, make_dyn_query

pytestmark = pytest.mark.gpu

B = 5
OUTS = dyn_ref.OUTS
ALL = dict(mass=True, bias=True, gravity=True, tau=True, ctrl_force=True)
_cache = {}


def _setup(name):
    """scene with a seeded random state, targets and accelerations; the float64 reference and the float32 port, computed once"""
    if name in _cache:
        return _cache[name]
    from gym_genesis.backend.lib import MirScene

    sb = models.franka_cube_pick_scene() if name == "pick" else models.franka_cube_stack_scene()
    spec = sb.build()
    model = kin_ref.Model(spec)
    sc = MirScene(spec, B)
    assert sc.kernel == (16 if name == "pick" else 64) and model.nv == (15 if name == "pick" else 39)
    q, v = kin_ref.random_state(spec, model, B, seed=31 if name == "pick" else 32)
    tgt, qacc = dyn_ref.random_targets_and_acc(spec, q, v, seed=33 if name == "pick" else 34)
    # (checked here, on the CPU: no position-controlled dof sits within 1e-3 of its force range of a clamp limit)
    margin = dyn_ref.pd_margin(spec, q, v, tgt)
    assert margin.min() > 1e-3, margin.min()
    sc.set_state(qpos=q, qvel=v, target=tgt)
    ref = dyn_ref.oracle_dynamics(orc.Oracle(spec, B), q, v, targets=tgt, qacc=qacc)
    port = dyn_ref.oracle_dynamics(orc.Oracle(spec, B, f32=True if name == "pick" else "big"), q, v, targets=tgt, qacc=qacc, f32=True)
    ctrl = [i for i in range(spec.ndof) if spec.dof[i].ctrl_mode == 1]
    hi = np.array([float(np.float32(spec.dof[i].frc_range[1])) for i in ctrl])
    at_limit = np.abs(ref["ctrl_force"][:, ctrl]) == hi[None, :]
    assert at_limit.any() and not at_limit.all(), "some dofs clamp, some do not"
    yard = {k: float(np.abs(port[k] - ref[k]).max()) for k in OUTS}
    dev = lambda a: torch.as_tensor(a, device=sc.device)  # noqa: E731
    _cache[name] = dict(sb=sb, spec=spec, model=model, sc=sc, q=q, v=v, tgt=tgt, qacc=qacc, ref=ref, port=port, yard=yard,
                        qacc_d=dev(qacc), full=sc.dynamics(qacc=dev(qacc), **ALL))
    return _cache[name]


def _tree_of_dof(model):
    root = [0] * model.nbody
    for b in range(1, model.nbody):
        root[b] = b if model.parent[b] == 0 else root[model.parent[b]]
    return np.array([root[max(b for b in range(model.nbody) if model.dofadr[b] <= d and model.jtype[b] != kin_ref.FIXED)] for d in range(model.nv)])


@pytest.mark.parametrize("name", ["pick", "stack"])
def test_parity_with_the_float64_reference(name):
    s = _setup(name)
    got = {k: x.cpu().numpy().astype(np.float64) for k, x in s["full"].items()}
    nv = s["model"].nv
    assert got["mass"].shape == (B, nv, nv) and all(got[k].shape == (B, nv) for k in OUTS[1:])
    e = {k: float(np.abs(got[k] - s["ref"][k]).max()) for k in OUTS}
    print(f"\n[dynamics, {name}] max |x - x64| over {B} envs:  " + "   ".join(f"{k}: GPU {e[k]:.3e} port {s['yard'][k]:.3e} allowed {4 * s['yard'][k]:.3e}" for k in OUTS))
    for k in OUTS:
        assert e[k] <= 4.0 * s["yard"][k], (name, k, e[k], s["yard"][k])
    # ... and per kinematic tree and dof kind (tests/tree_metrics.py): pooled, the arm's yardstick (mass 2e-6, tau 3e-5) is as large as
    # a cube's whole rotational inertia (3.4e-6) or torque (6.6e-6), so the cube's rotational rows could be wrong by half their size
    model = s["model"]
    bad = tree_metrics.report(f"dynamics, {name}, mass", tree_metrics.matrix_blocks(model, got["mass"], s["port"]["mass"], s["ref"]["mass"]))
    for k in OUTS[1:]:
        bad += tree_metrics.report(f"dynamics, {name}, {k}", tree_metrics.vector_blocks(model, got[k], s["port"][k], s["ref"][k]))
    assert not bad, bad


@pytest.mark.parametrize("name", ["pick", "stack"])
def test_rows_by_env_index_repeats_and_any_order(name):
    s = _setup(name)
    sc, full = s["sc"], s["full"]
    for idx in ([4, 0, 0, 3], [4, 3, 2, 1, 0], [2]):
        it = torch.tensor(idx, device=sc.device)
        rows = sc.dynamics(env_idx=it, qacc=s["qacc_d"][idx].contiguous(), **ALL)
        for k in OUTS:
            assert rows[k].shape[0] == len(idx) and torch.equal(rows[k], full[k][idx]), (name, k, idx)


def _raw(sc, idx, dof0, nd, want, qpos=None, qvel=None, qacc=None, offset=0, h=None, q=None, n_rows=None):
    """mir_dynamics into NaN-filled tensors (`offset` floats into a larger allocation: an unaligned output) -> (rc, tensors)"""
    q = make_dyn_query(dof0, nd) if q is None else q
    R = sc.num_envs if idx is None else len(idx)
    shapes = dict(mass=(R, nd, nd), bias=(R, nd), gravity=(R, nd), tau=(R, nd), ctrl_force=(R, nd))
    out = {}
    for k in want:
        n = int(np.prod(shapes[k]))
        out[k] = torch.full((n + offset,), float("nan"), device=sc.device)[offset:].view(shapes[k])
    it = None if idx is None else torch.tensor(idx, dtype=torch.long, device=sc.device)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    rc = sc.lib.mir_dynamics(sc.h if h is None else h, None if q == "null" else C.byref(q), p(it), R if n_rows is None else n_rows, p(qpos), p(qvel), p(qacc),
                             p(out.get("mass")), p(out.get("bias")), p(out.get("gravity")), p(out.get("tau")), p(out.get("ctrl_force")), sc._stream())
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("name", ["pick", "stack"])
def test_windows_coverage_symmetry_and_cross_tree_zeros(name):
    s = _setup(name)
    sc, model, full = s["sc"], s["model"], s["full"]
    nv = model.nv
    rc, out = _raw(sc, None, 0, nv, OUTS, qacc=s["qacc_d"])
    assert rc == 0
    for k in OUTS:
        assert torch.isfinite(out[k]).all() and torch.equal(out[k], full[k]), k
    M = out["mass"]
    assert torch.equal(M.view(torch.int32), M.transpose(1, 2).contiguous().view(torch.int32)), "bitwise symmetric"
    tree = _tree_of_dof(model)
    cross = torch.as_tensor(tree[:, None] != tree[None, :], device=sc.device)
    assert bool(cross.any()) and bool((M[:, cross] == 0.0).all())
    assert bool((M[:, ~cross].abs().amax(0) > 0).any())
    # sub-windows: a window that cuts the arm's tree, one that cuts a cube's six dofs with an odd n_dofs, the last dof alone; outputs at
    # an address that is not 16-byte aligned
    for d0, nd, off in ((3, 4, 0), (7, 5, 1), (nv - 1, 1, 3), (9, 6, 0), (1, nv - 1, 1)):
        rc, part = _raw(sc, [4, 0, 0], d0, nd, OUTS, qacc=s["qacc_d"][[4, 0, 0]].contiguous(), offset=off)
        assert rc == 0
        for k in OUTS:
            want = full[k][[4, 0, 0]][:, d0:d0 + nd, d0:d0 + nd] if k == "mass" else full[k][[4, 0, 0]][:, d0:d0 + nd]
            assert torch.isfinite(part[k]).all() and torch.equal(part[k], want), (name, k, d0, nd)
    # nullable outputs: each alone gives the same numbers; none at all is MIR_OK without a launch
    for k in OUTS:
        rc, one = _raw(sc, None, 0, nv, (k,), qacc=s["qacc_d"] if k == "tau" else None)
        assert rc == 0 and torch.equal(one[k], full[k]), k
    n0 = sc.__dict__.get("dynamics_launches", 0)
    assert sc.dynamics(mass=False, bias=False) == {} and sc.__dict__.get("dynamics_launches", 0) == n0


@pytest.mark.parametrize("name", ["pick", "stack"])
def test_state_overrides(name):
    from gym_genesis.backend.lib import MirScene

    s = _setup(name)
    sc, model, full = s["sc"], s["model"], s["full"]
    q, v = (x.clone() for x in sc.get_state()[:2])
    same = sc.dynamics(qpos=q, qvel=v, qacc=s["qacc_d"], **ALL)
    for k in OUTS:
        assert torch.equal(same[k], full[k]), k
    # other states: the call after set_state of those states on a second scene (same targets)
    q2, v2 = kin_ref.random_state(s["spec"], model, B, seed=41)
    other = MirScene(s["spec"], B)
    other.set_state(qpos=q2, qvel=v2, target=s["tgt"])
    want = other.dynamics(qacc=s["qacc_d"], **ALL)
    got = sc.dynamics(qpos=torch.as_tensor(q2, device=sc.device), qvel=torch.as_tensor(v2, device=sc.device), qacc=s["qacc_d"], **ALL)
    for k in OUTS:
        assert torch.equal(got[k], want[k]) and not torch.equal(got[k], full[k]), k
    idx = [3, 3, 1]
    got = sc.dynamics(env_idx=torch.tensor(idx, device=sc.device), qpos=torch.as_tensor(q2[idx], device=sc.device),
                      qvel=torch.as_tensor(v2[idx], device=sc.device), qacc=s["qacc_d"][idx].contiguous(), **ALL)
    for k in OUTS:
        assert torch.equal(got[k], want[k][idx]), k
    # qvel alone: the current qpos
    other.set_state(qpos=s["q"], qvel=v2, target=s["tgt"])
    want = other.dynamics(qacc=s["qacc_d"], **ALL)
    got = sc.dynamics(qvel=torch.as_tensor(v2, device=sc.device), qacc=s["qacc_d"], **ALL)
    for k in OUTS:
        assert torch.equal(got[k], want[k]), k
    assert torch.equal(got["mass"], full["mass"]) and torch.equal(got["gravity"], full["gravity"])
    for x, y in zip(sc.get_state()[:2], (q, v)):
        assert torch.equal(x, y), "an override changes nothing"
    other.close() if hasattr(other, "close") else None


@pytest.mark.parametrize("name", ["pick", "stack"])
def test_against_mir_forward_and_the_bitwise_identities(name):
    """mir_forward is another float32 evaluation of the same M and qfrc_bias: each within 4 x the yardstick of the reference, 8 x
    between them (the kinematics test's rule against mir_get_links)."""
    s = _setup(name)
    sc, full, yard = s["sc"], s["full"], s["yard"]
    M, bias, _, _ = sc.forward()
    eM, eb = float((M - full["mass"]).abs().max()), float((bias - full["bias"]).abs().max())
    print(f"\n[dynamics, {name}] against mir_forward: mass {eM:.3e} (allowed {8 * yard['mass']:.3e}), bias {eb:.3e} (allowed {8 * yard['bias']:.3e})")
    assert eM <= 8 * yard["mass"] and eb <= 8 * yard["bias"]
    zero = torch.zeros_like(s["qacc_d"])
    rest = sc.dynamics(qvel=zero, qacc=zero, mass=False, bias=True, gravity=True, tau=True)
    assert torch.equal(rest["bias"].view(torch.int32), full["gravity"].view(torch.int32)), "gravity is the bias of the state with qvel = 0"
    assert torch.equal(rest["gravity"].view(torch.int32), full["gravity"].view(torch.int32))
    moving = sc.dynamics(qacc=zero, mass=False, bias=True, tau=True)
    assert torch.equal(moving["tau"], moving["bias"]) and torch.equal(moving["bias"], full["bias"]), "tau at qacc = 0 is the bias"


def _grasp(n, seed=5):
    G_ = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "grasp_targets.json")))
    T = np.array(G_["targets"], np.float32)
    return np.tile(np.repeat(T.transpose(1, 0, 2), G_["steps_per_stage"], axis=0), (1, n // 4, 1))


def test_through_genesis_env_against_the_reference_on_the_state_read_back():
    from gym_genesis.env import GenesisEnv

    n = 8
    acts = _grasp(n)
    env = GenesisEnv(task="cube_pick", robot="franka", num_envs=n, enable_pixels=False)
    env.reset(seed=2)
    task = env._env
    mir, robot, cube = task._mir, task.franka, task.cube
    spec = mir.spec
    o64, port = orc.Oracle(spec, n), orc.Oracle(spec, n, f32=True)
    A = torch.as_tensor(acts, device=mir.device)
    qacc = np.random.default_rng(7).uniform(-2, 2, (n, 9)).astype(np.float32)
    full_acc = np.concatenate([qacc, np.zeros((n, 6), np.float32)], 1)
    keys = ("mass", "bias", "tau", "ctrl_force")
    worst, yard = dict.fromkeys(keys, 0.0), dict.fromkeys(keys, 0.0)
    m = float(np.float32(spec.body[cube.root].mass))
    frc_lo, frc_hi = (np.array([spec.dof[i].frc_range[j] for i in range(9)]) for j in (0, 1))
    skipped, worst_rot = 0, 0.0
    for t in range(20):
        env.step(A[20 * t % acts.shape[0]])
        got = dict(mass=robot.get_mass_mat(), bias=robot.get_dofs_bias_force(), tau=robot.inverse_dynamics(qacc), ctrl_force=robot.get_dofs_control_force())
        assert got["mass"].shape == (n, 9, 9) and all(got[k].shape == (n, 9) for k in keys[1:])
        q, v, tg = (x.cpu().numpy().astype(np.float64) for x in mir.get_state()[:3])
        ref = dyn_ref.oracle_dynamics(o64, q, v, targets=tg, qacc=full_acc)
        prt = dyn_ref.oracle_dynamics(port, q, v, targets=tg, qacc=full_acc, f32=True)
        near = dyn_ref.pd_margin(spec, q, v, tg) < 1e-3   # (a dof on a clamp limit: either side is legitimate)
        at = lambda f: (f == np.float32(frc_lo)[None, :]) | (f == np.float32(frc_hi)[None, :])  # noqa: E731
        ref_at = at(ref["ctrl_force"][:, 0:9].astype(np.float32))
        for k in keys:
            pick = (lambda r: r[k][:, 0:9, 0:9]) if k == "mass" else (lambda r: r[k][:, 0:9])
            d, y = np.abs(got[k].cpu().numpy() - pick(ref)), np.abs(pick(prt) - pick(ref))
            if k == "ctrl_force":   # left out: only a near-limit dof whose clamp state differs from the float64 reference's
                skip_g, skip_p = near & (at(got[k].cpu().numpy()) != ref_at), near & (at(pick(prt).astype(np.float32)) != ref_at)
                skipped += int(skip_g.sum()) + int(skip_p.sum())
                d, y = np.where(skip_g, 0.0, d), np.where(skip_p, 0.0, y)
            worst[k], yard[k] = max(worst[k], float(d.max())), max(yard[k], float(y.max()))
        Mc = cube.get_mass_mat().cpu().numpy()
        assert Mc.shape == (n, 6, 6) and (Mc[:, 0:3, 0:3] == np.float32(m) * np.eye(3, dtype=np.float32)).all(), "the cube's mass block is diag(m, m, m, .)"
        assert (Mc[:, 0:3, 3:6] == 0).all() and (Mc[:, 3:6, 0:3] == 0).all()
        # the cube's rotational 3 x 3 block against the reference, by its own yardstick (the arm's is as large as the block itself)
        rot = slice(12, 15)
        e_rot, y_rot = float(np.abs(Mc[:, 3:6, 3:6] - ref["mass"][:, rot, rot]).max()), float(np.abs(prt["mass"][:, rot, rot] - ref["mass"][:, rot, rot]).max())
        a_rot = tree_metrics.allowed(y_rot, ref["mass"][:, rot, rot])
        worst_rot = max(worst_rot, e_rot / a_rot)
        assert e_rot <= a_rot, (t, e_rot, y_rot, a_rot)
    print("\n[dynamics, GenesisEnv, 20 steps x 8 envs] " + "   ".join(f"{k}: GPU {worst[k]:.3e} port {yard[k]:.3e} allowed {4 * yard[k]:.3e}" for k in keys))
    # a near-limit band is 2e-3 of the force range wide per limit: a stepped state lands in one about once in 250 dof evaluations,
    # and only some of those flip; more than 1 % of the 2 x 20 x 8 x 9 comparisons would be a broken clamp, not rounding
    print(f"[dynamics, GenesisEnv] the cube's rotational block of mass: worst error / allowed over the steps {worst_rot:.3f}")
    print(f"[dynamics, GenesisEnv] ctrl_force comparisons left out (near a clamp limit AND clamp state differs): {skipped} of {2 * 20 * n * 9}")
    assert skipped <= 0.01 * 2 * 20 * n * 9
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
    A = torch.as_tensor(acts, device=mirs[0].device)
    rng = np.random.default_rng(8)
    dev = lambda a: torch.as_tensor(a.astype(np.float32), device=mirs[0].device)  # noqa: E731
    q2, v2 = kin_ref.random_state(mirs[0].spec, kin_ref.Model(mirs[0].spec), n, seed=9)
    over = dict(qpos=dev(q2), qvel=dev(v2), qacc=dev(rng.uniform(-1, 1, (n, mirs[0].nv))))
    v0 = [m.state_version for m in mirs]
    counters = ("link_kinematics_launches", "raycast_launches", "contact_force_launches")
    for t in range(50):
        res = [e.step(A[8 * t % acts.shape[0]]) for e in envs]
        mirs[0].dynamics(**over, **ALL)
        for k in ("agent_pos", "environment_state"):
            assert torch.equal(res[0][0][k], res[1][0][k]), (t, k)
        assert torch.equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])
        for x, y in zip(mirs[0].get_state(), mirs[1].get_state()):   # qpos, qvel, targets, warm start
            assert torch.equal(x, y), t
        assert mirs[0].state_version - v0[0] == mirs[1].state_version - v0[1]
    K = 4
    stride = mirs[0].agent_dim + mirs[0].env_dim + 2
    rows = [torch.zeros((K, n, stride), device=m.device) for m in mirs]
    for call in range(2):
        a = A[100 + K * call:100 + K * (call + 1)].contiguous()
        for m, r in zip(mirs, rows):
            m.rollout_exact(a, r)
        mirs[0].dynamics(**over, **ALL)
        assert torch.equal(rows[0], rows[1]), call
        for x, y in zip(mirs[0].get_state(), mirs[1].get_state()):
            assert torch.equal(x, y), call
    assert mirs[0].dynamics_launches == 52
    assert [mirs[0].__dict__.get(k, 0) for k in counters] == [mirs[1].__dict__.get(k, 0) for k in counters], "the other queries' launch counters"
    assert mirs[1].__dict__.get("dynamics_launches", 0) == 0


def test_errors_name_the_entry_point_and_launch_nothing():
    from gym_genesis.backend.lib import MirError

    s = _setup("pick")
    sc, nv = s["sc"], s["model"].nv
    bad = []
    bad.append(_raw(sc, None, 0, nv, OUTS, qacc=s["qacc_d"], q="null"))
    bad.append(_raw(sc, None, 0, nv, OUTS, qacc=s["qacc_d"], h=C.c_void_p(0)))
    q = make_dyn_query(0, nv); q.struct_size -= 4; bad.append(_raw(sc, None, 0, nv, OUTS, qacc=s["qacc_d"], q=q))
    for d0, nd in ((1, nv), (-1, 2), (0, -1), (nv + 1, 0)):
        q = make_dyn_query(0, nv); q.dof0, q.n_dofs = d0, nd; bad.append(_raw(sc, None, 0, nv, OUTS, qacc=s["qacc_d"], q=q))
    for bit in (1, 1 << 31):
        q = make_dyn_query(0, nv); q.flags = bit; bad.append(_raw(sc, None, 0, nv, OUTS, qacc=s["qacc_d"], q=q))
    bad.append(_raw(sc, None, 0, nv, OUTS))                                    # tau without qacc
    for rc, out in bad:
        assert rc == -1 and b"mir_dynamics" in sc.lib.mir_last_error(), rc
        assert all(torch.isnan(x).all() for x in out.values()), "a refused call launches nothing"
    rc, out = _raw(sc, [0], 0, nv, ("mass",), n_rows=(2 ** 31 - 1) // (nv * nv) + 1)   # R x n^2 does not fit 2^31 - 1
    assert rc == -2 and b"mir_dynamics" in sc.lib.mir_last_error() and torch.isnan(out["mass"]).all()
    # between mir_step_begin and mir_step_end
    bufs = (sc.empty(sc.agent_dim), sc.empty(sc.env_dim), sc.empty(), sc.empty(dtype=torch.uint8))
    before = [x.clone() for x in sc.get_state()]
    n0 = sc.__dict__.get("dynamics_launches", 0)
    sc.step_begin(None, *bufs)
    rc, out = _raw(sc, None, 0, nv, OUTS, qacc=s["qacc_d"])
    msg = sc.lib.mir_last_error()
    with pytest.raises(MirError, match="mir_dynamics.*pending"):
        sc.dynamics()
    sc.step_end()
    assert rc == -1 and b"mir_dynamics" in msg and b"pending" in msg
    assert all(torch.isnan(x).all() for x in out.values()) and sc.__dict__.get("dynamics_launches", 0) == n0
    sc.set_state(*before)   # (the shared scene goes back to the state the other tests compare)
    assert C.sizeof(MirDynQuery) == sc.lib.mir_dyn_query_sizeof()
    with pytest.raises(ValueError):
        sc.dynamics(tau=True)
