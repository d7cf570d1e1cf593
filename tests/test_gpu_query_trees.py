"""The four query kernels (mir_link_kinematics, mir_link_accelerations, mir_dynamics, mir_task_dynamics) on the synthetic trees of
tests/tree_cases.py: oblique axes, arbitrary frame rotations, prismatic and fixed joints in mid-chain, branching at every level, a path of
15 bodies, 15 dofs in one tree, a free root with limbs, anisotropic free bodies with their centre of mass off the origin, and three trees
of very different scale in one launch of the wave-kernel model.  The other GPU tests of these entry points know the two Franka scenes.

States are SET (set_state of kin_ref.random_state, seeded targets), never stepped: no step, forward, reset or get_links here.  B = 5 envs
(rows x items is not a multiple of four: the clamped pairs run).  One launch per entry point and case, compared with the float64
references (kin_ref, acc_ref, dyn_ref, task_ref) per kinematic tree and per dof kind -- tests/tree_metrics.py, never pooled over the
scene.  Allowed per block: max(4 x the float32 port's error on that block, 2^-23 x max |reference| of that block).  Every figure is
printed: GPU, port, allowed.  Measured figures: DESIGN.md, next to the "measured errors" paragraphs of the four entry points.
"""
import numpy as np
import pytest
import torch

import acc_ref
import dyn_ref
import kin_ref
import orc
import task_ref
import tree_cases
import tree_metrics as tm

pytestmark = pytest.mark.gpu

B = 5
DAMPINGS = (0.0, 0.05)
ROWS = [4, 0, 0, 3]
DYN_ALL = dict(mass=True, bias=True, gravity=True, tau=True, ctrl_force=True)
TASK_ALL = dict(minv=True, solve=True, lambda_inv=True, lambda_=True, jbar=True)
_cache = {}


def _setup(name):
    """scene, seeded state / targets / qacc / x / local points / sensor axes, both oracles at that state: once per case"""
    if name in _cache:
        return _cache[name]
    from gym_genesis.backend.lib import MirScene

    sb, spec = tree_cases.build(name)
    model = kin_ref.Model(spec)
    sc = MirScene(spec, B)
    assert sc.kernel == tree_cases.KERNEL[name] and (model.nbody, model.nv) == tree_cases.DIMS[name]
    q, v = kin_ref.random_state(spec, model, B, seed=3)
    tgt, qacc = dyn_ref.random_targets_and_acc(spec, q, v, seed=4)
    margin = dyn_ref.pd_margin(spec, q, v, tgt)   # (on the CPU: no position-controlled dof within 1e-3 of its force range of a clamp limit)
    assert margin.min() > 1e-3, margin.min()
    sc.set_state(qpos=q, qvel=v, target=tgt)
    f32 = "big" if tree_cases.KERNEL[name] == 64 else True
    o64, port = orc.Oracle(spec, B), orc.Oracle(spec, B, f32=f32)
    for o in (o64, port):
        o.write_all(orc.F_QPOS, q.astype(np.float64))
        o.write_all(orc.F_QVEL, v.astype(np.float64))
    rng = np.random.default_rng(5)
    links = list(range(1, spec.nbody))   # every link of the scene in one query
    lps = rng.uniform(-0.05, 0.05, (len(links), 3)).astype(np.float32)
    qoff = rng.normal(size=(len(links), 4))
    qoff = (qoff / np.linalg.norm(qoff, axis=1, keepdims=True)).astype(np.float32)
    x = rng.uniform(-2.0, 2.0, (B, model.nv)).astype(np.float32)
    dev = lambda a: torch.as_tensor(a, device=sc.device)  # noqa: E731
    _cache[name] = dict(sb=sb, spec=spec, model=model, sc=sc, q=q, v=v, tgt=tgt, qacc=qacc, x=x, f32=f32, o64=o64, port=port, links=links,
                        lps=lps, qoff=qoff, dev=dev)
    return _cache[name]


def _np64(d):
    return {k: a.cpu().numpy().astype(np.float64) for k, a in d.items()}


def _same_sign(q, ref):
    """q or -q, whichever is nearer the reference (B, L, 4)"""
    return np.where((q * ref).sum(-1, keepdims=True) < 0, -q, q)


def _path_dofs(model, link):
    return [d for b in model.path(link) for d in range(model.dofadr[b], model.dofadr[b] + {0: 0, 1: 1, 2: 1, 3: 6}[model.jtype[b]])]


# ---- kinematics ------------------------------------------------------------------------------------------------------------------
def _kin(s):
    if "kin" not in s:
        ref = kin_ref.oracle_kinematics(s["o64"], s["model"], s["links"], s["lps"])
        port = {k: a.astype(np.float64) for k, a in kin_ref.oracle_kinematics(s["port"], s["model"], s["links"], s["lps"], dtype=np.float32).items()}
        s["kin"] = (ref, port, s["sc"].link_kinematics(s["links"], s["lps"]))
    return s["kin"]


@pytest.mark.parametrize("name", tree_cases.CASES)
def test_kinematics(name):
    s = _setup(name)
    sc, model, links = s["sc"], s["model"], s["links"]
    ref, port, full = _kin(s)
    got = _np64(full)
    L, nv = len(links), model.nv
    assert got["pos"].shape == (B, L, 3) and got["quat"].shape == (B, L, 4) and got["vel"].shape == (B, L, 6) and got["jac"].shape == (B, L, 6, nv)
    print()
    bad = tm.report(f"kinematics, {name}, pos", tm.link_blocks(model, links, got["pos"], port["pos"], ref["pos"]))
    bad += tm.report(f"kinematics, {name}, quat", tm.link_blocks(model, links, _same_sign(got["quat"], ref["quat"]), _same_sign(port["quat"], ref["quat"]), ref["quat"]))
    bad += tm.report(f"kinematics, {name}, vel", tm.link_blocks(model, links, got["vel"], port["vel"], ref["vel"]))
    bad += tm.report(f"kinematics, {name}, jac", tm.jac_blocks(model, links, got["jac"], port["jac"], ref["jac"]))
    assert not bad, bad
    assert np.abs(np.linalg.norm(got["quat"], axis=-1) - 1.0).max() < 1e-6
    for i, b in enumerate(links):   # off-path columns are exact zeros, on-path columns are not
        on = _path_dofs(model, b)
        off = [d for d in range(nv) if d not in on]
        assert (got["jac"][:, i][:, :, off] == 0.0).all(), (name, b)
        assert all(np.abs(got["jac"][:, i, :, d]).max() > 0 for d in on), (name, b)
    # a dof window (on `floating` and `many` it cuts the six columns of a free root): the same bits, addressed by dof0 / n_dofs
    d0 = 2 if name != "many" else model.dofadr[10] + 2
    nd = min(7, nv - d0)
    sub = sc.link_kinematics(links, s["lps"], dof0=d0, n_dofs=nd, pos=False, quat=False)
    assert sub["jac"].shape == (B, L, 6, nd) and torch.equal(sub["jac"], full["jac"][:, :, :, d0:d0 + nd]) and torch.equal(sub["vel"], full["vel"])


# ---- accelerations ---------------------------------------------------------------------------------------------------------------
def _acc(s):
    if "acc" not in s:
        ref = acc_ref.oracle_accelerations(s["o64"], s["model"], s["links"], s["qacc"], s["lps"], s["qoff"])
        port = {k: a.astype(np.float64) for k, a in
                acc_ref.oracle_accelerations(s["port"], s["model"], s["links"], s["qacc"], s["lps"], s["qoff"], dtype=np.float32).items()}
        full = s["sc"].link_accelerations(s["links"], s["lps"], s["qoff"], qacc=s["dev"](s["qacc"]), acc=True, bias_acc=True, imu=True)
        s["acc"] = (ref, port, full)
    return s["acc"]


@pytest.mark.parametrize("name", tree_cases.CASES)
def test_accelerations(name):
    s = _setup(name)
    model, links = s["model"], s["links"]
    ref, port, full = _acc(s)
    got = _np64(full)
    print()
    bad = []
    for k in ("acc", "bias_acc", "imu"):
        assert got[k].shape == (B, len(links), 6), k
        bad += tm.report(f"accelerations, {name}, {k}", tm.link_blocks(model, links, got[k], port[k], ref[k]))
    assert not bad, bad


# ---- dynamics --------------------------------------------------------------------------------------------------------------------
def _dyn(s):
    if "dyn" not in s:
        ref = dyn_ref.oracle_dynamics(orc.Oracle(s["spec"], B), s["q"], s["v"], targets=s["tgt"], qacc=s["qacc"])
        port = dyn_ref.oracle_dynamics(orc.Oracle(s["spec"], B, f32=s["f32"]), s["q"], s["v"], targets=s["tgt"], qacc=s["qacc"], f32=True)
        s["dyn"] = (ref, port, s["sc"].dynamics(qacc=s["dev"](s["qacc"]), **DYN_ALL))
    return s["dyn"]


@pytest.mark.parametrize("name", tree_cases.CASES)
def test_dynamics(name):
    s = _setup(name)
    sc, model, spec = s["sc"], s["model"], s["spec"]
    ref, port, full = _dyn(s)
    got = _np64(full)
    nv = model.nv
    assert got["mass"].shape == (B, nv, nv) and all(got[k].shape == (B, nv) for k in dyn_ref.OUTS[1:])
    ctrl = [i for i in range(spec.ndof) if spec.dof[i].ctrl_mode == 1]
    at_limit = np.abs(ref["ctrl_force"][:, ctrl]) == 40.0
    assert at_limit.any() and not at_limit.all(), "some dofs clamp, some do not"
    print()
    bad = tm.report(f"dynamics, {name}, mass", tm.matrix_blocks(model, got["mass"], port["mass"], ref["mass"]))
    for k in dyn_ref.OUTS[1:]:
        bad += tm.report(f"dynamics, {name}, {k}", tm.vector_blocks(model, got[k], port[k], ref[k]))
    assert not bad, bad
    M = full["mass"]
    assert torch.equal(M.view(torch.int32), M.transpose(1, 2).contiguous().view(torch.int32)), "bitwise symmetric"
    tree = np.zeros(nv, np.int64)
    for (root, _), idx in tm.dof_groups(model):
        tree[idx] = root
    cross = torch.as_tensor(tree[:, None] != tree[None, :], device=sc.device)
    assert bool(cross.any()) == (name == "many") and bool((M[:, cross] == 0.0).all())
    zero = torch.zeros_like(full["bias"])
    rest = sc.dynamics(qvel=zero, qacc=zero, mass=False, bias=True, gravity=True, tau=True)
    assert torch.equal(rest["bias"].view(torch.int32), full["gravity"].view(torch.int32)), "gravity is the bias of the state with qvel = 0"
    assert torch.equal(rest["gravity"].view(torch.int32), full["gravity"].view(torch.int32)) and torch.equal(rest["tau"], rest["bias"])
    # windows: one inside a free root's six dofs (`floating`, `many`), one that cuts the tree elsewhere
    free = [b for b in range(1, model.nbody) if model.jtype[b] == kin_ref.FREE]
    for d0, nd in ([(model.dofadr[free[0]] + 2, 3)] if free else []) + [(1, min(6, nv - 1)), (nv - 1, 1)]:
        part = sc.dynamics(dof0=d0, n_dofs=nd, qacc=s["dev"](s["qacc"]), **DYN_ALL)
        for k in dyn_ref.OUTS:
            want = full[k][:, d0:d0 + nd, d0:d0 + nd] if k == "mass" else full[k][:, d0:d0 + nd]
            assert torch.equal(part[k], want), (name, k, d0, nd)


# ---- task dynamics -----------------------------------------------------------------------------------------------------------------
def _task(s, name):
    """two links with >= 6 dofs on their path (bushy has none: its two deepest leaves, singular without damping); the pivot condition
    of tests/test_gpu_task_dynamics.py is checked here, on the CPU"""
    if "task" not in s:
        model, spec = s["model"], s["spec"]
        links = tree_cases.links_on_long_paths(model)[:2] or [model.nbody - 1, model.nbody - 2]
        lps = s["lps"][[b - 1 for b in links]]
        M, J = task_ref.oracle_mass_and_jacobian(spec, model, s["q"], links, lps)
        M32, J32 = task_ref.oracle_mass_and_jacobian(spec, model, s["q"], links, lps, f32=s["f32"])
        ref, port, full = {}, {}, {}
        for d in DAMPINGS:
            ref[d] = task_ref.combine(M, J, s["x"].astype(np.float64), d)
            port[d] = {k: np.asarray(a, np.float64) for k, a in task_ref.combine(M32, J32, s["x"], d).items()}
            sing = np.isnan(ref[d]["lambda"]).all(axis=(2, 3))
            assert np.array_equal(sing, np.isnan(port[d]["lambda"]).all(axis=(2, 3)))
            if name == "bushy":
                assert sing.all() == (d == 0.0) and (d > 0 or (ref[d]["relpivot"] < 1e-6).all()), (d, ref[d]["relpivot"])
            else:
                assert not sing.any() and (ref[d]["relpivot"] > 1e-4).all(), (name, d, ref[d]["relpivot"])
            full[d] = s["sc"].task_dynamics(links=links, local_points=lps, x=s["dev"](s["x"]), damping=d, **TASK_ALL)
        s["task"] = (links, lps, ref, port, full)
    return s["task"]


def _residual(lam, lam_inv64, d):
    return float(np.abs(lam @ (lam_inv64 + d * d * np.eye(6)) - np.eye(6)).max())


@pytest.mark.parametrize("name", tree_cases.CASES)
def test_task_dynamics(name):
    s = _setup(name)
    model = s["model"]
    links, lps, ref, port, full = _task(s, name)
    nv = model.nv
    bad = []
    print()
    for d in DAMPINGS:
        got, r, p = _np64(full[d]), ref[d], port[d]
        assert got["minv"].shape == (B, nv, nv) and got["solve"].shape == (B, nv) and got["jbar"].shape == (B, 2, nv, 6)
        assert got["lambda_inv"].shape == (B, 2, 6, 6) and got["lambda"].shape == (B, 2, 6, 6)
        t = f"task dynamics, {name}, damping {d}"
        bad += tm.report(f"{t}, minv", tm.matrix_blocks(model, got["minv"], p["minv"], r["minv"]))
        bad += tm.report(f"{t}, solve", tm.vector_blocks(model, got["solve"], p["solve"], r["solve"]))
        for l, b in enumerate(links):
            e, y = float(np.abs(got["lambda_inv"][:, l] - r["lambda_inv"][:, l]).max()), float(np.abs(p["lambda_inv"][:, l] - r["lambda_inv"][:, l]).max())
            bad += tm.report(f"{t}, lambda_inv", [((b,), e, y, tm.allowed(y, r["lambda_inv"][:, l]))])
        assert np.isfinite(got["minv"]).all() and np.isfinite(got["solve"]).all() and np.isfinite(got["lambda_inv"]).all()
        if name == "bushy":
            if d == 0.0:   # four dofs on every path: the NaN rule on links other than the Panda's link3; nothing else is affected
                assert np.isnan(got["lambda"]).all() and np.isnan(got["jbar"]).all()
            continue       # (with damping 0.05 that 6 x 6 sits at a relative pivot of ~1e-4: a bar would measure conditioning)
        for l, b in enumerate(links):
            # jbar (nv, 6) by the dof groups of its rows, the other trees' rows included: exact zeros
            rows = tm.vector_blocks(model, got["jbar"][:, l].transpose(0, 2, 1).reshape(-1, nv), p["jbar"][:, l].transpose(0, 2, 1).reshape(-1, nv),
                                    r["jbar"][:, l].transpose(0, 2, 1).reshape(-1, nv))
            bad += tm.report(f"{t}, jbar of link {b}", rows)
            e, y = _residual(got["lambda"][:, l], r["lambda_inv"][:, l], d), _residual(p["lambda"][:, l], r["lambda_inv"][:, l], d)
            bad += tm.report(f"{t}, lambda residual", [((b,), e, y, max(4.0 * y, tm.EPS32))])
    assert not bad, bad
    for k in ("minv", "solve", "lambda_inv"):
        assert torch.equal(full[0.0][k], full[0.05][k]), "damping reaches lambda and jbar only"
    Mi, Li = full[0.05]["minv"], full[0.05]["lambda_inv"]
    assert torch.equal(Mi.view(torch.int32), Mi.transpose(1, 2).contiguous().view(torch.int32)), "minv bitwise symmetric"
    assert torch.equal(Li.view(torch.int32), Li.transpose(2, 3).contiguous().view(torch.int32)), "lambda_inv bitwise symmetric"


# ---- rows ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["floating", "many"])   # one case on each model
def test_rows_by_env_index_repeats_and_any_order(name):
    s = _setup(name)
    sc, links, lps = s["sc"], s["links"], s["lps"]
    it = torch.tensor(ROWS, device=sc.device)
    qacc, x = s["dev"](s["qacc"])[ROWS].contiguous(), s["dev"](s["x"])[ROWS].contiguous()
    tl, tlp, _, _, tfull = _task(s, name)
    pairs = [(_kin(s)[2], sc.link_kinematics(links, lps, env_idx=it)),
             (_acc(s)[2], sc.link_accelerations(links, lps, s["qoff"], env_idx=it, qacc=qacc, acc=True, bias_acc=True, imu=True)),
             (_dyn(s)[2], sc.dynamics(env_idx=it, qacc=qacc, **DYN_ALL)),
             (tfull[0.05], sc.task_dynamics(links=tl, local_points=tlp, env_idx=it, x=x, damping=0.05, **TASK_ALL))]
    for full, rows in pairs:
        assert set(full) == set(rows)
        for k in full:
            assert rows[k].shape[0] == len(ROWS) and torch.equal(rows[k].view(torch.int32), full[k][ROWS].contiguous().view(torch.int32)), (name, k)
