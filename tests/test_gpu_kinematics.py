"""Link poses, velocities and Jacobians on the GPU (include/mirigid.h: mir_link_kinematics; views: get_jacobian, get_links_*, get_vel).

States are SET (set_state), not stepped to: the GPU, the float64 oracle and its float32 port hold the same float32 bits.  B = 5 envs
(not a multiple of four: the last wave has clamped pairs), the Franka pick scene (16-lane model, qpos rows of 16 floats) and the
five-cube stack scene (wave-kernel model, rows of 64).

  * parity: pos, quat (up to sign), vel, jac against the float64 reference of tests/kin_ref.py; metric = max absolute error per output
    over the batch; the GPU is allowed 4 x the same error of the float32 port (kin_ref in float32 on the poses of the oracle's float32
    build) on the same states.  Both figures are printed;
  * off-path columns are exact zeros, every element is written, nullable outputs;
  * vel = jac_full @ qvel from the same call; poses agree with mir_get_links;
  * through GenesisEnv; a read is invisible; the error returns.
The MIR_E_CAPACITY case (a path of more than 16 bodies) is left out: the scene compilers refuse such a scene before it exists -- the
bodies of a subtree must share a row of 16 body indices ("the bodies of a subtree must share a 16-lane row", mir_compile64.cpp), so no
path world -> link can hold more than 16 bodies.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import kin_ref
import orc
from gym_genesis.backend import models
from gym_genesis.backend.spec import MirKinQuery, make_kin_query

pytestmark = pytest.mark.gpu

B = 5
OUTS = ("pos", "quat", "vel", "jac")
_cache = {}


def _setup(name):
    """scene with a seeded random state, the float64 reference and the float32 port of EVERY link (origins), computed once"""
    if name in _cache:
        return _cache[name]
    from gym_genesis.backend.lib import MirScene

    sb = models.franka_cube_pick_scene() if name == "pick" else models.franka_cube_stack_scene()
    spec = sb.build()
    model = kin_ref.Model(spec)
    sc = MirScene(spec, B)
    assert sc.kernel == (16 if name == "pick" else 64)
    q, v = kin_ref.random_state(spec, model, B, seed=21 if name == "pick" else 22)
    sc.set_state(qpos=q, qvel=v)
    o64, port = orc.Oracle(spec, B), orc.Oracle(spec, B, f32=True if name == "pick" else "big")
    for o in (o64, port):
        o.write_all(orc.F_QPOS, q.astype(np.float64))
        o.write_all(orc.F_QVEL, v.astype(np.float64))
    every = list(range(1, spec.nbody))
    ref_all = kin_ref.oracle_kinematics(o64, model, every)
    port_all = kin_ref.oracle_kinematics(port, model, every, dtype=np.float32)
    _cache[name] = dict(sb=sb, spec=spec, model=model, sc=sc, q=q, v=v, o64=o64, port=port, every=every, ref_all=ref_all, port_all=port_all)
    return _cache[name]


def _queried(s, name):
    """hand, both fingers (the longest path), every cube; a non-zero local point on the hand and on the first cube"""
    sb = s["sb"]
    cubes = ["cube"] if name == "pick" else list(models.STACK_CUBES)
    links = [sb.body_index(n) for n in ["hand", "left_finger", "right_finger"] + cubes]
    lps = np.zeros((len(links), 3))
    lps[0], lps[3] = (0.0, 0.01, 0.1), (0.02, -0.02, 0.02)
    return links, lps


def _errs(got, ref):
    """max absolute error per output (quat up to sign)"""
    e = {k: float(np.abs(got[k].astype(np.float64) - ref[k]).max()) for k in ("pos", "vel", "jac") if k in got}
    if "quat" in got:
        g = got["quat"].astype(np.float64)
        e["quat"] = float(np.minimum(np.abs(g - ref["quat"]).max(-1), np.abs(g + ref["quat"]).max(-1)).max())
    return e


def _parity_refs(s, name):
    key = "parity"
    if key not in s:
        links, lps = _queried(s, name)
        s[key] = (links, lps, kin_ref.oracle_kinematics(s["o64"], s["model"], links, lps),
                  kin_ref.oracle_kinematics(s["port"], s["model"], links, lps, dtype=np.float32))
    return s[key]


def _bound(s, name):
    """4 x the float32 port's error per output, over the queried links with their local points"""
    links, lps, ref, port = _parity_refs(s, name)
    yard = _errs(port, ref)
    return {k: 4.0 * v for k, v in yard.items()}, yard


@pytest.mark.parametrize("name", ["pick", "stack"])
def test_parity_with_the_float64_reference(name):
    s = _setup(name)
    sc, model = s["sc"], s["model"]
    links, lps, ref, port = _parity_refs(s, name)
    allowed, yard = _bound(s, name)
    got = {k: x.cpu().numpy() for k, x in sc.link_kinematics(links, lps).items()}
    assert got["jac"].shape == (B, len(links), 6, model.nv) and got["vel"].shape == (B, len(links), 6)
    e = _errs(got, ref)
    print(f"\n[kinematics, {name}] max |x - x64| over {B} envs x {len(links)} links:  " + "   ".join(f"{k}: GPU {e[k]:.3e} port {yard[k]:.3e} allowed {allowed[k]:.3e}" for k in OUTS))
    for k in OUTS:
        assert e[k] <= allowed[k], (name, k, e[k], yard[k])
    assert np.abs(np.linalg.norm(got["quat"], axis=-1) - 1.0).max() < 1e-6
    # each entity's own columns: the same numbers, addressed by dof0 / n_dofs
    ranges = [(0, 9)] + [(9 + 6 * k, 6) for k in range((model.nv - 9) // 6)]
    for d0, nd in ranges:
        sub = sc.link_kinematics(links, lps, dof0=d0, n_dofs=nd, pos=False, quat=False)
        assert sub["jac"].shape == (B, len(links), 6, nd)
        assert np.array_equal(sub["jac"].cpu().numpy(), got["jac"][:, :, :, d0:d0 + nd]), (name, d0, nd)
        assert np.array_equal(sub["vel"].cpu().numpy(), got["vel"]), "vel does not depend on the column range"


@pytest.mark.parametrize("name", ["pick", "stack"])
def test_rows_by_env_index_repeats_and_any_order(name):
    s = _setup(name)
    sc = s["sc"]
    links, lps, ref, port = _parity_refs(s, name)
    idx = [4, 0, 0, 3]
    full = sc.link_kinematics(links, lps)
    rows = sc.link_kinematics(links, lps, env_idx=torch.tensor(idx, device=sc.device))
    for k in OUTS:
        assert rows[k].shape[0] == 4 and torch.equal(rows[k], full[k][idx]), (name, k)
    one = sc.link_kinematics([links[1]], env_idx=torch.tensor([2], device=sc.device))   # (one pair: three clamped pairs in its wave)
    assert torch.equal(one["jac"][0, 0], sc.link_kinematics([links[1]])["jac"][2, 0])


def _raw(sc, links, lps, idx, dof0, nd, want):
    """mir_link_kinematics into NaN-filled tensors -> (rc, tensors)"""
    q = make_kin_query(links, lps, dof0, nd)
    R, L = (sc.num_envs if idx is None else len(idx)), len(links)
    shapes = dict(pos=(R, L, 3), quat=(R, L, 4), vel=(R, L, 6), jac=(R, L, 6, nd))
    out = {k: torch.full(shapes[k], float("nan"), device=sc.device) for k in want}
    it = None if idx is None else torch.tensor(idx, dtype=torch.long, device=sc.device)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    rc = sc.lib.mir_link_kinematics(sc.h, C.byref(q), p(it), R, p(out.get("pos")), p(out.get("quat")), p(out.get("vel")), p(out.get("jac")), sc._stream())
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("name", ["pick", "stack"])
def test_every_element_is_written_and_off_path_columns_are_exact_zeros(name):
    s = _setup(name)
    sc, model = s["sc"], s["model"]
    links, lps = _queried(s, name)
    nv = model.nv
    rc, out = _raw(sc, links, lps, None, 0, nv, OUTS)
    assert rc == 0
    for k in OUTS:
        assert torch.isfinite(out[k]).all(), k
    jac = out["jac"].cpu().numpy()
    nd_of = {0: 0, 1: 1, 2: 1, 3: 6}
    for i, b in enumerate(links):
        on = {d for pb in model.path(b) for d in range(model.dofadr[pb], model.dofadr[pb] + nd_of[model.jtype[pb]])}
        off = [d for d in range(nv) if d not in on]
        assert (jac[:, i][:, :, off] == 0.0).all(), (name, b)
        assert (np.abs(jac[:, i][:, :, sorted(on)]).max(axis=(0, 1)) > 0).all(), "every dof of the path has a column"
    # an odd column count and an odd number of pairs (blocks that are not a multiple of 16 bytes), a range that cuts a cube's six dofs
    rc, part = _raw(sc, links[:3], lps[:3], [4, 0, 0], 7, 5, ("jac",))
    assert rc == 0 and torch.isfinite(part["jac"]).all()
    assert np.array_equal(part["jac"].cpu().numpy(), jac[[4, 0, 0]][:, :3, :, 7:12])
    # nullable outputs: jac alone, vel alone -- the others stay untouched (there is nothing to touch), the result is the same
    rc, ja = _raw(sc, links, lps, None, 0, nv, ("jac",))
    assert rc == 0 and torch.equal(ja["jac"], out["jac"])
    rc, ve = _raw(sc, links, lps, None, 0, nv, ("vel",))
    assert rc == 0 and torch.equal(ve["vel"], out["vel"])
    rc, none = _raw(sc, links, lps, None, 0, nv, ())
    assert rc == 0 and none == {}


@pytest.mark.parametrize("name", ["pick", "stack"])
def test_velocity_is_the_jacobian_times_qvel_and_poses_are_those_of_get_links(name):
    """vel against jac_full @ qvel in torch: both are sums of the same <= nv products J_ki qvel_i in float32, in different orders and
    with or without fused multiply-adds: each side carries at most nv x 2^-24 x sum_i |J_ki| |qvel_i|, the tolerance is the two together.
    Poses against mir_get_links: two float32 forward kinematics of the same state, each within the parity bound of the reference."""
    s = _setup(name)
    sc, model = s["sc"], s["model"]
    k = sc.link_kinematics(s["every"])
    qv = sc.get_state()[1]
    jv = torch.einsum("blkd,bd->blk", k["jac"], qv)
    tol = 2 * model.nv * 2.0 ** -24 * torch.einsum("blkd,bd->blk", k["jac"].abs(), qv.abs()) + 1e-30
    err = (k["vel"] - jv).abs()
    print(f"\n[kinematics, {name}] |vel - jac @ qvel| max {float(err.max()):.3e}, worst ratio to its tolerance {float((err / tol).max()):.3f}")
    assert bool((err <= tol).all())
    assert float(k["vel"].abs().max()) > 0.1
    yard = _errs(s["port_all"], s["ref_all"])
    pos, quat = (x.cpu().numpy().astype(np.float64) for x in sc.get_links())
    ep = float(np.abs(k["pos"].cpu().numpy() - pos[:, 1:]).max())
    g = k["quat"].cpu().numpy().astype(np.float64)
    qn = quat[:, 1:] / np.linalg.norm(quat[:, 1:], axis=-1, keepdims=True)
    eq = float(np.minimum(np.abs(g - qn).max(-1), np.abs(g + qn).max(-1)).max())
    print(f"[kinematics, {name}] against mir_get_links, all links: pos {ep:.3e} (allowed {8 * yard['pos']:.3e}), quat {eq:.3e} (allowed {8 * yard['quat']:.3e})")
    assert ep <= 2 * 4 * yard["pos"] and eq <= 2 * 4 * yard["quat"]


def _grasp(n):
    import test_gpu_contact_forces as cf

    return cf._grasp(n)


def test_through_genesis_env_against_the_oracle_on_the_state_read_back():
    from gym_genesis.env import GenesisEnv

    n = 8
    _, acts = _grasp(n)
    env = GenesisEnv(task="cube_pick", robot="franka", num_envs=n, enable_pixels=False)
    env.reset(seed=2)
    task = env._env
    mir, robot, cube = task._mir, task.franka, task.cube
    hand = robot.get_link("hand")
    spec = mir.spec
    model = kin_ref.Model(spec)
    o64, port = orc.Oracle(spec, n), orc.Oracle(spec, n, f32=True)
    links = [hand.idx, cube.root]
    A = torch.as_tensor(acts, device=mir.device)
    worst = dict(jac=0.0, vel=0.0, cube=0.0)
    yard = dict(jac=0.0, vel=0.0, cube=0.0)
    for t in range(20):
        env.step(A[20 * t % acts.shape[0]])
        J, hv, cv = robot.get_jacobian(hand), hand.get_vel(), cube.get_links_vel()
        assert J.shape == (n, 6, 9) and hv.shape == (n, 3) and cv.shape == (n, 1, 3)
        q, v = (x.cpu().numpy().astype(np.float64) for x in mir.get_state()[:2])
        for o in (o64, port):
            o.write_all(orc.F_QPOS, q)
            o.write_all(orc.F_QVEL, v)
        ref = kin_ref.oracle_kinematics(o64, model, links)
        prt = kin_ref.oracle_kinematics(port, model, links, dtype=np.float32)
        for key, got, pick in (("jac", J.cpu().numpy(), lambda r: r["jac"][:, 0, :, 0:9]), ("vel", hv.cpu().numpy(), lambda r: r["vel"][:, 0, 0:3]),
                               ("cube", cv.cpu().numpy()[:, 0], lambda r: r["vel"][:, 1, 0:3])):
            worst[key] = max(worst[key], float(np.abs(got - pick(ref)).max()))
            yard[key] = max(yard[key], float(np.abs(pick(prt).astype(np.float64) - pick(ref)).max()))
    print("\n[kinematics, GenesisEnv, 20 steps x 8 envs] " + "   ".join(f"{k}: GPU {worst[k]:.3e} port {yard[k]:.3e} allowed {4 * yard[k]:.3e}" for k in worst))
    for k in worst:
        assert worst[k] <= 4.0 * yard[k], (k, worst[k], yard[k])


def test_a_read_is_invisible():
    from gym_genesis.env import GenesisEnv

    n = 8
    _, acts = _grasp(n)
    envs = [GenesisEnv(task="cube_pick", robot="franka", num_envs=n, enable_pixels=False) for _ in range(2)]
    for e in envs:
        e.reset(seed=3)
    mirs = [e._env._mir for e in envs]
    links = list(range(1, mirs[0].nbody))
    A = torch.as_tensor(acts, device=mirs[0].device)
    v0 = [m.state_version for m in mirs]
    for t in range(50):
        res = [e.step(A[8 * t % acts.shape[0]]) for e in envs]
        mirs[0].link_kinematics(links, jac=(t % 2 == 0))
        for k in ("agent_pos", "environment_state"):
            assert torch.equal(res[0][0][k], res[1][0][k]), (t, k)
        assert torch.equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])
        for x, y in zip(mirs[0].get_state(), mirs[1].get_state()):   # qpos, qvel, targets, warm start
            assert torch.equal(x, y), t
        assert mirs[0].state_version - v0[0] == mirs[1].state_version - v0[1]
    # ... and between two device-resident rollouts that keep every contact point
    K = 4
    stride = mirs[0].agent_dim + mirs[0].env_dim + 2
    rows = [torch.zeros((K, n, stride), device=m.device) for m in mirs]
    for call in range(2):
        a = A[100 + K * call:100 + K * (call + 1)].contiguous()
        for m, r in zip(mirs, rows):
            m.rollout_exact(a, r)
        mirs[0].link_kinematics(links)
        assert torch.equal(rows[0], rows[1]), call
        for x, y in zip(mirs[0].get_state(), mirs[1].get_state()):
            assert torch.equal(x, y), call


def test_errors_name_the_entry_point_and_launch_nothing():
    s = _setup("pick")
    sc = s["sc"]
    lib, nv, nbody = sc.lib, s["model"].nv, s["spec"].nbody
    pos = torch.full((B, 1, 3), float("nan"), device=sc.device)

    def call(q, h=None):
        rc = lib.mir_link_kinematics(sc.h if h is None else h, None if q is None else C.byref(q), None, 0, C.c_void_p(pos.data_ptr()), None, None, None, sc._stream())
        return rc, lib.mir_last_error()

    good = make_kin_query([9], None, 0, nv)
    assert call(good)[0] == 0
    torch.cuda.synchronize()
    assert torch.isfinite(pos).all()
    pos.fill_(float("nan"))
    bad = []
    bad.append(call(None))                                            # null query
    bad.append(call(good, h=C.c_void_p(0)))                           # null handle
    q = make_kin_query([9], None, 0, nv); q.struct_size -= 4; bad.append(call(q))
    q = make_kin_query([9], None, 0, nv); q.n_links = 0; bad.append(call(q))
    q = make_kin_query([9], None, 0, nv); q.n_links = 33; bad.append(call(q))
    q = make_kin_query([nbody], None, 0, nv); bad.append(call(q))     # link outside 1 .. nbody - 1
    q = make_kin_query([0], None, 0, nv); bad.append(call(q))         # the world
    q = make_kin_query([9], None, 1, nv); bad.append(call(q))         # columns beyond nv
    q = make_kin_query([9], None, -1, 2); bad.append(call(q))
    q = make_kin_query([9], None, 0, -1); bad.append(call(q))
    for rc, msg in bad:
        assert rc == -1 and b"mir_link_kinematics" in msg, (rc, msg)
    # between mir_step_begin and mir_step_end
    bufs = (sc.empty(sc.agent_dim), sc.empty(sc.env_dim), sc.empty(), sc.empty(dtype=torch.uint8))
    before = [x.clone() for x in sc.get_state()]
    sc.step_begin(None, *bufs)
    rc, msg = call(good)
    sc.step_end()
    assert rc == -1 and b"mir_link_kinematics" in msg and b"pending" in msg
    torch.cuda.synchronize()
    assert torch.isnan(pos).all(), "a refused call launches nothing"
    sc.set_state(*before)   # (the shared scene goes back to the state the other tests compare)
    assert C.sizeof(MirKinQuery) == lib.mir_kin_query_sizeof()
