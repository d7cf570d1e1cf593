"""GPU tests of the multi-link inverse kinematics (mir_inverse_kinematics_multilink, csrc/mir_ikm.hip) against tests/ikm_ref.py: the
float64 reference and its float32 port on `Oracle(f32=...)`, the yardstick for what a float32 kernel that sums in another order may
differ by.

  * seven cases (ikm_ref.GPU_CASES) x two scenes (the Franka pick scene: 16-lane model; the five-cube stack scene: wave model), B = 5
    rows.  tests/test_ikm_cpu.py asserts that every one of them converges on every row, in the reference and in the port, within half of
    max_iters: that is what lets this file demand convergence on every row.  Finger targets are drawn over [0, 0.04], or over the
    scene's own finger range where that is narrower (the stack scene's fingers open to 0.024: a target beyond it cannot be reached).
  * agreement with the existing single-link kernel; rows by env index; the error returns; a call is invisible to the state and the next
    step; the route through GenesisEnv; restarts.
The MIR_E_CAPACITY return (a union of more than 16 elements) is left out, as the capacity cases of tests/test_gpu_task_dynamics.py are:
the scene compilers refuse a kinematic tree of more than 16 bodies before such a scene exists.

Measured on an MI355X (gfx950), worst over the 14 case x scene pairs -- the figures each test prints (multi-link IK, has the table):
  float64 residual at the returned q: position 4.43e-04 m (tolerance 5e-4), orientation 8.93e-04 rad (tolerance 5e-3);
  max |q - q_ref64| 5.32e-05 rad against the port's 1.9e-6 at most, median 1.14e-05: inside the floors 5e-3 / 1e-4;
  iterations equal to the float64 reference's on every row of every case.
One link with full masks against the existing kernel: 1.27e-5.  Restarts: 26 of 32 rows converge with one sample, 32 with eight (the
reference: 26 and 32), the winning samples those of the reference.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import ikm_ref
import orc
from gym_genesis.backend import models
from gym_genesis.backend.spec import IK_INIT_BY_ENV, IK_POS_BY_ENV, IK_QUAT_BY_ENV, IK_QUAT_ONE, MirIkMulti, MirIkOptions, MirIkRows, make_ik_multi

pytestmark = pytest.mark.gpu

HOME = models.FRANKA_HOME
B = 5
POS_TOL, ROT_TOL, MAX_ITERS = 5e-4, 5e-3, 20
_cache = {}


def _setup(scene: str, n: int = B) -> dict:
    key = (scene, n)
    if key not in _cache:
        from gym_genesis.backend.lib import MirScene

        b = models.franka_cube_pick_scene() if scene == "pick" else models.franka_cube_stack_scene()
        spec = b.build()
        sc = MirScene(spec, n)
        assert sc.kernel == (16 if scene == "pick" else 64)
        _cache[key] = dict(b=b, spec=spec, sc=sc, o64=orc.Oracle(spec, 1), o32=orc.Oracle(spec, 1, f32=True if scene == "pick" else "big"),
                           arm=ikm_ref.Arm(spec))
    return _cache[key]


def _gpu(sc, case, **kw):
    q, err, info = sc.inverse_kinematics_multilink(case["links"], case["poss"], case["quats"], case["seed_q"], return_error=True,
                                                   return_info=True, **ikm_ref.kwargs(case), **kw)
    torch.cuda.synchronize()
    return q.cpu().numpy(), err.cpu().numpy(), info["iters"].cpu().numpy(), info["sample"].cpu().numpy()


def _residuals(s, case, q):
    """float64 masked errors (R, L, 2) at the joint rows q, and the float32 port's own discrepancy at the same q"""
    quats = case["quats"]
    e64 = np.stack([ikm_ref.masked_errors(s["o64"], s["arm"], case["links"], case["poss"][r], None if quats is None else quats[r], q[r],
                                          case["pos_mask"], case["rot_mask"]) for r in range(len(q))])
    e32 = np.stack([ikm_ref.masked_errors(s["o32"], s["arm"], case["links"], case["poss"][r], None if quats is None else quats[r], q[r],
                                          case["pos_mask"], case["rot_mask"], dtype=np.float32) for r in range(len(q))])
    return e64, np.abs(e32.astype(np.float64) - e64)


def _assert_residual(e64, disc, rows=None):
    rows = slice(None) if rows is None else rows
    assert (e64[rows, :, 0] < POS_TOL + 4 * disc[rows, :, 0]).all(), (e64[rows, :, 0].max(), disc[rows, :, 0].max())
    assert (e64[rows, :, 1] < ROT_TOL + 4 * disc[rows, :, 1]).all(), (e64[rows, :, 1].max(), disc[rows, :, 1].max())


@pytest.mark.parametrize("ci", range(len(ikm_ref.GPU_CASES)))
@pytest.mark.parametrize("scene", ["pick", "stack"])
def test_case_converges_and_matches_the_reference(scene, ci):
    s = _setup(scene)
    case = ikm_ref.build_case(s["b"], s["spec"], s["o64"], s["arm"], ikm_ref.GPU_CASES[ci], HOME, B, 100 + ci)
    ref = ikm_ref.solve(s["o64"], s["arm"], case["links"], case["poss"], case["quats"], case["seed_q"], **ikm_ref.kwargs(case))
    port = ikm_ref.solve(s["o32"], s["arm"], case["links"], case["poss"], case["quats"], case["seed_q"], dtype=np.float32, **ikm_ref.kwargs(case))
    q, err, iters, sample = _gpu(s["sc"], case)
    e64, disc = _residuals(s, case, q)
    dq, dport = np.abs(q - ref["q"]).max(1), np.abs(port["q"] - ref["q"]).max(1)
    print(f"\n{scene} / {case['name']}: err_out pos {err[:, :, 0].max():.2e} rot {err[:, :, 1].max():.2e}; float64 residual pos {e64[:, :, 0].max():.2e} "
          f"rot {e64[:, :, 1].max():.2e} (port discrepancy {disc[:, :, 0].max():.1e} / {disc[:, :, 1].max():.1e}); |q - q_ref64| max {dq.max():.2e} "
          f"median {np.median(dq):.2e} (port {dport.max():.2e} / {np.median(dport):.2e}); iters {iters.tolist()} ref {ref['iters'].tolist()}")
    # convergence on every row (the CPU tier shows the reference and the port converge on every row of every case)
    assert (err[:, :, 0] < POS_TOL).all() and (err[:, :, 1] < ROT_TOL).all(), err
    # the masked errors recomputed in float64 at the returned q
    _assert_residual(e64, disc)
    # agreement with the reference: 4 x the port's own distance, floored at the bars of tests/test_gpu_ik.py
    assert dq.max() <= max(4 * dport.max(), 5e-3), (dq.max(), dport.max())
    assert np.median(dq) <= max(4 * np.median(dport), 1e-4), (np.median(dq), np.median(dport))
    assert (iters <= MAX_ITERS).all() and (iters >= 0).all() and (sample == 0).all()
    # columns that may not move are the seed, bit for bit
    assert np.array_equal(q[:, ~case["moving"]].view(np.uint32), case["seed_q"][:, ~case["moving"]].view(np.uint32))


def test_one_link_full_masks_agrees_with_the_existing_kernel():
    s = _setup("pick")
    sc, arm = s["sc"], s["arm"]
    hand = s["b"].body_index("hand")
    case = ikm_ref.build_case(s["b"], s["spec"], s["o64"], arm, dict(name="hand pose", links=("hand",)), HOME, B, 31)
    q, err, iters, _ = _gpu(sc, case)
    q0 = sc.inverse_kinematics(hand, case["poss"][:, 0], case["quats"][:, 0], case["seed_q"]).cpu().numpy()
    free = ~(((q0 == arm.lo.astype(np.float32)) | (q0 == arm.hi.astype(np.float32)))[:, :7].any(1))   # rows where no joint ends on a limit
    assert free.sum() >= 3
    d = np.abs(q - q0)[free].max()
    print(f"\none link, full masks: max |q_multilink - q_existing| = {d:.2e} on {int(free.sum())} rows")
    assert d < 1e-3, d


def test_rows_by_env_index_and_addressing():
    s = _setup("pick")
    sc = s["sc"]
    case = ikm_ref.build_case(s["b"], s["spec"], s["o64"], s["arm"], ikm_ref.GPU_CASES[1], HOME, B, 41)
    kw = ikm_ref.kwargs(case)
    seeds = case["seed_q"] + np.random.default_rng(2).uniform(-0.05, 0.0, case["seed_q"].shape).astype(np.float32)   # (a seed per env)
    full_q, full_e, full_i = sc.inverse_kinematics_multilink(case["links"], case["poss"], case["quats"], seeds, return_error=True, return_info=True, **kw)
    dev = sc.device
    for idx in ([3, 0, 4, 1, 2], [2, 2, 0, 2], [4], [1, 3, 3, 0]):   # a permutation, a repeated index, n_rows of 1 and 4
        it = torch.tensor(idx, device=dev)
        # by row
        q, e, inf = sc.inverse_kinematics_multilink(case["links"], case["poss"][idx], case["quats"][idx], seeds[idx], env_idx=it, return_error=True,
                                                    return_info=True, **kw)
        assert torch.equal(q, full_q[it]) and torch.equal(e, full_e[it]) and torch.equal(inf["iters"], full_i["iters"][it]), idx
        # by env
        q2 = sc.inverse_kinematics_multilink(case["links"], case["poss"], case["quats"], seeds, env_idx=it,
                                             flags=IK_POS_BY_ENV | IK_QUAT_BY_ENV | IK_INIT_BY_ENV, **kw)   # (nullable outputs: only q)
        assert torch.equal(q2, full_q[it]), idx
    # one quaternion set for all rows == the same set repeated by row; the seed from the scene state where init_qpos is NULL
    one = case["quats"][0]
    qa = sc.inverse_kinematics_multilink(case["links"], case["poss"], one, seeds, flags=IK_QUAT_ONE, **kw)
    qb = sc.inverse_kinematics_multilink(case["links"], case["poss"], np.tile(one[None], (B, 1, 1)), seeds, **kw)
    assert torch.equal(qa, qb)
    q16 = sc.get_state()[0].clone()
    q16[:, :9] = torch.as_tensor(seeds, device=dev)
    sc.set_state(qpos=q16)
    qc = sc.inverse_kinematics_multilink(case["links"], case["poss"], case["quats"], None, **kw)
    qd = sc.inverse_kinematics_multilink(case["links"], case["poss"], case["quats"], seeds[:, :7], init_col0=0, init_ncols=7, **kw)
    assert torch.equal(qc, full_q) and torch.equal(qd, full_q)
    # an index outside the batch is clamped
    qe = sc.inverse_kinematics_multilink(case["links"], case["poss"][[4, 0]], case["quats"][[4, 0]], None, env_idx=torch.tensor([99, -3], device=dev), **kw)
    assert torch.equal(qe, full_q[torch.tensor([4, 0], device=dev)])
    # no rows: nothing to do
    q0 = sc.inverse_kinematics_multilink(case["links"], case["poss"][:0], case["quats"][:0], None, env_idx=torch.zeros(0, dtype=torch.long, device=dev), **kw)
    assert q0.shape == (0, 9)


def test_error_returns():
    s = _setup("pick")
    sc, b = s["sc"], s["b"]
    hand, cube = b.body_index("hand"), b.body_index("cube")
    tp = torch.zeros((B, 4, 3), device=sc.device)
    tq = torch.zeros((B, 4, 4), device=sc.device)
    tq[..., 0] = 1
    out = torch.empty((B, 9), device=sc.device)
    fn = sc.lib.mir_inverse_kinematics_multilink

    def query(links=(hand,), pos_mask=(1, 1, 1), rot_mask=(1, 1, 1), max_samples=1, rows=None):
        q = MirIkMulti()
        q.struct_size = C.sizeof(MirIkMulti)
        q.n_links = len(links)
        q.link_body[:min(len(links), 4)] = list(links)[:4]
        q.pos_mask[:], q.rot_mask[:] = list(pos_mask), list(rot_mask)
        q.max_samples = max_samples
        q.rows = rows or MirIkRows(None, 0, 0, 0, 0)
        return q

    def call(q, pos=tp, quat=tq, opt=None, o=out, h=None):
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        return fn(sc.h if h is None else h, None if q is None else C.byref(q), p(pos), p(quat), None, None if opt is None else C.byref(opt), p(o),
                  None, None, None, sc._stream())

    INVALID = -1
    assert call(query()) == 0
    assert call(query(), pos=None) == INVALID and call(query(), o=None) == INVALID and call(None) == INVALID   # null required pointers
    assert fn(None, C.byref(query()), tp.data_ptr(), None, None, None, out.data_ptr(), None, None, None, None) == INVALID
    assert call(query(links=())) == INVALID and call(query(links=(hand,) * 5)) == INVALID          # n_links outside 1 .. 4
    assert call(query(links=(0,))) == INVALID and call(query(links=(sc.nbody,))) == INVALID          # a link out of range
    assert call(query(links=(hand, cube))) == INVALID                                               # a link hanging off a free body
    for rm in ((1, 1, 0), (0, 1, 1), (1, 0, 1)):
        assert call(query(rot_mask=rm)) == INVALID                                                  # two true entries
    assert call(query(pos_mask=(0, 0, 0), rot_mask=(0, 0, 0))) == INVALID                           # no task row at all
    assert call(query(pos_mask=(0, 0, 0)), quat=None) == INVALID                                    # ... nor without a quaternion
    assert call(query(pos_mask=(0, 0, 0))) == 0                                                     # orientation rows alone are a task
    assert call(query(max_samples=0)) == INVALID
    bad = query()
    bad.struct_size -= 4
    assert call(bad) == INVALID
    for o in (MirIkOptions(0, 1, 0.05, 5e-4, 5e-3, 0.5), MirIkOptions(20, 1, 0.0, 5e-4, 5e-3, 0.5), MirIkOptions(20, 1, 0.05, 5e-4, 5e-3, 0.0)):
        assert call(query(), opt=o) == INVALID                                                      # bad options
    for r in (MirIkRows(None, 0, 0, -1, 3), MirIkRows(None, 0, 0, 7, 3), MirIkRows(None, 0, 16, 0, 0), MirIkRows(None, -1, 0, 0, 0)):
        assert call(query(rows=r)) == INVALID                                                       # bad init columns / row description
    idx = torch.zeros(1, dtype=torch.long, device=sc.device)
    assert call(query(rows=MirIkRows(idx.data_ptr(), 0, 0, 0, 0))) == 0                             # n_rows == 0
    # the Python layers refuse the same before any call
    with pytest.raises(ValueError, match="You can only align 0, 1 axis or all 3 axes."):
        make_ik_multi([hand], rot_mask=(True, True, False))
    with pytest.raises(ValueError):
        make_ik_multi([hand] * 5)
    with pytest.raises(ValueError):
        make_ik_multi([hand], max_samples=0)
    torch.cuda.synchronize()


def test_a_call_is_invisible_to_the_state_and_the_next_step():
    from gym_genesis.backend.lib import MirScene

    s = _setup("pick")
    spec = s["spec"]
    case = ikm_ref.build_case(s["b"], spec, s["o64"], s["arm"], ikm_ref.GPU_CASES[5], HOME, B, 51)
    rng = np.random.RandomState(0)
    pos = np.stack([rng.uniform(0.45, 0.8, B), rng.uniform(-0.25, 0.25, B), np.full(B, 0.02)], 1).astype(np.float32)
    quat, home = np.tile(np.array([0, 0, 0, 1], np.float32), (B, 1)), np.tile(np.asarray(HOME, np.float32), (B, 1))
    act = torch.as_tensor(home + rng.uniform(-0.3, 0.3, (B, 9)).astype(np.float32))
    finals = []
    for with_call in (False, True):
        sc = MirScene(spec, B)
        sc.reset(pos, quat, home)
        bufs = (sc.empty(sc.agent_dim), sc.empty(sc.env_dim), sc.empty(), sc.empty(dtype=torch.uint8))
        sc.step_fused(act.to(sc.device), *bufs)
        if with_call:
            before, ver = [t.clone() for t in sc.get_state()], sc.state_version
            sc.inverse_kinematics_multilink(case["links"], case["poss"], case["quats"], None, max_samples=3, **ikm_ref.kwargs(case))
            assert sc.state_version == ver and all(torch.equal(a, b) for a, b in zip(before, sc.get_state()))
        sc.step_fused(act.to(sc.device), *bufs)
        finals.append([t.clone() for t in sc.get_state()] + [b.clone() for b in bufs])
        sc.close()
    assert all(torch.equal(a, b) for a, b in zip(*finals))


def test_route_through_genesis_env():
    from gym_genesis.env import GenesisEnv

    env = GenesisEnv(task="cube_pick", robot="franka", num_envs=B, enable_pixels=False)
    env.reset(seed=0)
    robot = env.get_robot()
    mir = robot._mir
    s = _setup("pick")
    lf, rf, hand = robot.get_link("left_finger"), robot.get_link("right_finger"), robot.get_link("hand")
    case = ikm_ref.build_case(s["b"], s["spec"], s["o64"], s["arm"], ikm_ref.GPU_CASES[5], HOME, B, 61)
    dev = mir.device
    poss = [torch.as_tensor(case["poss"][:, l], device=dev) for l in range(2)]
    quats = [torch.as_tensor(case["quats"][:, l], device=dev) for l in range(2)]
    init = torch.as_tensor(case["seed_q"], device=dev)
    q, err = robot.inverse_kinematics_multilink(links=[lf, rf], poss=poss, quats=quats, init_qpos=init, return_error=True)
    assert q.shape == (B, 9) and err.shape == (B, 2, 2) and (err[:, :, 0] < POS_TOL).all() and (err[:, :, 1] < ROT_TOL).all()
    direct = mir.inverse_kinematics_multilink(case["links"], case["poss"], case["quats"], case["seed_q"])
    assert torch.equal(q, direct)
    # rows by envs_idx, every argument by row; arm dofs only: the finger columns are the seed
    idx = torch.tensor([4, 1, 1], device=dev)
    q2 = robot.inverse_kinematics_multilink([lf, rf], [p[idx] for p in poss], [t[idx] for t in quats], init_qpos=init[idx], envs_idx=idx)
    assert torch.equal(q2, q[idx])
    q3 = robot.inverse_kinematics_multilink([lf, rf], poss, quats, init_qpos=init, dofs_idx_local=list(range(7)))
    assert torch.equal(q3[:, 7:], init[:, 7:])
    # robot.inverse_kinematics with one of Genesis's further arguments goes to the same kernel with one link ...
    c3 = ikm_ref.build_case(s["b"], s["spec"], s["o64"], s["arm"], ikm_ref.GPU_CASES[2], HOME, B, 62)
    n0 = mir.__dict__.get("ik_multilink_launches", 0)
    qz, ez = robot.inverse_kinematics(link=hand, pos=torch.as_tensor(c3["poss"][:, 0], device=dev), quat=torch.as_tensor(c3["quats"][:, 0], device=dev),
                                      init_qpos=init, rot_mask=[False, False, True], return_error=True)
    assert mir.ik_multilink_launches == n0 + 1 and qz.shape == (B, 9) and ez.shape == (B, 2) and (ez[:, 0] < POS_TOL).all() and (ez[:, 1] < ROT_TOL).all()
    assert torch.equal(qz, mir.inverse_kinematics_multilink(c3["links"], c3["poss"], c3["quats"], c3["seed_q"], rot_mask=(False, False, True)))
    # ... and a call that leaves them at their defaults takes the path it always took
    n1 = mir.ik_multilink_launches
    qd = robot.inverse_kinematics(link=hand, pos=torch.as_tensor(c3["poss"][:, 0], device=dev), quat=torch.as_tensor(c3["quats"][:, 0], device=dev), init_qpos=init)
    assert mir.ik_multilink_launches == n1
    assert torch.equal(qd, mir.inverse_kinematics(c3["links"][0], c3["poss"][:, 0], c3["quats"][:, 0], c3["seed_q"]))
    with pytest.raises(ValueError, match="You can only align 0, 1 axis or all 3 axes."):
        robot.inverse_kinematics(link=hand, pos=poss[0], quat=quats[0], rot_mask=[True, True, False])
    env.close()


def test_restarts():
    n = 32
    s = _setup("pick", n)
    sc = s["sc"]
    case = ikm_ref.restart_case(s["b"], s["spec"], s["o64"], s["arm"], HOME, n, 7)
    case.update(pos_mask=(True,) * 3, rot_mask=(True,) * 3, dof_mask=None)
    ref8 = ikm_ref.solve(s["o64"], s["arm"], case["links"], case["poss"], case["quats"], case["seed_q"], max_samples=8, seed=5)
    q1, e1, i1, s1 = _gpu(sc, case, max_samples=1, seed=5)
    q8, e8, i8, s8 = _gpu(sc, case, max_samples=8, seed=5)
    conv = lambda e: (e[:, 0, 0] < POS_TOL) & (e[:, 0, 1] < ROT_TOL)  # noqa: E731
    c1, c8 = conv(e1), conv(e8)
    print(f"\nrestarts: converged {int(c1.sum())} of {n} with 1 sample, {int(c8.sum())} with 8 (reference: {int(ref8['converged'].sum())}); "
          f"samples {s8.tolist()}; iterations up to {int(i8.max())}")
    assert c8.sum() >= ref8["converged"].sum() - 2      # (1/16 of the rows: a float32 accept / reject decision that flips on a far target)
    assert c8.sum() > c1.sum()
    e64, disc = _residuals(s, case, q8)
    _assert_residual(e64, disc, rows=c8)
    assert (s1 == 0).all() and (s8 >= 0).all() and (s8 < 8).all() and (s8[c1] == 0).all()
    assert np.array_equal(q8[c1].view(np.uint32), q1[c1].view(np.uint32))   # sample 0 converged: the result is sample 0's
    assert (i8 >= i1).all() and (i1 <= MAX_ITERS).all() and (i8 <= 8 * MAX_ITERS).all()
    q8b, e8b, i8b, s8b = _gpu(sc, case, max_samples=8, seed=5)
    assert np.array_equal(q8.view(np.uint32), q8b.view(np.uint32)) and np.array_equal(e8.view(np.uint32), e8b.view(np.uint32))
    assert np.array_equal(i8, i8b) and np.array_equal(s8, s8b)
    q8c, *_ = _gpu(sc, case, max_samples=8, seed=6)
    assert (q8c != q8).any(1).any()
