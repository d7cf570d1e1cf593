"""CPU-tier tests of the multi-link inverse kinematics: the float64 reference tests/ikm_ref.py (the checker of
mir_inverse_kinematics_multilink) against the oracle's single-link solver and against forward kinematics, the sample hash, the
conditions under which tests/test_gpu_ikm.py may demand convergence on every row, the restart counts, and the views' argument
handling on an oracle-backed test double.

Restart counts computed by this file (32 hand poses at configurations uniform over the arm's whole joint ranges, seed = home pose):
the float64 reference converges 26 rows with one sample and 32 with eight; the float32 port the same."""
import numpy as np
import pytest
import torch

import fake_scene
import ikm_ref
import orc
from gym_genesis.backend import models

HOME = models.FRANKA_HOME
POS_TOL, ROT_TOL, MAX_ITERS = 5e-4, 5e-3, 20


@pytest.fixture(scope="module")
def pick():
    b = models.franka_cube_pick_scene()
    spec = b.build()
    return dict(b=b, spec=spec, o64=orc.Oracle(spec, 1), o32=orc.Oracle(spec, 1, f32=True), arm=ikm_ref.Arm(spec))


@pytest.fixture(scope="module")
def stack():
    b = models.franka_cube_stack_scene()
    spec = b.build()
    return dict(b=b, spec=spec, o64=orc.Oracle(spec, 1), o32=orc.Oracle(spec, 1, f32="big"), arm=ikm_ref.Arm(spec))


def _solve(s, case, port=False, **kw):
    return ikm_ref.solve(s["o32" if port else "o64"], s["arm"], case["links"], case["poss"], case["quats"], case["seed_q"],
                         dtype=np.float32 if port else np.float64, **ikm_ref.kwargs(case), **kw)


def test_one_link_full_masks_is_the_oracles_iteration(pick):
    n = 8
    hand, arm, o = pick["b"].body_index("hand"), pick["arm"], pick["o64"]
    qt = ikm_ref.arm_configs(HOME, n, np.random.default_rng(0))
    poses = [ikm_ref.link_poses(o, arm, [hand], q) for q in qt]
    tp, tq = np.stack([p[0] for p, _ in poses]), np.stack([q[0] for _, q in poses])
    seed = np.tile(np.asarray(HOME, np.float64), (n, 1))
    qo, erro = o.ik(hand, tp, tq, seed)
    iters_o = o.ik_iters.copy()
    r = ikm_ref.solve(o, arm, [hand], tp[:, None], tq[:, None], seed)
    assert not ((qo[:, :7] == arm.lo[:7]) | (qo[:, :7] == arm.hi[:7])).any()    # no joint on a limit: the limit rule is idle
    assert r["converged"].all() and (erro[:, 0] < POS_TOL).all() and (erro[:, 1] < ROT_TOL).all()
    d = np.abs(r["q"] - qo).max()
    print(f"reference against orc_ik: {d:.2e}")
    assert d < 1e-6, d
    assert np.array_equal(r["iters"], iters_o)
    # position only as well
    qo2, _ = o.ik(hand, tp, None, seed)
    r2 = ikm_ref.solve(o, arm, [hand], tp[:, None], None, seed)
    assert np.abs(r2["q"] - qo2).max() < 1e-6 and np.array_equal(r2["iters"], o.ik_iters)


@pytest.mark.parametrize("scene", ["pick", "stack"])
def test_gpu_cases_converge_in_the_reference_and_in_the_port(scene, request):
    """the condition that lets tests/test_gpu_ikm.py demand convergence on every row: every case converges on every row, in float64 and
    in the float32 port, in at most half of max_iters; the result meets the masked targets under float64 forward kinematics; the
    joints off the chains and outside the dof subset are the seed, bit for bit"""
    s = request.getfixturevalue(scene)
    for ci, c in enumerate(ikm_ref.GPU_CASES):
        case = ikm_ref.build_case(s["b"], s["spec"], s["o64"], s["arm"], c, HOME, 5, 100 + ci)
        for port in (False, True):
            r = _solve(s, case, port)
            assert r["converged"].all(), (scene, c["name"], port)
            assert (r["iters"] <= MAX_ITERS // 2).all(), (scene, c["name"], port, r["iters"])
            assert (r["err"][:, :, 0] < POS_TOL).all() and (r["err"][:, :, 1] < ROT_TOL).all()
            # bit for bit: columns that may not move (compared in the dtype of the solve)
            dt = np.float32 if port else np.float64
            assert np.array_equal(r["q"][:, ~case["moving"]].astype(dt), case["seed_q"][:, ~case["moving"]].astype(dt))
            assert (r["q"][:, case["moving"]] != case["seed_q"][:, case["moving"]]).any()
            for row in range(5):
                e = ikm_ref.masked_errors(s["o64"], s["arm"], case["links"], case["poss"][row], None if case["quats"] is None else case["quats"][row],
                                          r["q"][row], case["pos_mask"], case["rot_mask"])
                assert (e[:, 0] < POS_TOL + (1e-6 if port else 0)).all() and (e[:, 1] < ROT_TOL + (1e-5 if port else 0)).all(), (c["name"], e)


def test_masked_targets_mean_what_the_header_says(pick):
    """the masks checked without the reference's own error function: the link's z axis on the target's, the masked position
    components on the target's, and the free ones left free"""
    s = pick
    hand = s["b"].body_index("hand")
    import kin_ref

    for ci in (2, 3):
        case = ikm_ref.build_case(s["b"], s["spec"], s["o64"], s["arm"], ikm_ref.GPU_CASES[ci], HOME, 5, 100 + ci)
        r = _solve(s, case)
        k = int(np.argmax(case["rot_mask"]))
        pm = np.array(case["pos_mask"])
        free_rot = 0.0
        for row in range(5):
            p, q = ikm_ref.link_poses(s["o64"], s["arm"], [hand], r["q"][row])
            a = kin_ref.quat_to_mat(q[0])[:, k]
            tq = case["quats"][row, 0].astype(np.float64)
            at = kin_ref.quat_to_mat(tq / np.linalg.norm(tq))[:, k]
            assert np.arccos(np.clip(a @ at, -1, 1)) < ROT_TOL
            assert np.linalg.norm((p[0] - case["poss"][row, 0])[pm]) < POS_TOL
            other = kin_ref.quat_to_mat(q[0])[:, (k + 1) % 3] @ kin_ref.quat_to_mat(tq / np.linalg.norm(tq))[:, (k + 1) % 3]
            free_rot = max(free_rot, np.arccos(np.clip(other, -1, 1)))
        assert free_rot > 10 * ROT_TOL   # the rotation about the aligned axis is free: some row uses the freedom


def test_limit_rule_is_what_makes_the_two_finger_case_converge(pick):
    """both fingertips, all nine dofs, finger targets inside 0 .. 0.04: with the limit rule every row converges in a few iterations;
    a joint on its range stops being asked to move past it"""
    s = pick
    case = ikm_ref.build_case(s["b"], s["spec"], s["o64"], s["arm"], ikm_ref.GPU_CASES[5], HOME, 16, 9)
    r = _solve(s, case)
    assert r["converged"].all() and r["iters"].max() <= 6, r["iters"]
    lo, hi = s["arm"].lo, s["arm"].hi
    assert (r["q"] >= lo).all() and (r["q"] <= hi).all()


def test_hash_known_values():
    # (seed, env, sample, column) -> x >> 8, from the header's recipe compiled as C with uint32_t arithmetic
    for args, want in (((0, 0, 1, 0), 2662513), ((1, 2, 3, 4), 1988290), ((12345, 4095, 7, 8), 8717670)):
        u = ikm_ref.hash_u(*args)
        assert u == want * 2.0 ** -24 and 0.0 <= u < 1.0
        assert np.float32(u) == u   # 24 bits: exact in float32
    # env and not the row enters: two rows of the same env draw the same sample
    assert ikm_ref.hash_u(3, 5, 1, 2) != ikm_ref.hash_u(3, 6, 1, 2)


def test_restarts_converge_more_rows(pick):
    s = pick
    n = 32
    case = ikm_ref.restart_case(s["b"], s["spec"], s["o64"], s["arm"], HOME, n, 7)
    case.update(pos_mask=(True,) * 3, rot_mask=(True,) * 3, dof_mask=None)
    counts = {}
    for port in (False, True):
        for ms in (1, 8):
            r = _solve(s, case, port, max_samples=ms, seed=5)
            counts[port, ms] = int(r["converged"].sum())
            assert (r["sample"] < ms).all() and (r["iters"] <= ms * MAX_ITERS).all()
            if ms == 8:
                r1 = _solve(s, case, port, max_samples=1, seed=5)
                c1 = r1["converged"]
                assert (r["sample"][c1] == 0).all() and np.array_equal(r["q"][c1], r1["q"][c1])
                again = _solve(s, case, port, max_samples=8, seed=5)
                assert np.array_equal(again["q"], r["q"]) and np.array_equal(again["sample"], r["sample"])
    print(f"restarts, converged of {n}: reference {counts[False, 1]} -> {counts[False, 8]}, port {counts[True, 1]} -> {counts[True, 8]}")
    assert counts[False, 8] > counts[False, 1] and counts[True, 8] > counts[True, 1]
    assert abs(counts[True, 8] - counts[False, 8]) <= 2 and abs(counts[True, 1] - counts[False, 1]) <= 2


class IkmScene(fake_scene.OracleScene):
    """the oracle-backed double with MirScene.inverse_kinematics_multilink restated on tests/ikm_ref.py (NumPy indexing around the
    reference's solver, the row rules of include/mirigid.h); it records what the views passed"""

    def inverse_kinematics_multilink(self, links, poss, quats=None, init_qpos=None, env_idx=None, flags=0, init_col0=0, init_ncols=0,
                                     pos_mask=(True,) * 3, rot_mask=(True,) * 3, dof_mask=None, max_samples=1, seed=0, return_error=False,
                                     return_info=False, **opts):
        Bn, L = self.num_envs, len(links)
        idx = np.arange(Bn) if env_idx is None else np.clip(self._np(env_idx).astype(np.int64).reshape(-1), 0, Bn - 1)
        n = idx.size
        P = self._np(poss).reshape(-1, L, 3)
        P = P[idx] if flags & 1 else P[:n]
        Q = None
        if quats is not None:
            Qa = self._np(quats).reshape(-1, L, 4)
            Q = np.tile(Qa[:1], (n, 1, 1)) if flags & 4 else (Qa[idx] if flags & 2 else Qa[:n])
        seed_q = self.get_state()[0][:, :self.n_arm].numpy()[idx].copy()
        if init_qpos is not None:
            nc = init_ncols or self.n_arm
            I = self._np(init_qpos).reshape(-1, nc)
            seed_q[:, init_col0:init_col0 + nc] = I[idx] if flags & 8 else I[:n]
        self.last = dict(links=list(links), n=n, flags=flags, pos_mask=tuple(pos_mask), rot_mask=tuple(rot_mask), dof_mask=dof_mask,
                         max_samples=max_samples, seed=seed, init_col0=init_col0, init_ncols=init_ncols, opts=opts)
        self.calls = getattr(self, "calls", 0) + 1
        o = orc.Oracle(self.spec, 1)
        r = ikm_ref.solve(o, ikm_ref.Arm(self.spec), links, P, Q, seed_q, envs=idx, pos_mask=pos_mask, rot_mask=rot_mask, dof_mask=dof_mask,
                          max_samples=max_samples, seed=seed, **opts)
        res = (torch.from_numpy(r["q"].astype(np.float32)),)
        if return_error:
            res += (torch.from_numpy(r["err"].astype(np.float32)),)
        if return_info:
            res += ({"iters": torch.from_numpy(r["iters"].astype(np.int32)), "sample": torch.from_numpy(r["sample"].astype(np.int32))},)
        return res if len(res) > 1 else res[0]


def test_views_argument_handling_on_the_test_double(monkeypatch, pick):
    from gym_genesis.env import GenesisEnv
    from gym_genesis.tasks.franka import cube_pick

    monkeypatch.setattr(cube_pick, "MirScene", IkmScene)
    Bn = 3
    env = GenesisEnv(task="cube_pick", robot="franka", num_envs=Bn, enable_pixels=False)
    env.reset(seed=0)
    robot = env.get_robot()
    mir = robot._mir
    s = pick
    lf, rf, hand = robot.get_link("left_finger"), robot.get_link("right_finger"), robot.get_link("hand")
    case = ikm_ref.build_case(s["b"], s["spec"], s["o64"], s["arm"], ikm_ref.GPU_CASES[5], HOME, Bn, 71)
    poss = [torch.from_numpy(case["poss"][:, l]) for l in range(2)]
    quats = [torch.from_numpy(case["quats"][:, l]) for l in range(2)]
    init = torch.from_numpy(case["seed_q"])
    # all envs, by env; LinkViews resolved to body indices; (R, n_dofs) and (R, L, 2)
    q, err = robot.inverse_kinematics_multilink(links=[lf, rf], poss=poss, quats=quats, init_qpos=init, return_error=True)
    assert q.shape == (Bn, 9) and q.dtype == torch.float32 and err.shape == (Bn, 2, 2)
    assert mir.last["links"] == case["links"] and mir.last["n"] == Bn and mir.last["flags"] == 0 and mir.last["dof_mask"] is None
    assert (err[:, :, 0] < POS_TOL).all() and (err[:, :, 1] < ROT_TOL).all()
    ref = _solve(s, case)
    assert np.abs(q.numpy() - ref["q"]).max() < 1e-6
    # rows by envs_idx (a list, a repeated index): every argument by row
    idx = [2, 0, 2]
    q2 = robot.inverse_kinematics_multilink([lf, rf], [p[idx] for p in poss], [t[idx] for t in quats], init_qpos=init[idx], envs_idx=idx)
    assert torch.equal(q2, q[idx]) and mir.last["n"] == 3
    with pytest.raises(ValueError):   # full-batch arguments beside a shorter envs_idx are not rows
        robot.inverse_kinematics_multilink([lf, rf], poss, quats, envs_idx=[1, 2])
    with pytest.raises(IndexError):
        robot.inverse_kinematics_multilink([lf, rf], poss, quats, envs_idx=[0, 1, Bn])
    with pytest.raises(ValueError):   # one entry per link
        robot.inverse_kinematics_multilink([lf, rf], poss[:1], quats)
    # local link indices; one quaternion for all links and rows; dofs_idx_local -> a mask over the joint columns; options pass through
    one = [0.0, 1.0, 0.0, 0.0]
    q3 = robot.inverse_kinematics_multilink([robot.link_idx.index(lf.idx), robot.link_idx.index(rf.idx)], poss, one, dofs_idx_local=[0, 1, 2, 3, 4, 5, 6],
                                            max_samples=2, seed=9, max_iters=7)
    assert mir.last["links"] == case["links"] and mir.last["flags"] == 4 and mir.last["dof_mask"] == [True] * 7 + [False] * 2
    assert mir.last["max_samples"] == 2 and mir.last["seed"] == 9 and mir.last["opts"] == {"max_iters": 7}
    assert torch.equal(q3[:, 7:], robot.get_qpos()[:, 7:])   # the seed (the current state), bit for bit
    with pytest.raises(IndexError):
        robot.inverse_kinematics_multilink([lf], poss[:1], None, dofs_idx_local=[9])
    with pytest.raises(ValueError, match="You can only align 0, 1 axis or all 3 axes."):
        robot.inverse_kinematics_multilink([lf, rf], poss, quats, rot_mask=(True, False, True))
    # robot.inverse_kinematics: the defaults take the path they always took, any of the five further arguments the new one
    n0 = mir.calls
    c3 = ikm_ref.build_case(s["b"], s["spec"], s["o64"], s["arm"], ikm_ref.GPU_CASES[2], HOME, Bn, 72)
    p3, t3 = torch.from_numpy(c3["poss"][:, 0]), torch.from_numpy(c3["quats"][:, 0])
    qd = robot.inverse_kinematics(link=hand, pos=p3, quat=t3, init_qpos=init)
    assert mir.calls == n0 and qd.shape == (Bn, 9)
    qz, ez = robot.inverse_kinematics(link=hand, pos=p3, quat=t3, init_qpos=init, rot_mask=[False, False, True], return_error=True)
    assert mir.calls == n0 + 1 and qz.shape == (Bn, 9) and ez.shape == (Bn, 2)
    assert mir.last["links"] == [hand.idx] and mir.last["rot_mask"] == (False, False, True) and mir.last["pos_mask"] == (True, True, True)
    for kw in (dict(pos_mask=[True, True, False]), dict(dofs_idx_local=[0, 1, 2, 3]), dict(max_samples=2), dict(seed=1)):
        robot.inverse_kinematics(link=hand, pos=p3, quat=t3, init_qpos=init, **kw)
    assert mir.calls == n0 + 5
    sub = robot.inverse_kinematics(link=hand, pos=p3[1:2], quat=t3[1:2], envs_idx=[1], max_samples=2)
    assert sub.shape == (1, 9)
    with pytest.raises(ValueError, match="You can only align 0, 1 axis or all 3 axes."):
        robot.inverse_kinematics(link=hand, pos=p3, quat=t3, rot_mask=[True, True, False])
    # a scene without the entry point says so
    monkeypatch.delattr(IkmScene, "inverse_kinematics_multilink")
    with pytest.raises(NotImplementedError):
        robot.inverse_kinematics_multilink([lf, rf], poss, quats)
