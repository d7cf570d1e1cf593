"""Motion planning without a GPU: the random numbers of mir_plan_path pinned by known answers, the NumPy reference of the planner
(tests/plan_ref.py) on the cases of tests/plan_cases.py -- direct edge, failures, smoothing, the resampler, the validator -- the condition
the GPU tests lean on, and EntityView.plan_path's argument handling against a stub scene.
"""
import numpy as np
import pytest
import torch

import dist_ref
import plan_cases as pc
import plan_ref
import ray_cases


def test_mix_and_u_known_answers():
    # MurmurHash3's 32-bit finaliser: fmix32(0) = 0; the other values follow from the five steps by hand (Python integers)
    assert plan_ref.mix(0) == 0
    assert plan_ref.mix(1) == 0x514E28B7 and plan_ref.mix(0xFFFFFFFF) == 0x81F16F39
    x = 1
    x ^= x >> 16; x = (x * 0x85EBCA6B) % 2 ** 32; x ^= x >> 13; x = (x * 0xC2B2AE35) % 2 ** 32; x ^= x >> 16
    assert x == plan_ref.mix(1)
    v = plan_ref.u(5, 3, 7, 2)
    assert v.dtype == np.float32 and float(v) == (plan_ref.mix(plan_ref.mix(plan_ref.mix(5 ^ 3) ^ 7) ^ 2) >> 8) / 2 ** 24
    us = np.array([plan_ref.u(0, e, c, j) for e in range(4) for c in (0, 1, 0x80000000) for j in range(9)], np.float64)
    assert (us >= 0).all() and (us < 1).all() and len(set(us.tolist())) == len(us) and 0.3 < us.mean() < 0.7
    assert plan_ref.u(1, 2, 0, 0) == plan_ref.u(2, 1, 0, 0), "keyed by seed ^ env"


def test_forward_kinematics_and_clearance_against_the_oracle():
    """plan_ref's own forward kinematics against the oracle's, and its clearance against dist_ref.signed_distance on the oracle's poses.
    The oracle normalises every quaternion it composes; plan_ref, like the library's query kernels, composes the spec's quaternions as
    they are, and the Panda's link quaternions are unit quaternions to seven digits only: 1e-7 m of difference, not 1e-12."""
    c = pc.case("post")
    pb = pc.problem("post")
    q = c["q"].copy()
    q[:, c["qadr"]] = c["goal"]
    xp, xq = ray_cases.poses(c["spec"], q)
    ref = dist_ref.signed_distance(dist_ref.Scene(c["spec"]), xp, xq, c["probes"], c["links"], 1.0, c["skip"], with_ambiguous=False)
    for r in range(pc.B):
        pb.set_row(c["q"][r])
        got = pb.clearance(c["goal"][r].astype(np.float64))
        assert np.abs(pb.xp - xp[r]).max() < 2e-7 and min(np.abs(pb.xq - xq[r]).max(), np.abs(pb.xq + xq[r]).max()) < 2e-7
        assert abs(got - ref["row_min"][r]) < 2e-7


def test_cases_are_what_they_say():
    for name in ("post", "clear", "sealed"):
        c, pb = pc.case(name), pc.problem(name)
        for r in range(pc.B):
            s = pb.set_row(c["q"][r])
            g = c["goal"][r].astype(np.float64)
            seg, _ = plan_ref.polyline_clearance(pb, c["q"][r], [s, g], pc.RESOLUTION)
            cs, cg = pb.clearance(s), pb.clearance(g)
            if name == "sealed":
                assert cs > 0.01 and cg > 0.01 and seg.min() < -0.01, (name, r, cs, cg, seg.min())
            else:
                assert cs >= 0.02 and cg >= 0.02, (name, r, cs, cg)
                assert seg.min() >= 0.02 if name == "clear" else seg.min() <= -0.01, (name, r, seg.min())
            assert (g >= pb.lo).all() and (g <= pb.hi).all()


def test_direct_edge_and_failures():
    c = pc.case("clear")
    for dt in ("float64", "float32"):
        r = pc.reference("clear", 2, 0, dt)
        assert r["status"] == plan_ref.OK and r["iterations"] == 0 and len(r["poly"]) == 2 and r["nodes"] == (1, 1)
        assert np.array_equal(r["path"][0].astype(np.float32), c["start"][2]) and np.array_equal(r["path"][-1].astype(np.float32), c["goal"][2])
    c = pc.case("post")
    pb = pc.problem("post")
    pb.set_row(c["q"][0])
    deep = min(plan_ref.edge_samples(c["start"][0].astype(np.float64), c["goal"][0].astype(np.float64), pc.RESOLUTION, np.float64), key=pb.clearance)
    kw = dict(W=8, max_nodes=16, max_iterations=8)
    q = c["q"][0].copy()
    q[c["qadr"]] = deep
    r = plan_ref.plan(pb, q, c["goal"][0], 0, **kw)
    assert r["status"] == plan_ref.START_IN_COLLISION and np.array_equal(r["path"], np.repeat(deep[None].astype(np.float32).astype(np.float64), 8, 0))
    assert plan_ref.plan(pb, c["q"][0], deep, 0, **kw)["status"] == plan_ref.GOAL_IN_COLLISION
    out = c["goal"][0].copy()
    out[0] = 3.0
    r = plan_ref.plan(pb, c["q"][0], out, 0, **kw)
    assert r["status"] == plan_ref.GOAL_OUT_OF_LIMITS and len(r["poly"]) == 1 and r["checked"] == 0
    r = plan_ref.plan(pb, c["q"][0], c["goal"][0], 0, ignore_collision=True, **kw)
    assert r["status"] == plan_ref.OK and len(r["poly"]) == 2 and r["checked"] == 0
    # the budgets of the GPU test's failure rows, in both precisions
    for dt in ("float64", "float32"):
        for row in range(pc.B):
            assert pc.reference("sealed", row, 0, dt, max_iterations=32)["status"] == plan_ref.ITERATION_LIMIT
            few = pc.reference("post", row, 0, dt, max_nodes=4)
            assert few["status"] == plan_ref.NODE_LIMIT and max(few["nodes"]) == 4, (row, few["status"], few["nodes"])


def test_resampler():
    rng = np.random.default_rng(5)
    poly = np.cumsum(rng.uniform(-0.4, 0.4, (6, 9)), 0)
    for dt in (np.float64, np.float32):
        p = poly.astype(dt)
        out = plan_ref.resample(p, 23, dt)
        assert out.dtype == dt and np.array_equal(out[0], p[0]) and np.array_equal(out[-1], p[-1])
    out = plan_ref.resample(poly, 23, np.float64)
    # every waypoint lies on the polyline, at equal steps of its arc length
    cum = np.concatenate([[0], np.cumsum(np.linalg.norm(np.diff(poly, axis=0), axis=1))])
    arc = []
    for w in out:
        best = None
        for k in range(5):
            d = poly[k + 1] - poly[k]
            t = np.clip((w - poly[k]) @ d / (d @ d), 0, 1)
            e = np.linalg.norm(poly[k] + t * d - w)
            if best is None or e < best[0]:
                best = (e, cum[k] + t * np.linalg.norm(d))
        assert best[0] < 1e-12
        arc.append(best[1])
    assert np.abs(np.diff(arc) - cum[-1] / 22).max() < 1e-12
    two = plan_ref.resample(poly[:2], 5, np.float64)
    assert np.abs(two - np.stack([poly[0] + (w / 4) * (poly[1] - poly[0]) for w in range(5)])).max() < 1e-15
    assert np.array_equal(plan_ref.resample(poly[:1], 4, np.float64), np.repeat(poly[:1], 4, 0))


def test_the_condition_the_gpu_test_leans_on():
    """on "post", every row, seeds 0, 1, 2: the float64 reference and the float32 port finish with iterations <= max_iterations / 4 and
    nodes <= max_nodes / 2; the validator accepts the reference's own polylines, the straight line it does not"""
    worst_it, worst_n = 0, 0
    for dt in ("float64", "float32"):
        for seed in (0, 1, 2):
            for row in range(pc.B):
                r = pc.reference("post", row, seed, dt)
                assert r["status"] == plan_ref.OK and len(r["poly"]) >= 3, (dt, seed, row, r["status"])
                worst_it, worst_n = max(worst_it, r["iterations"]), max(worst_n, *r["nodes"])
                if seed == 0:
                    ok, low = pc.valid_polyline("post", row, r["poly"], tol=0.0 if dt == "float64" else 1e-5)
                    assert ok, (dt, row, low)
    print(f"\n[plan, post] most iterations {worst_it} of {pc.BUDGET['max_iterations']}, most nodes {worst_n} of {pc.BUDGET['max_nodes']}")
    assert worst_it <= pc.BUDGET["max_iterations"] // 4 and worst_n <= pc.BUDGET["max_nodes"] // 2
    c = pc.case("post")
    assert not pc.valid_polyline("post", 0, np.stack([c["start"][0], c["goal"][0]]))[0]
    assert not pc.valid_polyline("post", 0, pc.reference("post", 1)["poly"])[0], "another row's polyline does not start here"


def test_smoothing_of_the_reference():
    for row in range(pc.B):
        rough, smooth = pc.reference("post", row, 0, "float64", smooth_passes=0), pc.reference("post", row)
        assert len(smooth["poly"]) <= len(rough["poly"]) and plan_ref.polyline_length(smooth["poly"]) <= plan_ref.polyline_length(rough["poly"]) + 1e-12
        assert pc.valid_polyline("post", row, rough["poly"])[0]
        assert smooth["iterations"] == rough["iterations"] and smooth["nodes"] == rough["nodes"]
    assert any(len(pc.reference("post", r, 0, "float64", smooth_passes=0)["poly"]) > len(pc.reference("post", r)["poly"]) for r in range(pc.B))


class _StubScene:
    """what EntityView.plan_path asks of a scene: records the call"""
    num_envs, device, nq = pc.B, torch.device("cpu"), 16

    def __init__(self):
        self.calls = []
        self.q = torch.zeros((pc.B, 16))

    def get_state(self):
        return (self.q, None, None, None)

    def plan_path(self, **kw):
        self.calls.append(("plan", kw))
        R, W, D = kw["qpos_goal"].shape[0], kw["num_waypoints"], len(kw["dof_qadr"])
        return {"path": torch.arange(R * W * D, dtype=torch.float32).reshape(R, W, D), "status": torch.tensor([0] * (R - 1) + [5], dtype=torch.int32),
                "poly": torch.zeros((R, 128, D)), "n_poly": torch.ones(R, dtype=torch.int32), "stats": torch.zeros((R, 4), dtype=torch.int32)}

    def path_clearance(self, **kw):
        self.calls.append(("clearance", kw))
        R, K = kw["paths"].shape[:2]
        return {"seg_min": torch.zeros((R, K - 1)), "row_min": torch.tensor([0.02] * (R - 1) + [-0.01]), "row_first_blocked": torch.full((R,), -1, dtype=torch.int32)}


def test_entity_view_argument_handling():
    from gym_genesis.tasks.views import EntityView

    c = pc.case("post")
    st = _StubScene()
    robot, cube = pc.arm(c["sb"], st), EntityView(st, c["sb"], "cube", ())
    goal = torch.as_tensor(c["goal"])
    path = robot.plan_path(goal)
    kind, kw = st.calls[-1]
    assert path.shape == (100, pc.B, 9) and torch.equal(path[:, 2], torch.arange(pc.B * 900, dtype=torch.float32).reshape(pc.B, 100, 9)[2])
    assert kw["skip_geoms"] == robot._own_geoms() and kw["smooth_passes"] == 64 and kw["max_nodes"] == 256 and kw["max_iterations"] == 2000
    assert kw["qpos_start"] is None and kw["env_idx"] is None and list(kw["dof_qadr"]) == list(range(9)) and not kw["ignore_collision"]
    assert kw["resolution"] == 0.05 and kw["step"] == 0.3 and kw["margin"] == 0.0 and kw["seed"] == 0 and len(kw["links"]) == len(c["links"])
    p, valid = robot.plan_path(goal[:2], qpos_start=torch.as_tensor(c["start"][:2]), envs_idx=[4, 0], smooth_path=False, num_waypoints=7, ignore_collision=True,
                               return_valid_mask=True, timeout=3.0, margin=0.6, ignore_entities=[cube], seed=9)
    kind, kw = st.calls[-1]
    assert p.shape == (7, 2, 9) and valid.tolist() == [True, False]
    assert kw["smooth_passes"] == 0 and kw["ignore_collision"] and kw["env_idx"].tolist() == [4, 0] and kw["seed"] == 9 and kw["max_distance"] == 1.2
    assert kw["skip_geoms"] == robot._own_geoms() | cube._own_geoms() and kw["qpos_start"].shape == (2, 16)
    assert torch.equal(kw["qpos_start"][:, :9], torch.as_tensor(c["start"][:2]))
    robot.plan_path(goal, with_entity=cube)
    assert st.calls[-1][1]["skip_geoms"] == ((1 << len(c["sb"].geoms)) - 1) & ~cube._own_geoms() | robot._own_geoms()
    det = robot.plan_path(goal, return_detail=True)
    assert sorted(det) == ["n_poly", "path", "poly", "stats", "status", "valid"]
    with pytest.raises(NotImplementedError):
        robot.plan_path(goal, planner="PRM")
    with pytest.raises(ValueError):
        robot.plan_path(goal[:, :7])
    flag = robot.path_in_collision(path, margin=0.0)
    assert st.calls[-1][0] == "clearance" and st.calls[-1][1]["paths"].shape == (pc.B, 100, 9) and flag.tolist() == [False] * (pc.B - 1) + [True]
    with pytest.raises(ValueError):
        robot.get_path_clearance(path[:1])


def test_unbatched_stack_task_plans_without_an_env_axis(monkeypatch):
    """GenesisEnv(num_envs=0) -> FrankaCubeStackOne: robot.plan_path gives (W, n), and every companion result drops the env axis"""
    import fake_scene
    from gym_genesis.env import GenesisEnv
    from gym_genesis.tasks import stack_common

    class Scene(fake_scene.OracleScene):
        plan_path, path_clearance = _StubScene.plan_path, _StubScene.path_clearance
        calls = []

    monkeypatch.setattr(stack_common, "MirScene", Scene)
    env = GenesisEnv(task="cube_stack", robot="franka", num_envs=0, enable_pixels=False)
    env.reset(seed=2)
    robot = env.get_robot()
    assert type(env._env).__name__ == "FrankaCubeStackOne" and robot.unbatched
    goal = torch.as_tensor(env._env._home_qpos(), dtype=torch.float32)
    path = robot.plan_path(qpos_goal=goal, num_waypoints=5)
    assert path.shape == (5, 9) and Scene.calls[-1][1]["qpos_goal"].shape == (1, 9)
    path, valid = robot.plan_path(goal, num_waypoints=5, return_valid_mask=True)
    assert path.shape == (5, 9) and valid.dim() == 0
    det = robot.plan_path(goal, num_waypoints=5, return_detail=True)
    assert det["path"].shape == (5, 9) and det["status"].dim() == 0 and det["poly"].shape == (128, 9) and det["n_poly"].dim() == 0 and det["stats"].shape == (4,)
    clear = robot.get_path_clearance(path)
    assert clear.dim() == 0 and Scene.calls[-1][1]["paths"].shape == (1, 5, 9)
    d = robot.get_path_clearance(path, return_detail=True)
    assert d["seg_min"].shape == (4,) and d["first_blocked"].dim() == 0 and robot.path_in_collision(path).dim() == 0
