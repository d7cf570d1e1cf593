"""Goal-set planning without a GPU: the NumPy reference of mir_plan_path_goals (tests/goal_ref.py) on the goal sets of
tests/goal_cases.py -- that the cases are what they say, that one goal is plan_ref.plan itself, the direct edge to the nearer goal, the
rejected goals, n_goals -- the condition the GPU tests lean on, and EntityView.plan_path_to_goals's argument handling against a stub.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import goal_cases as gc
import goal_ref
import plan_cases as pc
import plan_ref
from gym_genesis.backend import spec as S

DTYPES = ("float64", "float32")


def test_status_and_struct():
    assert S.PLAN_GOAL_STATUS[S.PLAN_NO_VALID_GOAL] == "NO_VALID_GOAL" and S.PLAN_NO_VALID_GOAL == goal_ref.NO_VALID_GOAL == 9
    assert S.PLAN_GOAL_STATUS[:9] == S.PLAN_STATUS and len(S.PLAN_GOAL_STATUS) == 10
    assert S.PLAN_MAX_GOALS == goal_ref.MAX_GOALS == 8
    q = S.make_goal_query(3)
    assert q.struct_size == C.sizeof(S.MirGoalQuery) == 16 and q.max_goals == 3 and q.flags == 0


def test_cases_are_what_they_say():
    c, pb = pc.case("post"), pc.problem("post")
    for r in range(gc.B):
        s = pb.set_row(c["q"][r])
        mid, out, far = gc.goals("bad_first")[r].astype(np.float64)
        assert pb.clearance(mid) <= -0.01 and (mid >= pb.lo).all() and (mid <= pb.hi).all(), (r, pb.clearance(mid))
        assert out[0] > pb.hi[0] + 0.09 and np.array_equal(out[1:], far[1:])
        assert np.array_equal(gc.goals("all_bad")[r], gc.goals("bad_first")[r, :2])
        for g in gc.goals("two_detours")[r].astype(np.float64):
            seg, _ = plan_ref.polyline_clearance(pb, c["q"][r], [s, g], pc.RESOLUTION)
            assert pb.clearance(g) >= 0.01 and seg.min() <= -0.01 and (g >= pb.lo).all() and (g <= pb.hi).all(), (r, pb.clearance(g), seg.min())
        assert not np.array_equal(*gc.goals("two_detours")[r])
        far, near = gc.goals("near_far")[r]
        assert np.array_equal(gc.goals("far_near")[r], np.stack([near, far]))
        d = lambda g: float(((g.astype(np.float64) - s) ** 2).sum())   # noqa: E731
        assert d(near) < 0.5 * d(far), "the goal with the clear edge is also the nearer one"


def test_one_goal_is_the_planner_itself():
    """the forest with one root changes nothing: every field of plan_ref.plan, in both precisions"""
    c = pc.case("post")
    for dt in DTYPES:
        for r in range(gc.B):
            ref = pc.reference("post", r, 0, dt)
            got = goal_ref.plan_goals(pc.problem("post", np.dtype(dt).type), c["q"][r], c["goal"][r][None], r, W=pc.BUDGET["W"],
                                      max_nodes=pc.BUDGET["max_nodes"], max_iterations=pc.BUDGET["max_iterations"], resolution=pc.RESOLUTION,
                                      step=pc.STEP, margin=pc.MARGIN)
            assert got["status"] == ref["status"] == plan_ref.OK and got["goal_index"] == 0 and got["goal_status"].tolist() == [0]
            assert np.array_equal(got["poly"], ref["poly"]) and np.array_equal(got["path"], ref["path"])
            assert (got["iterations"], got["nodes"], got["checked"]) == (ref["iterations"], ref["nodes"], ref["checked"])


@pytest.mark.parametrize("name", ["near_far", "far_near"])
def test_near_far_is_the_direct_edge(name):
    c = pc.case("post")
    near = 1 if name == "near_far" else 0
    for dt in DTYPES:
        for r in range(gc.B):
            got = gc.reference(name, r, 0, dt)
            assert got["status"] == plan_ref.OK and got["iterations"] == 0 and len(got["poly"]) == 2 and got["goal_index"] == near, (dt, r, got["status"])
            assert got["goal_status"].tolist() == [0, 0] and got["nodes"] == (1, 1)
            assert np.array_equal(got["path"][-1].astype(np.float32), gc.goals(name)[r, near]) and np.array_equal(got["path"][0].astype(np.float32), c["start"][r])


def test_the_condition_the_gpu_test_leans_on():
    """"two_detours" and "bad_first", every row, both precisions: status OK within a quarter of max_iterations and half of max_nodes;
    the validator accepts the reference's own polylines"""
    worst_it, worst_n = 0, 0
    for name in ("two_detours", "bad_first"):
        for dt in DTYPES:
            for r in range(gc.B):
                got = gc.reference(name, r, 0, dt)
                assert got["status"] == plan_ref.OK and len(got["poly"]) >= 3, (name, dt, r, got["status"])
                worst_it, worst_n = max(worst_it, got["iterations"]), max(worst_n, *got["nodes"])
                gi = got["goal_index"]
                if name == "bad_first":
                    assert got["goal_status"].tolist() == [plan_ref.GOAL_IN_COLLISION, plan_ref.GOAL_OUT_OF_LIMITS, plan_ref.OK] and gi == 2
                else:
                    assert got["goal_status"].tolist() == [0, 0] and gi in (0, 1)
                ok, low, _ = gc.valid_polyline(r, got["poly"], gc.goals(name)[r, gi], tol=0.0 if dt == "float64" else 1e-5)
                assert ok, (name, dt, r, low)
    print(f"\n[goals] most iterations {worst_it} of {pc.BUDGET['max_iterations']}, most nodes {worst_n} of {pc.BUDGET['max_nodes']}")
    assert worst_it <= pc.BUDGET["max_iterations"] // 4 and worst_n <= pc.BUDGET["max_nodes"] // 2


def test_no_valid_goal_and_n_goals():
    c = pc.case("post")
    for dt in DTYPES:
        for r in range(gc.B):
            got = gc.reference("all_bad", r, 0, dt)
            assert got["status"] == goal_ref.NO_VALID_GOAL and got["goal_index"] == -1 and len(got["poly"]) == 1
            assert got["goal_status"].tolist() == [plan_ref.GOAL_IN_COLLISION, plan_ref.GOAL_OUT_OF_LIMITS]
            assert np.array_equal(got["path"].astype(np.float32), np.repeat(c["start"][r][None], pc.BUDGET["W"], 0))
    cut = gc.reference("bad_first", 1, 0, "float64", 2)
    assert cut["status"] == goal_ref.NO_VALID_GOAL and cut["goal_status"].tolist() == [3, 1, -1]
    none = gc.reference("bad_first", 3, 0, "float64", 0)
    assert none["status"] == goal_ref.NO_VALID_GOAL and none["goal_status"].tolist() == [-1, -1, -1] and none["checked"] == 1
    over = gc.reference("bad_first", 0, 0, "float64", 11)
    assert over["status"] == plan_ref.OK and np.array_equal(over["poly"], gc.reference("bad_first", 0)["poly"]), "a count above G is clamped"
    # entries behind the count are never read: NaN there changes nothing
    g = gc.goals("bad_first")[2].copy()
    g[2:] = np.nan
    nan = goal_ref.plan_goals(pc.problem("post"), c["q"][2], g, 2, n_goals=2, W=pc.BUDGET["W"])
    assert nan["status"] == goal_ref.NO_VALID_GOAL and nan["goal_status"].tolist() == [3, 1, -1]
    # ... and a NaN inside the count is a goal outside the limits
    assert goal_ref.plan_goals(pc.problem("post"), c["q"][2], g, 2, W=pc.BUDGET["W"])["goal_status"].tolist() == [3, 1, 1]


class _StubScene:
    """what EntityView.plan_path_to_goals asks of a scene: records the call"""
    num_envs, device, nq = pc.B, torch.device("cpu"), 16

    def __init__(self):
        self.calls = []
        self.q = torch.zeros((pc.B, 16))

    def get_state(self):
        return (self.q, None, None, None)

    def plan_path(self, **kw):
        raise AssertionError("plan_path_to_goals goes through plan_path_goals")

    def plan_path_goals(self, **kw):
        self.calls.append(kw)
        R, G, D = kw["qpos_goals"].shape
        W = kw["num_waypoints"]
        i32 = torch.int32
        return {"path": torch.arange(R * W * D, dtype=torch.float32).reshape(R, W, D), "status": torch.tensor([0] * (R - 1) + [9], dtype=i32),
                "poly": torch.zeros((R, 128, D)), "n_poly": torch.ones(R, dtype=i32), "stats": torch.zeros((R, 4), dtype=i32),
                "goal_index": torch.tensor([G - 1] * (R - 1) + [-1], dtype=i32), "goal_status": torch.zeros((R, G), dtype=i32)}


def test_entity_view_argument_handling():
    from gym_genesis.tasks.views import EntityView

    c = pc.case("post")
    st = _StubScene()
    robot, cube = pc.arm(c["sb"], st), EntityView(st, c["sb"], "cube", ())
    goals = torch.as_tensor(gc.goals("bad_first")).permute(1, 0, 2)   # (G, R, n)
    path = robot.plan_path_to_goals(goals)
    kw = st.calls[-1]
    assert path.shape == (100, pc.B, 9) and torch.equal(path[:, 2], torch.arange(pc.B * 900, dtype=torch.float32).reshape(pc.B, 100, 9)[2])
    assert kw["qpos_goals"].shape == (pc.B, 3, 9) and torch.equal(kw["qpos_goals"][:, 1], goals[1]) and kw["n_goals"] is None
    assert kw["skip_geoms"] == robot._own_geoms() and kw["smooth_passes"] == 64 and kw["max_nodes"] == 256 and kw["max_iterations"] == 2000
    assert kw["qpos_start"] is None and kw["env_idx"] is None and list(kw["dof_qadr"]) == list(range(9)) and not kw["ignore_collision"]
    assert kw["resolution"] == 0.05 and kw["step"] == 0.3 and kw["margin"] == 0.0 and kw["seed"] == 0
    p, valid = robot.plan_path_to_goals(goals[:, :2], n_goals=[3, 1], qpos_start=torch.as_tensor(c["start"][:2]), envs_idx=[4, 0], smooth_path=False,
                                        num_waypoints=7, return_valid_mask=True, margin=0.6, ignore_entities=[cube], seed=9)
    kw = st.calls[-1]
    assert p.shape == (7, 2, 9) and valid.tolist() == [True, False] and kw["n_goals"].tolist() == [3, 1] and kw["n_goals"].dtype == torch.int32
    assert kw["smooth_passes"] == 0 and kw["env_idx"].tolist() == [4, 0] and kw["seed"] == 9 and kw["max_distance"] == 1.2
    assert kw["skip_geoms"] == robot._own_geoms() | cube._own_geoms() and kw["qpos_start"].shape == (2, 16)
    det = robot.plan_path_to_goals(goals, return_detail=True)
    assert sorted(det) == ["goal_index", "goal_status", "n_poly", "path", "poly", "stats", "status", "valid"]
    assert det["goal_index"].tolist() == [2, 2, 2, 2, -1] and det["goal_status"].shape == (pc.B, 3)
    with pytest.raises(NotImplementedError):
        robot.plan_path_to_goals(goals, planner="PRM")
    with pytest.raises(ValueError):
        robot.plan_path_to_goals(goals[:, :, :7])
    with pytest.raises(ValueError):
        robot.plan_path_to_goals(goals[0])   # (a batched task needs the goal axis)
    with pytest.raises(ValueError):
        robot.plan_path_to_goals(goals, ee_link_name="hand")   # (belongs to attached_entity)


# ---------------------------------------------------------------- the order of the direct edges
def test_direct_edge_order_tie_and_second_pick():
    c, pb = pc.case("post"), pc.problem("post")
    for r in range(gc.B):
        s = pb.set_row(c["q"][r])
        far, beyond = gc.goals("blocked_near")[r].astype(np.float64)
        seg, _ = plan_ref.polyline_clearance(pb, c["q"][r], [s, beyond], pc.RESOLUTION)
        d = lambda g: float(((g - s) ** 2).sum())   # noqa: E731
        assert seg.min() >= 0.02 and (beyond >= pb.lo).all() and (beyond <= pb.hi).all() and d(beyond) > 1.05 * d(far), (r, seg.min(), d(beyond), d(far))
    for dt in DTYPES:
        for r in range(gc.B):
            tie = gc.reference("twice", r, 0, dt)
            assert tie["status"] == plan_ref.OK and tie["goal_index"] == 0 and tie["iterations"] == 0, "equal distances: the lower g"
            second = gc.reference("blocked_near", r, 0, dt)
            assert second["status"] == plan_ref.OK and second["goal_index"] == 1 and second["iterations"] == 0 and len(second["poly"]) == 2
            assert second["goal_status"].tolist() == [0, 0], "the nearer goal is valid: only its edge is blocked"


# ---------------------------------------------------------------- pose goals
def test_pose_targets_are_what_they_say():
    c, pb = pc.case("post"), pc.problem("post")
    ch = goal_ref.cart_ref.Chain(pb, gc.hand(), c["spec"])
    for name, cfgs in (("pose_far", c["goal"]), ("pose_near", pc.case("clear")["goal"])):
        tp, tq = gc.pose(name)
        for r in range(gc.B):
            pb.set_row(c["q"][r])
            p, q = ch.pose(cfgs[r].astype(np.float64))
            assert np.abs(p - tp[r]).max() < 1e-6 and min(np.abs(q - tq[r]).max(), np.abs(q + tq[r]).max()) < 1e-6, "a solution exists by construction"
    assert np.linalg.norm(gc.pose("pose_away")[0][0]) > 2.0 and gc.pose("pose_post")[1] is None
    assert np.array_equal(gc.pose("pose_post")[0][0], np.array(pc.POST["pos"], np.float32))


@pytest.mark.parametrize("name", ["pose_far", "pose_near"])
def test_reachable_poses_the_condition_the_gpu_test_leans_on(name):
    """both precisions, max_samples 16: every row keeps >= 1 goal and plans within a quarter of max_iterations and half of max_nodes; the
    kept goals are solutions, inside the limits, clear and pairwise `dedup` apart"""
    c, pb = pc.case("post"), pc.problem("post")
    ch = goal_ref.cart_ref.Chain(pb, gc.hand(), c["spec"])
    tp, tq = gc.pose(name)
    for dt in DTYPES:
        for r in range(gc.B):
            got = gc.pose_reference(name, r, 0, dt)
            assert got["status"] == plan_ref.OK and got["n_goals"] >= 1, (name, dt, r, got["status"], got["goal_stats"])
            assert got["iterations"] <= pc.BUDGET["max_iterations"] // 4 and max(got["nodes"]) <= pc.BUDGET["max_nodes"] // 2
            tried, conv, rej, iters = got["goal_stats"]
            assert 1 <= tried <= 16 and got["n_goals"] <= conv - rej and iters > 0
            pb.set_row(c["q"][r])
            G = got["goals"].astype(np.float64)
            for k, g in enumerate(G):
                p, q = ch.pose(g)
                assert np.linalg.norm(p - tp[r]) < 5e-4 + 1e-5 and np.linalg.norm(goal_ref.cart_ref.rot_error(tq[r].astype(np.float64), q, np.float64)) < 5e-3 + 1e-4
                assert (g >= pb.lo).all() and (g <= pb.hi).all() and pb.clearance(g) >= pc.MARGIN - 1e-5
                assert np.array_equal(g[7:], c["start"][r][7:].astype(np.float64)), "the fingers keep their start value"
                assert all(np.abs(g - h).max() >= pc.RESOLUTION - 1e-6 for h in G[:k])
            gi = got["goal_index"]
            assert gc.valid_polyline(r, got["poly"], G[gi].astype(np.float32), tol=0.0 if dt == "float64" else 1e-5)[0]
    assert gc.pose_reference(name, 0, 0, "float64", True)["status"] == plan_ref.OK, "position only"


def test_failing_poses_and_their_stats():
    for dt in DTYPES:
        for r in range(gc.B):
            away, post = gc.pose_reference("pose_away", r, 0, dt), gc.pose_reference("pose_post", r, 0, dt)
            assert away["status"] == goal_ref.NO_VALID_GOAL and away["goal_stats"][:3] == [16, 0, 0], "unreachable: nothing converged"
            assert post["status"] == goal_ref.NO_VALID_GOAL and post["goal_stats"][0] == 16 and post["goal_stats"][1] > 0
            assert post["goal_stats"][2] == post["goal_stats"][1], "every converged sample is rejected"
            assert away["n_goals"] == post["n_goals"] == 0 and away["goal_index"] == -1 and len(post["poly"]) == 1
    c = pc.case("post")
    tp, tq = gc.pose("pose_near")
    bad = tp[0].copy()
    bad[1] = np.nan
    kw = dict(W=pc.BUDGET["W"])
    assert goal_ref.plan_pose(pc.problem("post"), c["spec"], gc.hand(), c["q"][0], bad, tq[0], 0, **kw)["status"] == goal_ref.NOT_FINITE
    assert goal_ref.plan_pose(pc.problem("post"), c["spec"], gc.hand(), c["q"][0], tp[0], np.zeros(4, np.float32), 0, **kw)["status"] == goal_ref.NOT_FINITE


# ---------------------------------------------------------------- MirScene's own checks, through the scene double
def test_scene_wrapper_refusals_on_the_double():
    """MirScene.plan_path_goals / plan_path_pose refuse a wrong shape before anything reaches the library: on tests/fake_scene.py's double,
    which has no library behind it"""
    import fake_scene
    from gym_genesis.backend.lib import MirScene

    c = pc.case("post")

    class Scene(fake_scene.OracleScene):
        plan_path_goals, plan_path_pose = MirScene.plan_path_goals, MirScene.plan_path_pose
        _plan_front, _sphere_probes, _sphere_qrows, _row_alloc, _self_query = (MirScene._plan_front, MirScene._sphere_probes, MirScene._sphere_qrows,
                                                                              MirScene._row_alloc, MirScene._self_query)

    s = Scene(c["spec"], gc.B)
    args = (c["probes"], c["links"], c["qadr"])
    good = gc.goals("bad_first")
    for goals, n_goals in ((good[:, 0], None), (good[:3], None), (good[:, :, :7], None), (good[None], None), (good, [3, 3]), (good, np.ones((gc.B, 1)))):
        with pytest.raises(ValueError):
            s.plan_path_goals(*args, goals, n_goals, skip_geoms=c["skip"])
    tp, tq = gc.pose("pose_near")
    for pos, quat in ((tp[:3], tq), (tp[:, :2], tq), (tp, tq[:, :3]), (tp, tq[:2])):
        with pytest.raises(ValueError):
            s.plan_path_pose(*args, gc.hand(), pos, quat, skip_geoms=c["skip"])
