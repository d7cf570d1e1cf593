"""Goal-set planning on the GPU (include/mirigid.h: mir_plan_path_goals; tasks/views.py: plan_path_to_goals).

The goal sets are those of tests/goal_cases.py on the "post" scene and start rows of tests/plan_cases.py; tests/test_goal_cpu.py holds
the condition that makes "every row finds a plan" fair (the float64 reference and its float32 port finish every row of "two_detours" and
"bad_first" within a quarter of the iterations and half of the nodes).  States are SET.  B = 5, max_nodes 128, max_iterations 512, W = 16.

The GPU's plans are judged on their own, never against the reference's plan, with the float64 validator and the yardstick of
tests/test_gpu_plan.py: tol = 4 x max(error of the float32 port against float64 on the same samples, 2^-23 x L), tol_q the same for the
resampler; both are printed before they are used.  With ONE goal the call must be mir_plan_path / _self / _carry byte for byte: that test
keeps the tree loop of csrc/mir_plan_tree.h (the goal kernel's) and the one mir_plan.hip still holds for itself from drifting apart.

Pose goals (mir_plan_path_pose, plan_path_to_pose): the targets of tests/goal_cases.py; a kept goal's float64 hand pose must be within
pos_tol / rot_tol plus the yardstick of the forward kinematics (4 x max(float32 port against float64 at that configuration, 2^-23 L)).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import carry_cases as cc
import goal_cases as gc
import plan_cases as pc
import plan_ref
import self_cases as sc
from gym_genesis.backend import spec as S
from gym_genesis.backend.spec import make_carry_query, make_goal_query, make_plan_query

pytestmark = pytest.mark.gpu

B, W = pc.B, pc.BUDGET["W"]
_scenes = {}
KEYS = ("path", "poly", "n_poly", "stats", "status")


def _scene(name, c=None):
    if name not in _scenes:
        from gym_genesis.backend.lib import MirScene

        c = pc.case("post") if c is None else c
        s = MirScene(c["spec"], B)
        s.set_state(qpos=c["q"], qvel=np.zeros((B, s.nv), np.float32))
        _scenes[name] = s
    return _scenes[name]


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _budget(c, **kw):
    args = dict(num_waypoints=W, max_nodes=pc.BUDGET["max_nodes"], max_iterations=pc.BUDGET["max_iterations"], resolution=pc.RESOLUTION, step=pc.STEP,
                margin=pc.MARGIN, skip_geoms=c["skip"])
    args.update(kw)
    return args


def _goals(name, n_goals=None, goals=None, **kw):
    c, s = pc.case("post"), _scene("post")
    return _np(s.plan_path_goals(c["probes"], c["links"], c["qadr"], gc.goals(name) if goals is None else goals, n_goals, **_budget(c, **kw)))


# ---------------------------------------------------------------- one goal: the bytes of mir_plan_path
@pytest.mark.parametrize("form", ["post", "clear", "post, ignore_collision", "self", "carry"])
def test_one_goal_is_plan_path_byte_for_byte(form):
    kw = {}
    if form == "self":
        c = sc.case("fold")
        s = _scene("self:fold", c)
        kw = dict(self_model=dict(link_mask=c["mask"], n_extra=c["n_extra"]))
    elif form == "carry":
        c = cc.case("under")
        s = _scene("carry:under", c)
        kw = dict(self_model=dict(link_mask=c["mask"], n_extra=c["n_extra"]), carry=dict(body=c["body"], link=c["link"], grasp=None))
    else:
        c, s = pc.case("clear" if form == "clear" else "post"), _scene("post")
        kw = dict(ignore_collision=form.endswith("ignore_collision"))
    one = _np(s.plan_path(c["probes"], c["links"], c["qadr"], c["goal"], **_budget(c), **kw))
    got = _np(s.plan_path_goals(c["probes"], c["links"], c["qadr"], c["goal"][:, None], **_budget(c), **kw))
    print(f"\n[goals, one goal, {form}] status {one['status'].tolist()} n_poly {one['n_poly'].tolist()} iterations {one['stats'][:, 0].tolist()}")
    assert (one["status"] == 0).all(), "every row of the case plans"
    for k in KEYS + (("grasp",) if form == "carry" else ()):
        assert got[k].tobytes() == one[k].tobytes(), (form, k)
    assert (got["goal_index"] == 0).all() and (got["goal_status"] == 0).all() and got["goal_status"].shape == (B, 1)
    if form == "post":
        assert (one["n_poly"] >= 3).all() and (one["stats"][:, 0] > 0).all(), "both tree loops ran"


def test_one_rejected_goal_has_the_status_plan_path_gives():
    c, s = pc.case("post"), _scene("post")
    bad = gc.goals("bad_first")
    goal = c["goal"].copy()
    goal[0], goal[1] = bad[0, 0], bad[1, 1]   # row 0: inside the post; row 1: outside the limits
    one = _np(s.plan_path(c["probes"], c["links"], c["qadr"], goal, **_budget(c)))
    got = _np(s.plan_path_goals(c["probes"], c["links"], c["qadr"], goal[:, None], **_budget(c)))
    assert one["status"].tolist()[:2] == [S.PLAN_GOAL_IN_COLLISION, S.PLAN_GOAL_OUT_OF_LIMITS] and (one["status"][2:] == 0).all()
    assert got["goal_status"][:, 0].tolist() == one["status"].tolist()
    assert got["status"].tolist() == [S.PLAN_NO_VALID_GOAL] * 2 + [0] * 3 and got["goal_index"].tolist() == [-1, -1, 0, 0, 0]
    for k in ("path", "poly", "n_poly"):   # (a failed row holds its start, whatever refused it)
        assert got[k].tobytes() == one[k].tobytes(), k
    assert got["stats"][2:].tobytes() == one["stats"][2:].tobytes()


# ---------------------------------------------------------------- the direct edge to the nearer goal
@pytest.mark.parametrize("name", ["near_far", "far_near"])
def test_near_far_takes_the_clear_edge(name):
    c = pc.case("post")
    near = 1 if name == "near_far" else 0
    got = _goals(name)
    target = gc.goals(name)[:, near]
    assert (got["status"] == 0).all() and (got["stats"][:, 0] == 0).all() and (got["n_poly"] == 2).all(), (got["status"], got["stats"], got["n_poly"])
    assert (got["goal_index"] == near).all() and (got["goal_status"] == 0).all()
    assert np.array_equal(got["path"][:, 0], c["start"]) and np.array_equal(got["path"][:, -1], target), "the ends are the start's and the goal's bits"
    assert np.array_equal(got["poly"][:, 0], c["start"]) and np.array_equal(got["poly"][:, 1], target) and (got["poly"][:, 2:] == 0).all()
    allowed = 2.0 ** -22 * float(max(np.abs(c["start"]).max(), np.abs(target).max()))
    line = lambda a, b: np.stack([a + (w / (W - 1)) * (b - a) for w in range(W)])   # noqa: E731
    err = max(float(np.abs(got["path"][r] - line(c["start"][r].astype(np.float64), target[r].astype(np.float64))).max()) for r in range(B))
    print(f"\n[goals, {name}] straight line: waypoints against the float64 interpolation {err:.3e} allowed {allowed:.3e}")
    assert err <= allowed


# ---------------------------------------------------------------- the forest
def _tol(row, samples):
    """4 x max(float32 port against float64 on these configurations, 2^-23 L): the yardstick of tests/test_gpu_plan.py"""
    c = pc.case("post")
    p64, p32 = pc.problem("post"), pc.problem("post", np.float32)
    p64.set_row(c["q"][row])
    p32.set_row(c["q"][row])
    err, L = 0.0, 0.0
    for q in samples:
        c64, c32 = p64.clearance(q), p32.clearance(np.asarray(q, np.float32))
        err = max(err, abs(float(c32) - float(c64)))
        L = max(L, float(np.abs(p64.centres(q)).max()), abs(float(c64)))
    return 4.0 * max(err, 2.0 ** -23 * L), err, L


def _check_plans(name, got, label):
    c = pc.case("post")
    lim = pc.problem("post", np.float32)
    assert (got["status"] == 0).all(), (label, got["status"], got["stats"], got["goal_status"])
    for r in range(B):
        n, gi = int(got["n_poly"][r]), int(got["goal_index"][r])
        assert 0 <= gi < gc.goals(name).shape[1] and got["goal_status"][r, gi] == 0
        goal = gc.goals(name)[r, gi]
        poly = got["poly"][r, :n].astype(np.float64)
        ok, low, samples = gc.valid_polyline(r, poly, goal, tol=np.inf)
        tol, err, L = _tol(r, samples)
        ref64, ref32 = plan_ref.resample(poly, W, np.float64), plan_ref.resample(poly, W, np.float32)
        Q = float(np.abs(poly).max())
        port_q = float(np.abs(ref32.astype(np.float64) - ref64).max())
        tol_q = 4.0 * max(port_q, 2.0 ** -23 * Q)
        err_q = float(np.abs(got["path"][r] - ref64).max())
        ref = gc.reference(name, r)
        print(f"[goals, {label}] row {r}: goal {gi} (reference {ref['goal_index']}) n_poly {n} lowest clearance {low:.5f} (tol {tol:.3e}: port {err:.3e}, "
              f"L {L:.3f}); waypoints {err_q:.3e} (tol_q {tol_q:.3e}); iterations / nodes GPU {got['stats'][r, :3].tolist()} reference "
              f"{[ref['iterations'], *ref['nodes']]}")
        assert ok, "the polyline starts at the row's start and ends at the bits of goal goal_index"
        assert np.array_equal(got["path"][r, 0], c["start"][r]) and np.array_equal(got["path"][r, -1], goal)
        assert low >= pc.MARGIN - tol, (label, r, low, tol)
        assert err_q <= tol_q, (label, r, err_q, tol_q)
        assert (got["path"][r] >= lim.lo).all() and (got["path"][r] <= lim.hi).all() and (got["poly"][r, n:] == 0).all()


def test_two_detours_end_at_one_of_the_goals():
    got = _goals("two_detours")
    print()
    _check_plans("two_detours", got, "two_detours")
    assert (got["n_poly"] >= 3).all() and (got["stats"][:, 0] > 0).all() and (got["goal_status"] == 0).all()
    assert (got["stats"][:, 2] >= 2).all(), "Tb holds both roots"


def test_bad_first_and_all_bad():
    c = pc.case("post")
    got = _goals("bad_first")
    print()
    _check_plans("bad_first", got, "bad_first")
    assert (got["goal_status"] == np.array([S.PLAN_GOAL_IN_COLLISION, S.PLAN_GOAL_OUT_OF_LIMITS, S.PLAN_OK])).all() and (got["goal_index"] == 2).all()
    bad = _goals("all_bad")
    assert (bad["status"] == S.PLAN_NO_VALID_GOAL).all() and (bad["goal_index"] == -1).all() and (bad["n_poly"] == 1).all()
    assert np.array_equal(bad["path"], np.repeat(c["start"][:, None], W, 1)) and np.array_equal(bad["poly"][:, 0], c["start"]) and (bad["poly"][:, 1:] == 0).all()
    assert (bad["goal_status"] == np.array([S.PLAN_GOAL_IN_COLLISION, S.PLAN_GOAL_OUT_OF_LIMITS])).all() and (bad["stats"][:, 0] == 0).all()
    # n_goals = [3, 2, 3, 0, 3] with NaN behind each row's count
    counts = np.array([3, 2, 3, 0, 3], np.int32)
    g = gc.goals("bad_first").copy()
    for r in range(B):
        g[r, counts[r]:] = np.nan
    cut = _goals("bad_first", n_goals=counts, goals=g)
    for r in (0, 2, 4):
        assert all(cut[k][r].tobytes() == got[k][r].tobytes() for k in got), r
    assert all(cut[k][1].tobytes() == bad[k][1].tobytes() for k in KEYS) and cut["goal_status"][1].tolist() == [3, 1, -1] and cut["goal_index"][1] == -1
    assert cut["status"][3] == S.PLAN_NO_VALID_GOAL and cut["goal_status"][3].tolist() == [-1, -1, -1] and cut["goal_index"][3] == -1
    assert np.array_equal(cut["path"][3], np.repeat(c["start"][3][None], W, 0)) and cut["n_poly"][3] == 1
    # a count outside 0 .. G is clamped
    wide = _goals("bad_first", n_goals=np.array([9, 3, 100, 3, 2 ** 31 - 1], np.int32))
    assert all(wide[k].tobytes() == got[k].tobytes() for k in got)
    none = _goals("bad_first", n_goals=np.array([-1, -2 ** 31, 0, -5, 0], np.int32))
    assert (none["status"] == S.PLAN_NO_VALID_GOAL).all() and (none["goal_status"] == -1).all()


def test_a_start_in_collision_is_reported_before_the_goals():
    c, s = pc.case("post"), _scene("post")
    q = c["q"].copy()
    q[0, c["qadr"]] = gc.goals("bad_first")[0, 0]   # row 0 starts inside the post
    got = _np(s.plan_path_goals(c["probes"], c["links"], c["qadr"], gc.goals("two_detours"), qpos_start=torch.as_tensor(q, device=s.device), **_budget(c)))
    clean = _goals("two_detours")
    assert got["status"][0] == S.PLAN_START_IN_COLLISION and got["goal_index"][0] == -1 and got["goal_status"][0].tolist() == [-1, -1]
    assert np.array_equal(got["path"][0], np.repeat(q[0, c["qadr"]][None], W, 0))
    assert all(got[k][1:].tobytes() == clean[k][1:].tobytes() for k in got)


# ---------------------------------------------------------------- determinism and independence
def test_determinism_rows_and_seed():
    c, s = pc.case("post"), _scene("post")
    got, again = _goals("two_detours"), _goals("two_detours")
    assert all(got[k].tobytes() == again[k].tobytes() for k in got)
    for r in range(B):
        sub = _np(s.plan_path_goals(c["probes"], c["links"], c["qadr"], gc.goals("two_detours")[[r]], env_idx=torch.tensor([r], device=s.device), **_budget(c)))
        assert all(sub[k][0].tobytes() == got[k][r].tobytes() for k in got), r
    other = _goals("two_detours", seed=1)
    assert (other["status"] == 0).all() and any(other["poly"][r].tobytes() != got["poly"][r].tobytes() for r in range(B))


# ---------------------------------------------------------------- refusals
def test_refusals_launch_nothing():
    c, s = pc.case("post"), _scene("post")
    N, D = len(c["links"]), len(c["qadr"])
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    dev = lambda a: torch.as_tensor(a, device=s.device)  # noqa: E731
    probes, goals = dev(c["probes"]), dev(gc.goals("bad_first"))
    path = torch.full((B, W, D), float("nan"), device=s.device)
    status = torch.full((B,), -7, dtype=torch.int32, device=s.device)
    gidx = torch.full((B,), -7, dtype=torch.int32, device=s.device)
    grasp = torch.zeros((B, 7), device=s.device)
    lk, qa = np.ascontiguousarray(c["links"], np.int32), np.ascontiguousarray(c["qadr"], np.int32)
    ref = lambda x: None if x is None else C.byref(x)  # noqa: E731

    def raw(q, gq, goals=goals, cq=None, grasp_in=None, grasp_out=None):
        rc = s.lib.mir_plan_path_goals(s.h, C.byref(q), None, ref(cq), ref(gq), p(probes), lk.ctypes.data_as(C.c_void_p), qa.ctypes.data_as(C.c_void_p), None, 0,
                                       None, p(grasp_in), p(goals), None, p(path), p(status), None, None, None, p(grasp_out), p(gidx), None, s._stream())
        torch.cuda.synchronize()
        return rc, s.lib.mir_last_error()

    q = make_plan_query(N, D, W, 128, 512, skip_geoms=c["skip"])
    launches = s.__dict__.get("plan_launches", 0)
    for G_ in (0, -1, 9):
        rc, msg = raw(q, make_goal_query(G_))
        assert rc == -1 and b"mir_plan_path_goals" in msg and b"max_goals outside 1 .. 8" in msg, (G_, rc, msg)
    gq = make_goal_query(3)
    assert raw(q, None)[0] == -1 and raw(q, gq, goals=None)[0] == -1
    bad = make_goal_query(3); bad.struct_size += 4
    assert raw(q, bad)[0] == -1
    bad = make_goal_query(3); bad.flags = 2
    assert raw(q, bad)[0] == -1
    for nodes in (2, 3):
        rc, msg = raw(make_plan_query(N, D, W, nodes, 512, skip_geoms=c["skip"]), gq)
        assert rc == -1 and b"max_nodes <= max_goals" in msg, (nodes, rc, msg)
    rc, msg = raw(q, gq, grasp_in=grasp)
    assert rc == -1 and b"grasp without a MirCarryQuery" in msg
    rc, msg = raw(q, gq, grasp_out=grasp)
    assert rc == -1 and b"grasp_used without a MirCarryQuery" in msg
    # what mir_plan_path refuses stays refused; a carry query is checked as in mir_plan_path_carry
    assert raw(make_plan_query(N, D, W, 128, 512, resolution=0.0, skip_geoms=c["skip"]), gq)[0] == -1
    assert raw(make_plan_query(N, D, 1, 128, 512, skip_geoms=c["skip"]), gq)[0] == -1
    assert raw(q, gq, cq=make_carry_query(1, 2))[0] == -1   # (body 1 is no free-joint body)
    assert torch.isnan(path).all() and (status == -7).all() and (gidx == -7).all(), "a refused call launches nothing"
    assert raw(make_plan_query(N, D, W, 4, 512, skip_geoms=c["skip"]), gq)[0] == 0 and torch.isfinite(path).all() and (gidx >= -1).all()
    assert s.__dict__.get("plan_launches", 0) == launches
    assert C.sizeof(S.MirGoalQuery) == s.lib.mir_goal_query_sizeof()
    with pytest.raises(ValueError):
        s.plan_path_goals(c["probes"], c["links"], c["qadr"], c["goal"], **_budget(c))   # (R, D): the goal axis is missing


# ---------------------------------------------------------------- the entity's calls
def test_entity_view_is_the_same_launch():
    c, s = pc.case("post"), _scene("post")
    robot = pc.arm(c["sb"], s)
    cube = type(robot)(s, c["sb"], "cube", ())
    kw = dict(num_waypoints=W, max_nodes=pc.BUDGET["max_nodes"], max_iterations=pc.BUDGET["max_iterations"], resolution=pc.RESOLUTION, step=pc.STEP,
              margin=pc.MARGIN)
    raw = _goals("two_detours")
    goals = torch.as_tensor(gc.goals("two_detours"), device=s.device).permute(1, 0, 2)   # (G, R, n)
    det = _np(robot.plan_path_to_goals(goals, return_detail=True, **kw))
    assert det["path"].shape == (W, B, 9) and det["valid"].all() and np.array_equal(det["path"], raw["path"].transpose(1, 0, 2))
    assert all(det[k].tobytes() == raw[k].tobytes() for k in ("poly", "n_poly", "stats", "status", "goal_index", "goal_status"))
    path, valid = robot.plan_path_to_goals(goals, return_valid_mask=True, **kw)
    assert torch.equal(path.cpu(), torch.as_tensor(det["path"])) and valid.all()
    sub = robot.plan_path_to_goals(goals[:, [3, 0]], n_goals=[2, 1], envs_idx=[3, 0], return_detail=True, **kw)
    assert sub["path"].shape == (W, 2, 9) and np.array_equal(sub["path"][:, 0].cpu().numpy(), det["path"][:, 3])
    assert sub["goal_index"].tolist() == [int(det["goal_index"][3]), 0] and sub["goal_status"].tolist() == [[0, 0], [0, -1]]
    # the results go on into the companions of plan_path unchanged
    clear = robot.get_path_clearance(path)
    assert clear.shape == (B,) and (clear >= pc.MARGIN - 1e-4).all()
    timed = robot.retime_path(path, max_velocity=1.0, max_acceleration=2.0, return_detail=True)
    assert timed["valid"].all(), timed["status"]
    # the straight edge through an entity that is ignored is not through the post: still a detour, goals judged alike
    ign = robot.plan_path_to_goals(goals, ignore_entities=[cube], return_detail=True, **kw)
    assert ign["valid"].all()


# ---------------------------------------------------------------- the order of the direct edges
def test_direct_edge_order_tie_and_second_pick():
    tie = _goals("twice")
    assert (tie["status"] == 0).all() and (tie["goal_index"] == 0).all() and (tie["stats"][:, 0] == 0).all(), "equal distances: the lower g wins"
    got = _goals("blocked_near")
    beyond = gc.goals("blocked_near")[:, 1]
    assert (got["status"] == 0).all() and (got["goal_status"] == 0).all() and (got["goal_index"] == 1).all(), (got["status"], got["goal_index"])
    assert (got["stats"][:, 0] == 0).all() and (got["n_poly"] == 2).all() and np.array_equal(got["path"][:, -1], beyond)
    near_alone = _goals("blocked_near", n_goals=np.ones(B, np.int32))
    assert (near_alone["stats"][:, 0] > 0).all(), "the nearer goal's edge is blocked: alone it needs the trees"
    assert (got["stats"][:, 3] > 3).all(), "the blocked edge to the nearer goal was tried first"


# ---------------------------------------------------------------- pose goals
IK = dict(pos_tol=5e-4, rot_tol=5e-3)


def _pose(name, quat=True, pos=None, **kw):
    c, s = pc.case("post"), _scene("post")
    tp, tq = gc.pose(name)
    return _np(s.plan_path_pose(c["probes"], c["links"], c["qadr"], gc.hand(), tp if pos is None else pos, tq if quat else None, max_goals=4, max_samples=16,
                                **_budget(c, **kw)))


def _fk_tol(ch64, ch32, g):
    p64, q64 = ch64.pose(g)
    p32, q32 = ch32.pose(g.astype(np.float32))
    err = max(float(np.abs(p32 - p64).max()), float(min(np.abs(q32 - q64).max(), np.abs(q32 + q64).max())))
    return 4.0 * max(err, 2.0 ** -23 * max(float(np.abs(p64).max()), 1.0)), p64, q64


def _check_pose(name, got, label, quat=True):
    c = pc.case("post")
    tp, tq = gc.pose(name)
    pb64, pb32 = pc.problem("post"), pc.problem("post", np.float32)
    ch64, ch32 = gc.goal_ref.cart_ref.Chain(pb64, gc.hand(), c["spec"]), gc.goal_ref.cart_ref.Chain(pb32, gc.hand(), c["spec"])
    assert (got["status"] == 0).all(), (label, got["status"], got["goal_stats"])
    print()
    for r in range(B):
        pb64.set_row(c["q"][r])
        pb32.set_row(c["q"][r])
        n, gi, npoly = int(got["n_goals"][r]), int(got["goal_index"][r]), int(got["n_poly"][r])
        assert 1 <= n <= 4 and 0 <= gi < n and (got["goals"][r, n:] == 0).all()
        assert got["goal_status"][r].tolist() == [0] * n + [-1] * (4 - n)
        G = got["goals"][r, :n].astype(np.float64)
        worst_p = worst_r = 0.0
        for k, g in enumerate(G):
            tol_fk, p, q = _fk_tol(ch64, ch32, g)
            ep = float(np.linalg.norm(p - tp[r]))
            er = float(np.linalg.norm(gc.goal_ref.cart_ref.rot_error(tq[r].astype(np.float64), q, np.float64))) if quat else 0.0
            worst_p, worst_r = max(worst_p, ep), max(worst_r, er)
            assert ep <= IK["pos_tol"] + tol_fk and er <= IK["rot_tol"] + tol_fk, (label, r, k, ep, er, tol_fk)
            assert (g >= pb64.lo).all() and (g <= pb64.hi).all() and np.array_equal(got["goals"][r, k, 7:], c["start"][r, 7:])
            assert all(np.abs(got["goals"][r, k] - got["goals"][r, h]).max() >= np.float32(pc.RESOLUTION) for h in range(k)), "pairwise >= dedup apart"
            tol_c = _tol(r, [g])[0]
            assert pb64.clearance(g) >= pc.MARGIN - tol_c, (label, r, k, pb64.clearance(g), tol_c)
        goal = got["goals"][r, gi]
        poly = got["poly"][r, :npoly].astype(np.float64)
        ok, low, samples = gc.valid_polyline(r, poly, goal, tol=np.inf)
        tol = _tol(r, samples)[0]
        ref64, ref32 = plan_ref.resample(poly, W, np.float64), plan_ref.resample(poly, W, np.float32)
        tol_q = 4.0 * max(float(np.abs(ref32.astype(np.float64) - ref64).max()), 2.0 ** -23 * float(np.abs(poly).max()))
        err_q = float(np.abs(got["path"][r] - ref64).max())
        ref = gc.pose_reference(name, r, 0, "float64", not quat)
        print(f"[pose, {label}] row {r}: kept {n} (reference {ref['n_goals']}) goal {gi} stats {got['goal_stats'][r].tolist()} (reference {ref['goal_stats']}) "
              f"pose error {worst_p:.2e} m {worst_r:.2e} rad; n_poly {npoly} lowest clearance {low:.5f} (tol {tol:.3e}); waypoints {err_q:.3e} (tol_q {tol_q:.3e}); "
              f"iterations / nodes {got['stats'][r, :3].tolist()}")
        assert ok and np.array_equal(got["path"][r, -1], goal), "the last waypoint is goals[goal_index] bit for bit"
        assert low >= pc.MARGIN - tol and err_q <= tol_q, (label, r, low, tol, err_q, tol_q)
        st = got["goal_stats"][r]
        assert 1 <= st[0] <= 16 and n <= st[1] - st[2] and st[3] > 0


@pytest.mark.parametrize("name", ["pose_far", "pose_near"])
def test_pose_reachable(name):
    _check_pose(name, _pose(name), name)


def test_pose_position_only():
    _check_pose("pose_far", _pose("pose_far", quat=False), "pose_far, quat=None", quat=False)


def test_pose_failing():
    c = pc.case("post")
    away = _pose("pose_away")
    assert (away["status"] == S.PLAN_NO_VALID_GOAL).all() and (away["goal_stats"][:, 0] == 16).all() and (away["goal_stats"][:, 1] == 0).all()
    post = _pose("pose_post", quat=False)
    print(f"\n[pose, post centre] goal_stats {post['goal_stats'].tolist()}")
    assert (post["status"] == S.PLAN_NO_VALID_GOAL).all() and (post["goal_stats"][:, 1] > 0).all()
    assert (post["goal_stats"][:, 2] == post["goal_stats"][:, 1]).all(), "every converged sample is rejected"
    for got in (away, post):
        assert (got["n_goals"] == 0).all() and (got["goal_index"] == -1).all() and (got["goal_status"] == -1).all() and (got["goals"] == 0).all()
        assert np.array_equal(got["path"], np.repeat(c["start"][:, None], W, 1)) and (got["n_poly"] == 1).all()
    clean = _pose("pose_near")
    tp = gc.pose("pose_near")[0].copy()
    tp[2, 1] = np.nan
    got = _pose("pose_near", pos=tp)
    assert got["status"][2] == S.CART_NOT_FINITE and got["n_goals"][2] == 0 and got["goal_index"][2] == -1 and (got["goal_stats"][2] == 0).all()
    assert np.array_equal(got["path"][2], np.repeat(c["start"][2][None], W, 0))
    keep = [0, 1, 3, 4]
    assert all(got[k][keep].tobytes() == clean[k][keep].tobytes() for k in got), "the other rows keep the bytes of the clean call"


def test_pose_determinism_rows_and_seed():
    c, s = pc.case("post"), _scene("post")
    got, again = _pose("pose_far"), _pose("pose_far")
    assert all(got[k].tobytes() == again[k].tobytes() for k in got)
    tp, tq = gc.pose("pose_far")
    for r in range(B):
        sub = _np(s.plan_path_pose(c["probes"], c["links"], c["qadr"], gc.hand(), tp[[r]], tq[[r]], max_goals=4, max_samples=16,
                                   env_idx=torch.tensor([r], device=s.device), **_budget(c)))
        assert all(sub[k][0].tobytes() == got[k][r].tobytes() for k in got), r
    other = _pose("pose_far", seed=1)
    assert (other["status"] == 0).all() and any(other["goals"][r].tobytes() != got["goals"][r].tobytes() for r in range(B))
    one = _np(s.plan_path_pose(c["probes"], c["links"], c["qadr"], gc.hand(), tp, tq, max_goals=1, max_samples=1, **_budget(c)))
    assert (one["goal_stats"][:, 0] == 1).all() and (one["n_goals"] <= 1).all() and one["goals"].shape == (B, 1, 9)


def test_pose_refusals_launch_nothing():
    c, s = pc.case("post"), _scene("post")
    tp, tq = gc.pose("pose_near")
    launches = s.__dict__.get("plan_launches", 0)
    from gym_genesis.backend.lib import MirError

    for kw in (dict(max_goals=0), dict(max_goals=9), dict(max_samples=0), dict(dedup=-1.0), dict(max_goals=4, max_nodes=4), dict(link_body=-1),
               dict(link_body=c["sb"].body_index("cube"))):
        args = dict(link_body=gc.hand(), max_goals=4, max_samples=16)
        args.update(kw)
        with pytest.raises(MirError, match="mir_plan_path_pose"):
            s.plan_path_pose(c["probes"], c["links"], c["qadr"], target_pos=tp, target_quat=tq, **_budget(c, **args))
    assert s.__dict__.get("plan_launches", 0) == launches
    assert C.sizeof(S.MirPoseGoalQuery) == s.lib.mir_pose_goal_query_sizeof()


def test_entity_view_pose_is_the_same_launch():
    c, s = pc.case("post"), _scene("post")
    robot = pc.arm(c["sb"], s)
    kw = dict(num_waypoints=W, max_nodes=pc.BUDGET["max_nodes"], max_iterations=pc.BUDGET["max_iterations"], resolution=pc.RESOLUTION, step=pc.STEP,
              margin=pc.MARGIN)
    raw = _pose("pose_far")
    tp, tq = (torch.as_tensor(x, device=s.device) for x in gc.pose("pose_far"))
    det = _np(robot.plan_path_to_pose(robot.get_link("hand"), tp, tq, return_detail=True, **kw))
    assert det["path"].shape == (W, B, 9) and det["valid"].all() and np.array_equal(det["path"], raw["path"].transpose(1, 0, 2))
    assert all(det[k].tobytes() == raw[k].tobytes() for k in ("poly", "n_poly", "stats", "status", "goal_index", "goal_status", "goals", "n_goals", "goal_stats"))
    path, valid = robot.plan_path_to_pose(robot.get_link("hand"), tp, tq, return_valid_mask=True, **kw)
    assert torch.equal(path.cpu(), torch.as_tensor(det["path"])) and valid.all()
    clear = robot.get_path_clearance(path)
    assert clear.shape == (B,) and (clear >= pc.MARGIN - 1e-4).all()
    assert robot.retime_path(path, max_velocity=1.0, max_acceleration=2.0, return_detail=True)["valid"].all()
