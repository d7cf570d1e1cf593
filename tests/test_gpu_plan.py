"""Batched motion planning on the GPU (include/mirigid.h: mir_plan_path, mir_path_clearance; tasks/views.py: plan_path /
get_path_clearance / path_in_collision).

The cases -- scenes, start rows, goals, sphere model, budgets -- are those of tests/plan_cases.py; tests/test_plan_cpu.py holds the
condition that makes "every row finds a plan" fair (the float64 reference and its float32 port finish every "post" row within a quarter
of the iterations and half of the nodes).  States are SET.  B = 5.

The GPU's plans are judged on their own, never against the reference's plan: a float32 planner may take another branch at a sample that
lies within rounding of an obstacle.  Every polyline edge is sampled by the edge rule in float64 and must keep its clearance; the
waypoints are compared with the float64 resampler applied to the GPU's own polyline.

Yardstick (the rule of tests/test_gpu_distance.py): tol = 4 x max(error of the float32 port against float64 on the same samples,
2^-23 x L), L = the largest absolute world coordinate of a probe centre or clearance on those samples; tol_q the same for the resampler
with Q = max |q| in place of L.  Both are printed before they are used.

Failures (test_failures): one MirPlanQuery serves one call, so the rows that fail by their budget (max_iterations = 32 on "sealed",
max_nodes = 4 on "post") are calls of their own; the rows that fail by their configuration and an ordinary row share one call.
"sealed" shows ITERATION_LIMIT at that budget; that no budget would do is argued in tests/plan_cases.py, not proven here.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import plan_cases as pc
import plan_ref
from gym_genesis.backend import spec as S
from gym_genesis.backend.spec import MirPlanQuery, make_plan_query

pytestmark = pytest.mark.gpu

B, W = pc.B, pc.BUDGET["W"]
_scenes = {}


def _scene(name):
    if name not in _scenes:
        from gym_genesis.backend.lib import MirScene

        c = pc.case(name)
        sc = MirScene(c["spec"], B)
        sc.set_state(qpos=c["q"], qvel=np.zeros((B, sc.nv), np.float32))
        _scenes[name] = sc
    return _scenes[name]


def _plan(name, goal=None, **kw):
    c, sc = pc.case(name), _scene(name)
    args = dict(num_waypoints=W, max_nodes=pc.BUDGET["max_nodes"], max_iterations=pc.BUDGET["max_iterations"], resolution=pc.RESOLUTION,
                step=pc.STEP, margin=pc.MARGIN, skip_geoms=c["skip"])
    args.update(kw)
    out = sc.plan_path(c["probes"], c["links"], c["qadr"], c["goal"] if goal is None else goal, **args)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _straight(a, b, n):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.stack([a + (w / (n - 1)) * (b - a) for w in range(n)])


def _check_straight(name, got):
    c = pc.case(name)
    assert (got["status"] == 0).all() and (got["stats"][:, 0] == 0).all() and (got["n_poly"] == 2).all(), (got["status"], got["stats"], got["n_poly"])
    assert np.array_equal(got["path"][:, 0], c["start"]) and np.array_equal(got["path"][:, -1], c["goal"]), "the ends are the start's and the goal's bits"
    assert np.array_equal(got["poly"][:, 0], c["start"]) and np.array_equal(got["poly"][:, 1], c["goal"]) and (got["poly"][:, 2:] == 0).all()
    allowed = 2.0 ** -22 * float(max(np.abs(c["start"]).max(), np.abs(c["goal"]).max()))
    err = max(float(np.abs(got["path"][r] - _straight(c["start"][r], c["goal"][r], W)).max()) for r in range(B))
    print(f"\n[plan, {name}] straight line: waypoints against the float64 interpolation {err:.3e} allowed {allowed:.3e}")
    assert err <= allowed


def _tol(name, row, samples):
    """4 x max(float32 port against float64 on these configurations, 2^-23 L)"""
    c = pc.case(name)
    p64, p32 = pc.problem(name), pc.problem(name, np.float32)
    p64.set_row(c["q"][row])
    p32.set_row(c["q"][row])
    err, L = 0.0, 0.0
    for q in samples:
        c64, c32 = p64.clearance(q), p32.clearance(np.asarray(q, np.float32))
        err = max(err, abs(float(c32) - float(c64)))
        L = max(L, float(np.abs(p64.centres(q)).max()), abs(float(c64)))
    return 4.0 * max(err, 2.0 ** -23 * L), err, L


def _check_plan(name, got, label, seed=0):
    """the check of a planned batch, every row -> the polylines"""
    c = pc.case(name)
    lim = pc.problem(name, np.float32)
    assert (got["status"] == 0).all(), (label, got["status"], got["stats"])
    polys = []
    for r in range(B):
        n = int(got["n_poly"][r])
        poly = got["poly"][r, :n].astype(np.float64)
        seg, samples = plan_ref.polyline_clearance(pc.problem(name), c["q"][r], poly, pc.RESOLUTION)
        tol, err, L = _tol(name, r, samples)
        ref64, ref32 = plan_ref.resample(poly, W, np.float64), plan_ref.resample(poly, W, np.float32)
        Q = float(np.abs(poly).max())
        port_q = float(np.abs(ref32.astype(np.float64) - ref64).max())
        tol_q = 4.0 * max(port_q, 2.0 ** -23 * Q)
        err_q = float(np.abs(got["path"][r] - ref64).max())
        ref = pc.reference(name, r, seed)
        print(f"[plan, {label}] row {r}: n_poly {n} lowest clearance {seg.min():.5f} (tol {tol:.3e}: port {err:.3e}, L {L:.3f}); waypoints {err_q:.3e} "
              f"(tol_q {tol_q:.3e}: port {port_q:.3e}, Q {Q:.3f}); iterations / nodes GPU {got['stats'][r, :3].tolist()} reference "
              f"{[ref['iterations'], *ref['nodes']]}; checked {int(got['stats'][r, 3])}")
        assert np.array_equal(got["poly"][r, 0], c["start"][r]) and np.array_equal(got["poly"][r, n - 1], c["goal"][r])
        assert np.array_equal(got["path"][r, 0], c["start"][r]) and np.array_equal(got["path"][r, -1], c["goal"][r])
        assert seg.min() >= pc.MARGIN - tol, (label, r, seg.min(), tol)
        assert err_q <= tol_q, (label, r, err_q, tol_q)
        assert (got["path"][r] >= lim.lo).all() and (got["path"][r] <= lim.hi).all(), "the waypoints lie inside the joint limits"
        assert (got["poly"][r, n:] == 0).all()
        polys.append(poly)
    return polys


def test_clear_goal_is_a_straight_line():
    _check_straight("clear", _plan("clear"))


def test_ignore_collision_goes_straight_through_the_post():
    _check_straight("post", _plan("post", ignore_collision=True))


def test_post_is_planned_around():
    got = _plan("post")
    print()
    polys = _check_plan("post", got, "post")
    assert (got["n_poly"] >= 3).all()
    # the current state and the same rows given as qpos_start are the same plan
    c, sc = pc.case("post"), _scene("post")
    again = _plan("post", qpos_start=torch.as_tensor(c["q"], device=sc.device))
    assert all(np.array_equal(got[k], again[k]) for k in got)
    assert len(polys) == B


def _path_tol(name, paths):
    c = pc.case(name)
    tol = 0.0
    for r in range(B):
        _, samples = plan_ref.polyline_clearance(pc.problem(name), c["q"][r], paths[r].astype(np.float64), pc.RESOLUTION)
        tol = max(tol, _tol(name, r, samples)[0])
    return tol


@pytest.mark.parametrize("kind", ["straight, K = 2", "detour, K = 70"])
def test_path_clearance(kind):
    c, sc = pc.case("post"), _scene("post")
    margin = 0.01
    if kind.startswith("straight"):
        paths = np.stack([c["start"], c["goal"]], 1)
    else:   # the reference's detour, planned with a margin so that "not in collision" is not a matter of rounding
        paths = np.stack([plan_ref.resample(pc.reference("post", r, margin=margin)["poly"], 70, np.float64) for r in range(B)]).astype(np.float32)
    K = paths.shape[1]
    got = {k: v.cpu().numpy() for k, v in sc.path_clearance(c["probes"], c["links"], c["qadr"], paths, resolution=pc.RESOLUTION, margin=0.0, skip_geoms=c["skip"]).items()}
    assert got["seg_min"].shape == (B, K - 1)
    tol = _path_tol("post", paths)
    worst = 0.0
    for r in range(B):
        seg, rmin, first = plan_ref.path_clearance(pc.problem("post"), c["q"][r], paths[r].astype(np.float64), pc.RESOLUTION, 0.0)
        worst = max(worst, float(np.abs(got["seg_min"][r] - seg).max()), abs(float(got["row_min"][r]) - float(rmin)))
        sure = (np.abs(seg) > tol).all()   # (no segment's verdict is a matter of rounding)
        if sure:
            assert int(got["row_first_blocked"][r]) == first, (r, got["row_first_blocked"][r], first)
        assert float(got["row_min"][r]) == float(got["seg_min"][r].min())
    print(f"\n[path clearance, {kind}] seg_min / row_min against float64 {worst:.3e} allowed {tol:.3e}; row_min {got['row_min']}")
    assert worst <= tol
    robot = pc.arm(c["sb"], sc)
    flag = robot.path_in_collision(torch.as_tensor(paths, device=sc.device).permute(1, 0, 2))
    assert flag.shape == (B,) and bool(flag.all() if kind.startswith("straight") else (~flag).all()), flag
    det = robot.get_path_clearance(torch.as_tensor(paths, device=sc.device).permute(1, 0, 2), return_detail=True)
    assert np.array_equal(det["clearance"].cpu().numpy(), got["row_min"]) and np.array_equal(det["seg_min"].cpu().numpy(), got["seg_min"])
    assert np.array_equal(det["first_blocked"].cpu().numpy(), got["row_first_blocked"])


def test_a_configuration_that_is_not_finite_is_blocked():
    """a NaN or an infinity in a trajectory, in the start row's planned joints or in a free body's pose is never "clear": left to the
    comparisons of the distance code such a probe would lose against every geom and count as a miss"""
    c, sc = pc.case("clear"), _scene("clear")
    paths = np.stack([plan_ref.resample(np.stack([c["start"][r], c["goal"][r]]), 6, np.float32) for r in range(B)])
    clean = {k: v.cpu().numpy() for k, v in sc.path_clearance(c["probes"], c["links"], c["qadr"], paths, skip_geoms=c["skip"]).items()}
    assert (clean["row_first_blocked"] == -1).all() and (clean["row_min"] > 0.02).all()
    bad = paths.copy()
    bad[1, 3, 2] = np.nan          # one joint of one point: segments 2 and 3 of row 1
    bad[3, 5, 8] = np.inf          # the last point of row 3: its last segment
    got = {k: v.cpu().numpy() for k, v in sc.path_clearance(c["probes"], c["links"], c["qadr"], bad, skip_geoms=c["skip"]).items()}
    assert got["row_first_blocked"].tolist() == [-1, 2, -1, 4, -1] and np.isneginf(got["row_min"][[1, 3]]).all()
    assert np.isneginf(got["seg_min"][1, 2:4]).all() and np.isneginf(got["seg_min"][3, 4])
    keep = np.ones_like(got["seg_min"], bool)
    keep[1, 2:4], keep[3, 4] = False, False
    assert np.array_equal(got["seg_min"][keep], clean["seg_min"][keep]), "the other segments and rows are what they were"
    ref = plan_ref.path_clearance(pc.problem("clear"), c["q"][1], bad[1].astype(np.float64), pc.RESOLUTION, 0.0)
    assert ref[2] == 2 and np.isneginf(ref[1])
    robot = pc.arm(c["sb"], sc)
    assert robot.path_in_collision(torch.as_tensor(bad, device=sc.device).permute(1, 0, 2)).tolist() == [False, True, False, True, False]
    # the start row: a planned joint, then the cube's pose (a geom record)
    for col in (int(c["qadr"][4]), 9):
        q = c["q"].copy()
        q[2, col] = np.nan
        out = _plan("clear", qpos_start=torch.as_tensor(q, device=sc.device))
        assert out["status"].tolist() == [0, 0, S.PLAN_START_IN_COLLISION, 0, 0], (col, out["status"])
        r = sc.path_clearance(c["probes"], c["links"], c["qadr"], paths, qpos_start=torch.as_tensor(q, device=sc.device), skip_geoms=c["skip"])
        assert np.isneginf(r["row_min"].cpu().numpy()).tolist() == [False, False, col == 9, False, False]
    goal = c["goal"].copy()
    goal[0, 1] = np.nan
    assert _plan("clear", goal=goal)["status"].tolist() == [S.PLAN_GOAL_OUT_OF_LIMITS, 0, 0, 0, 0]


def test_smoothing_shortens():
    rough, smooth = _plan("post", smooth_passes=0), _plan("post")
    print()
    pr, ps = _check_plan("post", rough, "post, no smoothing"), _check_plan("post", smooth, "post, smoothed")
    for r in range(B):
        lr, ls = plan_ref.polyline_length(pr[r]), plan_ref.polyline_length(ps[r])
        print(f"[plan, smoothing] row {r}: {len(pr[r])} nodes, length {lr:.4f} -> {len(ps[r])} nodes, length {ls:.4f}")
        assert ls <= lr + 1e-6 * lr and len(ps[r]) <= len(pr[r])


def test_failures():
    c, sc = pc.case("post"), _scene("post")
    # the configuration of the straight segment deepest in the post, per row
    deep = []
    for r in range(B):
        pb = pc.problem("post")
        pb.set_row(c["q"][r])
        qs = plan_ref.edge_samples(c["start"][r].astype(np.float64), c["goal"][r].astype(np.float64), pc.RESOLUTION, np.float64)
        deep.append(min(qs, key=pb.clearance).astype(np.float32))
        assert pb.clearance(deep[-1]) < -0.01
    rows = [0, 1, 2, 3]
    start, goal = c["q"][rows].copy(), c["goal"][rows].copy()
    start[0, c["qadr"]] = deep[0]          # start in the post
    goal[1] = deep[1]                      # goal in the post
    goal[2, 0] = 3.0                       # joint 1 ends at 2.8973
    idx = torch.tensor(rows, device=sc.device)
    got = _plan("post", goal=goal, env_idx=idx, qpos_start=torch.as_tensor(start, device=sc.device))
    assert got["status"].tolist() == [S.PLAN_START_IN_COLLISION, S.PLAN_GOAL_IN_COLLISION, S.PLAN_GOAL_OUT_OF_LIMITS, S.PLAN_OK], got["status"]
    for k in range(3):
        assert np.array_equal(got["path"][k], np.repeat(start[k, c["qadr"]][None], W, 0)), "a failed row returns its start W times"
        assert got["n_poly"][k] == 1 and np.array_equal(got["poly"][k, 0], start[k, c["qadr"]])
    alone = _plan("post", goal=c["goal"][3:4], env_idx=torch.tensor([3], device=sc.device))
    full = _plan("post")
    for k in got:
        assert np.array_equal(got[k][3], alone[k][0]) and np.array_equal(got[k][3], full[k][3]), k
    # the budgets
    sealed = _plan("sealed", max_iterations=32)
    assert (sealed["status"] == S.PLAN_ITERATION_LIMIT).all() and (sealed["stats"][:, 0] == 32).all(), (sealed["status"], sealed["stats"])
    few = _plan("post", max_nodes=4)
    assert (few["status"] == S.PLAN_NODE_LIMIT).all() and (few["stats"][:, 1:3].max(1) == 4).all(), (few["status"], few["stats"])
    for out, cc in ((sealed, pc.case("sealed")), (few, c)):
        assert np.array_equal(out["path"], np.repeat(cc["start"][:, None], W, 1)) and (out["n_poly"] == 1).all()


def test_determinism_and_independence():
    sc = _scene("post")
    a, b = _plan("post"), _plan("post")
    assert all(np.array_equal(a[k], b[k]) for k in a)
    rows = _plan("post", goal=pc.case("post")["goal"][[3, 1]], env_idx=torch.tensor([3, 1], device=sc.device))
    for k in a:
        assert np.array_equal(rows[k], a[k][[3, 1]]), k
    other = _plan("post", seed=1)
    print()
    _check_plan("post", other, "post, seed 1", seed=1)
    assert any(other["n_poly"][r] != a["n_poly"][r] or not np.array_equal(other["poly"][r], a["poly"][r]) for r in range(B)), "another seed, another polyline"


def test_a_call_changes_nothing():
    import test_gpu_contact_forces as cf
    from gym_genesis.backend import models
    from gym_genesis.env import GenesisEnv

    n = 8
    _, acts = cf._grasp(n)
    envs = [GenesisEnv(task="cube_pick", robot="franka", num_envs=n, enable_pixels=False) for _ in range(2)]
    for e in envs:
        e.reset(seed=3)
    tasks = [e._env for e in envs]
    mirs = [t._mir for t in tasks]
    for m in mirs:
        m.set_diag(True)
    robot, cube = tasks[0].franka, tasks[0].cube
    A = torch.as_tensor(acts, device=mirs[0].device)
    v0 = [m.state_version for m in mirs]
    goal = torch.tensor(models.FRANKA_HOME, device=mirs[0].device).expand(n, 9).contiguous()
    for t in range(20):
        res = [e.step(A[8 * t % acts.shape[0]]) for e in envs]
        path, valid = robot.plan_path(goal, num_waypoints=8, max_iterations=64, ignore_entities=[cube], return_valid_mask=True)
        clear = robot.get_path_clearance(path, ignore_entities=[cube])
        for k in ("agent_pos", "environment_state"):
            assert torch.equal(res[0][0][k], res[1][0][k]), (t, k)
        assert torch.equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])
        for x, y in zip(mirs[0].get_state(), mirs[1].get_state()):   # qpos, qvel, targets, warm start
            assert torch.equal(x, y), t
        for x, y in zip(mirs[0].get_diag(points=True), mirs[1].get_diag(points=True)):
            assert torch.equal(x, y), t
        assert mirs[0].state_version - v0[0] == mirs[1].state_version - v0[1]
    assert path.shape == (8, n, 9) and valid.shape == (n,) and torch.isfinite(path).all() and torch.isfinite(clear).all()
    assert mirs[0].plan_launches == 40


def _raw_plan(sc, q, probes, links, qadr, goal, out, idx=None, R=0):
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    lk = None if links is None else np.ascontiguousarray(links, np.int32)
    qa = np.ascontiguousarray(qadr, np.int32)
    rc = sc.lib.mir_plan_path(sc.h, None if q is None else C.byref(q), p(probes), None if lk is None else lk.ctypes.data_as(C.c_void_p),
                              qa.ctypes.data_as(C.c_void_p), p(idx), R, None, p(goal), p(out["path"]), p(out["status"]), None, None, None, sc._stream())
    torch.cuda.synchronize()
    return rc, sc.lib.mir_last_error()


def test_refusals_launch_nothing():
    from gym_genesis.backend.lib import MirError, MirScene

    c, sc = pc.case("post"), _scene("post")
    N, D = len(c["probes"]), len(c["qadr"])
    probes, goal = torch.as_tensor(c["probes"], device=sc.device), torch.as_tensor(c["goal"], device=sc.device)
    out = {"path": torch.full((B, W, D), float("nan"), device=sc.device), "status": torch.full((B,), -7, dtype=torch.int32, device=sc.device)}
    good = lambda **kw: make_plan_query(N, D, W, 128, 512, skip_geoms=c["skip"], **kw)  # noqa: E731
    before, launches = sc.state_version, sc.__dict__.get("plan_launches", 0)
    assert _raw_plan(sc, good(), probes, c["links"], c["qadr"], goal, out)[0] == 0 and torch.isfinite(out["path"]).all()
    out["path"].fill_(float("nan"))
    out["status"].fill_(-7)
    bad = []
    q = good(); q.struct_size -= 8; bad.append(_raw_plan(sc, q, probes, c["links"], c["qadr"], goal, out))
    for d in (0, 17):
        q = good(); q.n_dofs = d; bad.append(_raw_plan(sc, q, probes, c["links"], c["qadr"], goal, out))
    for res in (0.0, -0.05, float("nan")):
        bad.append(_raw_plan(sc, good(resolution=res), probes, c["links"], c["qadr"], goal, out))
    q = good(); q.skip_geoms = 0; bad.append(_raw_plan(sc, q, probes, c["links"], c["qadr"], goal, out))   # the arm's own geoms move with the plan
    assert b"moving obstacle" in bad[-1][1]
    bad.append(_raw_plan(sc, good(margin=2.0), probes, c["links"], c["qadr"], goal, out))                  # max_distance <= margin
    q = good(); q.flags = 2; bad.append(_raw_plan(sc, q, probes, c["links"], c["qadr"], goal, out))
    bad.append(_raw_plan(sc, good(), probes, c["links"], [int(c["qadr"][0])] * D, goal, out))                # a joint twice
    bad.append(_raw_plan(sc, good(resolution=1e-3), probes, c["links"], c["qadr"], goal, out))             # range / resolution > 4096
    for rc, msg in bad:
        assert rc == -1 and b"mir_plan_path" in msg, (rc, msg)
    q = good(); q.max_nodes = 4096
    rc, msg = _raw_plan(sc, q, probes, c["links"], c["qadr"], goal, out)
    assert rc == -2 and b"LDS" in msg, (rc, msg)
    q = good(); q.n_probes = S.DIST_MAX_PROBES + 1
    rc, msg = _raw_plan(sc, q, probes, None, c["qadr"], goal, out)
    assert rc == -2 and b"mir_plan_path" in msg
    # an unlimited planned dof
    sb = pc.builder("post")
    sb.dofs[0]["limited"] = 0
    free = MirScene(sb.build(), 2)
    o2 = {"path": torch.full((2, W, D), float("nan"), device=free.device), "status": torch.full((2,), -7, dtype=torch.int32, device=free.device)}
    rc, msg = _raw_plan(free, good(), torch.as_tensor(c["probes"], device=free.device), c["links"], c["qadr"], torch.as_tensor(c["goal"][:2], device=free.device), o2)
    assert rc == -1 and b"no limits" in msg and torch.isnan(o2["path"]).all(), (rc, msg)
    free.close()
    # between mir_step_begin and mir_step_end
    bufs = (sc.empty(sc.agent_dim), sc.empty(sc.env_dim), sc.empty(), sc.empty(dtype=torch.uint8))
    state = [x.clone() for x in sc.get_state()]
    sc.step_begin(None, *bufs)
    rc, msg = _raw_plan(sc, good(), probes, c["links"], c["qadr"], goal, out)
    seg = torch.full((B, 1), float("nan"), device=sc.device)
    paths = torch.as_tensor(np.stack([c["start"], c["goal"]], 1), device=sc.device)
    qa = np.ascontiguousarray(c["qadr"], np.int32)
    rc2 = sc.lib.mir_path_clearance(sc.h, C.byref(good()), C.c_void_p(probes.data_ptr()), c["links"].ctypes.data_as(C.c_void_p), qa.ctypes.data_as(C.c_void_p),
                                    None, 0, None, C.c_void_p(paths.data_ptr()), 2, C.c_void_p(seg.data_ptr()), None, None, sc._stream())
    msg2 = sc.lib.mir_last_error()
    sc.step_end()
    assert rc == -1 and b"mir_plan_path" in msg and b"pending" in msg
    assert rc2 == -1 and b"mir_path_clearance" in msg2 and b"pending" in msg2
    sc.set_state(*state)   # (the shared scene goes back to the state the other tests compare)
    torch.cuda.synchronize()
    assert torch.isnan(out["path"]).all() and (out["status"] == -7).all() and torch.isnan(seg).all(), "a refused call launches nothing"
    assert sc.state_version >= before
    with pytest.raises(MirError):
        sc.plan_path(c["probes"], c["links"], c["qadr"], c["goal"], skip_geoms=0)
    assert sc.__dict__.get("plan_launches", 0) == launches
    assert C.sizeof(MirPlanQuery) == sc.lib.mir_plan_query_sizeof()


def test_entity_view_plan_path():
    from gym_genesis.backend import models
    from gym_genesis.backend.lib import MirScene
    from gym_genesis.tasks.views import EntityView

    c, sc = pc.case("clear"), _scene("clear")
    robot, cube = pc.arm(c["sb"], sc), EntityView(sc, c["sb"], "cube", ())
    raw = _plan("clear", num_waypoints=12)
    goal = torch.as_tensor(c["goal"], device=sc.device)
    path = robot.plan_path(goal, num_waypoints=12, max_nodes=128, max_iterations=512)
    assert path.shape == (12, B, 9) and np.array_equal(path.cpu().numpy(), raw["path"].transpose(1, 0, 2)), "qpos_start=None is the current state"
    p2, valid = robot.plan_path(goal[[3, 1]], qpos_start=torch.as_tensor(c["start"][[3, 1]], device=sc.device), envs_idx=[3, 1], num_waypoints=12,
                                max_nodes=128, max_iterations=512, return_valid_mask=True)
    assert valid.dtype == torch.bool and valid.all() and torch.equal(p2, path[:, [3, 1]])
    det = robot.plan_path(goal, num_waypoints=12, max_nodes=128, max_iterations=512, return_detail=True, timeout=5.0)
    assert sorted(det) == ["n_poly", "path", "poly", "stats", "status", "valid"] and det["poly"].shape == (B, S.PLAN_MAX_POLY, 9)
    with pytest.raises(NotImplementedError):
        robot.plan_path(goal, planner="PRM")
    # with_entity / ignore_entities reach the skip mask: the post scene, where only the post blocks the straight line
    cp, sp = pc.case("post"), _scene("post")
    rp, cube_p = pc.arm(cp["sb"], sp), EntityView(sp, cp["sb"], "cube", ())
    gp = torch.as_tensor(cp["goal"], device=sp.device)
    kw = dict(num_waypoints=12, max_nodes=128, max_iterations=512, return_detail=True)
    only_cube = rp.plan_path(gp, with_entity=cube_p, **kw)           # the post is not tested: straight through it
    assert (only_cube["n_poly"] == 2).all() and only_cube["valid"].all()
    without_cube = rp.plan_path(gp, ignore_entities=[cube_p], **kw)  # the post still is
    assert (without_cube["n_poly"] >= 3).all() and without_cube["valid"].all()
    # the stack scene: the second device model, a goal near the start
    sb = models.franka_cube_stack_scene()
    st = MirScene(sb.build(), 3)
    assert st.kernel == 64
    arm = EntityView(st, sb, "link0", models.FRANKA_JOINTS)
    full = st.get_state()[0].clone()
    full[:, arm._qcols] = torch.tensor(models.FRANKA_HOME[:7] + (0.02, 0.02), device=st.device)   # (this Panda is scaled: its fingers open to 0.024)
    st.set_state(qpos=full, qvel=torch.zeros((3, st.nv), device=st.device))
    q0 = arm.get_qpos().clone()
    g = q0.clone()
    g[:, 0] += 0.3
    g[:, 3] += 0.2
    d = arm.plan_path(g, num_waypoints=10, return_detail=True)
    assert d["path"].shape == (10, 3, 9) and d["valid"].all() and (d["n_poly"] == 2).all(), (d["status"], d["n_poly"])
    assert torch.equal(d["path"][0], q0) and torch.equal(d["path"][-1], g)
    assert not arm.path_in_collision(d["path"]).any()
    st.close()
