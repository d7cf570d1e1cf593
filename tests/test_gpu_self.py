"""Self-collision of the sphere model on the GPU (include/mirigid.h "self-collision": mir_self_distance, mir_plan_path_self,
mir_path_clearance_self; tasks/views.py: get_self_clearance / in_self_collision and the self_collision= argument of plan_path /
get_path_clearance / path_in_collision).

The cases are those of tests/self_cases.py ("fold", "swing": nothing of the scene is in the way, the straight segment drives the arm
into itself); tests/test_self_cpu.py holds the conditions that make "every row finds a plan" fair.  States are SET.  B = 5.

Yardstick (the rule of tests/test_gpu_distance.py and tests/test_gpu_plan.py): tol = 4 x max(error of the float32 port of
tests/self_ref.py against float64 on the same configurations, 2^-23 x L), L = the largest absolute world coordinate of a probe centre or
value on those configurations; tol_q the same for the resampler with Q = max |q|.  Both are printed before they are used.  The GPU's
plans are judged on their own, never against the reference's plan.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import plan_cases as pc
import plan_ref
import self_cases as sc
import self_ref
from gym_genesis.backend import spec as S
from gym_genesis.backend.spec import make_plan_query, make_self_query

pytestmark = pytest.mark.gpu

B, W = sc.B, sc.BUDGET["W"]
CASES = ("fold", "swing")
_scenes = {}


def _scene(name):
    """one scene per case ("post": that of tests/plan_cases.py), at the case's start rows"""
    if name not in _scenes:
        from gym_genesis.backend.lib import MirScene

        c = pc.case(name) if name == "post" else sc.case(name)
        s = MirScene(c["spec"], B)
        s.set_state(qpos=c["q"], qvel=np.zeros((B, s.nv), np.float32))
        _scenes[name] = s
    return _scenes[name]


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _self_model(c, **kw):
    return dict(link_mask=c["mask"], n_extra=c["n_extra"], **kw)


def _full_rows(c, planned):
    q = c["q"].copy()
    q[:, c["qadr"]] = planned
    return q


# ---------------------------------------------------------------- mir_self_distance
def _distance_rows(name):
    """five configurations that mix clear and self-colliding ones: the deepest point of rows 0, 2 and 4's straight edges, the goals of 1, 3"""
    c = sc.case(name)
    return np.stack([sc.deepest(name, r) if r % 2 == 0 else c["goal"][r] for r in range(B)])


def _check_self_distance(name, got, planned, label, max_distance=1.0):
    c = sc.case(name)
    p64, p32 = sc.problem(name), sc.problem(name, np.float32)
    worst, tol_all, skipped, compared = 0.0, 0.0, 0, 0
    for r in range(B):
        qp = None if planned is None else planned[r]
        d64, o64, m64, pair64, runner, raw = self_ref.self_distance(p64, c["q"][r], None if qp is None else qp.astype(np.float64), max_distance)
        d32 = self_ref.self_distance(p32, c["q"][r], qp, max_distance)[0]
        L = max(float(np.abs(p64.centres(p64.q[p64.qadr] if qp is None else qp.astype(np.float64))).max()), float(np.abs(d64).max()))
        port = float(np.abs(d32.astype(np.float64) - d64).max())
        tol = 4.0 * max(port, 2.0 ** -23 * L)
        near_cap = np.abs(raw - max_distance) <= tol   # (hit or miss is a matter of rounding there)
        err = float(np.abs(got["distance"][r] - d64)[~near_cap].max())
        worst, tol_all = max(worst, err, abs(float(got["row_min"][r]) - float(m64))), max(tol_all, tol)
        assert err <= tol and abs(float(got["row_min"][r]) - float(m64)) <= tol, (label, r, err, tol)
        sure = ((runner > 1e-4) | (o64 < 0)) & ~near_cap
        skipped, compared = skipped + int((~sure).sum()), compared + len(sure)
        assert np.array_equal(got["other"][r][sure], o64[sure]), (label, r)
        assert float(got["row_min"][r]) == float(got["distance"][r].min()) or pair64[0] < 0
        # the row's pair: compared when no other pair comes within 1e-4 m of the lowest
        others = np.delete(d64, [i for i in pair64 if i >= 0])
        if pair64[0] >= 0 and runner[pair64[0]] > 1e-4 and (len(others) == 0 or others.min() - m64 > 1e-4):
            assert tuple(got["row_pair"][r]) == pair64, (label, r, got["row_pair"][r], pair64)
        i, j = (int(v) for v in got["row_pair"][r])
        assert (i, j) == (-1, -1) or (0 <= i < j and got["other"][r][i] == j and got["distance"][r][i] == got["row_min"][r])
    print(f"[self distance, {label}] distance / row_min against float64 {worst:.3e} allowed {tol_all:.3e}; row_min {got['row_min']}; "
          f"{skipped} of {compared} probes ambiguous")
    assert skipped <= 0.05 * compared
    return got


@pytest.mark.parametrize("name", CASES)
def test_self_distance(name):
    c, s = sc.case(name), _scene(name)
    args = dict(link_mask=c["mask"], n_extra=c["n_extra"], other=True, row_min=True)
    print()
    at_state = _check_self_distance(name, _np(s.self_distance(c["probes"], c["links"], **args)), None, f"{name}, state")
    assert (at_state["row_min"] >= 0.02 - 1e-4).all(), "the start rows are clear of themselves"
    planned = _distance_rows(name)
    rows = torch.as_tensor(_full_rows(c, planned), device=s.device)
    at_rows = _check_self_distance(name, _np(s.self_distance(c["probes"], c["links"], qpos=rows, **args)), planned, f"{name}, qpos rows")
    assert (at_rows["row_min"][[0, 2, 4]] < -0.01).all() and (at_rows["row_min"][[1, 3]] >= 0.02 - 1e-4).all()
    # a short cap: misses are max_distance and -1
    capped = _check_self_distance(name, _np(s.self_distance(c["probes"], c["links"], qpos=rows, max_distance=0.03, **args)), planned, f"{name}, cap 0.03", 0.03)
    assert (capped["other"] == -1).any() and (capped["distance"][capped["other"] == -1] == np.float32(0.03)).all()
    # rows in another order, a subset, repeats
    idx = torch.tensor([3, 0, 0], device=s.device)
    sub = _np(s.self_distance(c["probes"], c["links"], env_idx=idx, **args))
    for k in at_state:
        assert np.array_equal(sub[k], at_state[k][[3, 0, 0]]), k
    # the entity's getters are the same launch
    robot = sc.arm(c, s)
    det = robot.get_self_clearance(qpos=torch.as_tensor(planned, device=s.device), return_detail=True)
    assert np.array_equal(det["clearance"].cpu().numpy(), at_rows["row_min"]) and np.array_equal(det["spheres"].cpu().numpy(), at_rows["row_pair"])
    assert np.array_equal(det["links"].cpu().numpy(), c["links"][at_rows["row_pair"]])
    assert robot.in_self_collision(qpos=torch.as_tensor(planned, device=s.device)).tolist() == [True, False, True, False, True]
    assert not robot.in_self_collision().any() and robot.in_self_collision(margin=0.06).all()
    # nothing enabled: every distance is the cap; a centre that is not finite: the row is -infinity
    none = _np(s.self_distance(c["probes"], c["links"], link_mask=np.zeros(32, np.uint32), n_extra=c["n_extra"], other=True, row_min=True))
    assert (none["distance"] == 1.0).all() and (none["other"] == -1).all() and (none["row_min"] == 1.0).all() and (none["row_pair"] == -1).all()
    bad = _full_rows(c, planned)
    bad[1, c["qadr"][3]] = np.nan
    nf = _np(s.self_distance(c["probes"], c["links"], qpos=torch.as_tensor(bad, device=s.device), **args))
    assert np.isneginf(nf["distance"][1]).all() and np.isneginf(nf["row_min"][1]) and (nf["other"][1] == -1).all() and (nf["row_pair"][1] == -1).all()
    keep = [0, 2, 3, 4]
    assert all(np.array_equal(nf[k][keep], at_rows[k][keep]) for k in nf)


# ---------------------------------------------------------------- nothing to test: the bytes of mir_plan_path / mir_path_clearance
def test_an_empty_self_model_is_the_plain_planner():
    c, s = pc.case("post"), _scene("post")
    args = dict(num_waypoints=W, max_nodes=pc.BUDGET["max_nodes"], max_iterations=pc.BUDGET["max_iterations"], resolution=pc.RESOLUTION, step=pc.STEP,
                margin=pc.MARGIN, skip_geoms=c["skip"])
    empty = dict(link_mask=np.zeros(32, np.uint32), n_extra=0)
    plain = _np(s.plan_path(c["probes"], c["links"], c["qadr"], c["goal"], **args))
    with_self = _np(s.plan_path(c["probes"], c["links"], c["qadr"], c["goal"], self_model=empty, **args))
    assert (plain["status"] == 0).all() and (plain["n_poly"] >= 3).all()
    for k in plain:
        assert plain[k].tobytes() == with_self[k].tobytes(), k
    for paths in (np.stack([c["start"], c["goal"]], 1), plain["path"]):
        kw = dict(resolution=pc.RESOLUTION, margin=0.0, skip_geoms=c["skip"])
        a = _np(s.path_clearance(c["probes"], c["links"], c["qadr"], paths, **kw))
        b = _np(s.path_clearance(c["probes"], c["links"], c["qadr"], paths, self_model=empty, **kw))
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k
        assert (b["seg_self_min"] == 1.0).all() and (b["row_self_min"] == 1.0).all()


# ---------------------------------------------------------------- planning
def _tol(name, row, samples):
    """4 x max(float32 port against float64 on these configurations -- both values --, 2^-23 L)"""
    c = sc.case(name)
    p64, p32 = sc.problem(name), sc.problem(name, np.float32)
    p64.set_row(c["q"][row])
    p32.set_row(c["q"][row])
    err, L = 0.0, 0.0
    for q in samples:
        v64, v32 = p64.both(q), p32.both(np.asarray(q, np.float32))
        err = max(err, abs(float(v32[0]) - float(v64[0])), abs(float(v32[1]) - float(v64[1])))
        L = max(L, float(np.abs(p64.centres(q)).max()), abs(float(v64[0])), abs(float(v64[1])))
    return 4.0 * max(err, 2.0 ** -23 * L), err, L


@pytest.mark.parametrize("name", CASES)
def test_planning_around_the_arm_itself(name):
    from gym_genesis.tasks.views import EntityView

    c, s = sc.case(name), _scene(name)
    robot, cube = sc.arm(c, s), EntityView(s, c["sb"], "cube", ())
    goal = torch.as_tensor(c["goal"], device=s.device)
    kw = dict(num_waypoints=W, max_nodes=sc.BUDGET["max_nodes"], max_iterations=sc.BUDGET["max_iterations"], resolution=sc.RESOLUTION, step=sc.STEP,
              margin=sc.MARGIN, ignore_entities=[cube], return_detail=True)
    # without the self test the straight line is "valid"
    blind = robot.plan_path(goal, self_collision=False, **kw)
    assert blind["valid"].all() and (blind["n_poly"] == 2).all() and (blind["stats"][:, 0] == 0).all()
    det = robot.get_path_clearance(blind["path"], self_collision=True, ignore_entities=[cube], return_detail=True)
    print(f"\n[self plan, {name}] the straight line: scene clearance {det['clearance'].cpu().numpy()} self clearance {det['self_clearance'].cpu().numpy()} "
          f"first blocked {det['first_blocked'].cpu().numpy()}")
    assert (det["first_blocked"] >= 0).all() and (det["self_clearance"] < 0).all() and (det["clearance"] >= 0.02 - 1e-4).all()
    assert det["self_seg_min"].shape == (B, W - 1) and torch.equal(det["self_seg_min"].min(1).values, det["self_clearance"])
    assert robot.path_in_collision(blind["path"], self_collision=True, ignore_entities=[cube]).all()
    assert not robot.path_in_collision(blind["path"], ignore_entities=[cube]).any(), "the scene's option is off: today's answer"
    both = robot.get_path_clearance(blind["path"], self_collision=True, ignore_entities=[cube])
    assert torch.equal(both, torch.minimum(det["clearance"], det["self_clearance"]))
    # with it: a detour on every row
    got = _np(robot.plan_path(goal, self_collision=True, **kw))
    assert (got["status"] == 0).all() and got["valid"].all(), (got["status"], got["stats"])
    assert (got["n_poly"] >= 3).all(), got["n_poly"]
    lim = sc.problem(name, np.float32)
    path = got["path"].transpose(1, 0, 2)
    for r in range(B):
        n = int(got["n_poly"][r])
        poly = got["poly"][r, :n].astype(np.float64)
        seg, seg_self, samples = self_ref.polyline_clearances(sc.problem(name), c["q"][r], poly, sc.RESOLUTION)
        tol, err, L = _tol(name, r, samples)
        ref64, ref32 = plan_ref.resample(poly, W, np.float64), plan_ref.resample(poly, W, np.float32)
        Q = float(np.abs(poly).max())
        port_q = float(np.abs(ref32.astype(np.float64) - ref64).max())
        tol_q = 4.0 * max(port_q, 2.0 ** -23 * Q)
        err_q = float(np.abs(path[r] - ref64).max())
        print(f"[self plan, {name}] row {r}: n_poly {n} lowest scene clearance {seg.min():.5f} self {seg_self.min():.5f} (tol {tol:.3e}: port {err:.3e}, "
              f"L {L:.3f}); waypoints {err_q:.3e} (tol_q {tol_q:.3e}: port {port_q:.3e}, Q {Q:.3f}); iterations / nodes / checked {got['stats'][r].tolist()}")
        assert np.array_equal(got["poly"][r, 0], c["start"][r]) and np.array_equal(got["poly"][r, n - 1], c["goal"][r])
        assert np.array_equal(path[r, 0], c["start"][r]) and np.array_equal(path[r, -1], c["goal"][r])
        assert seg.min() >= sc.MARGIN - tol, (name, r, seg.min(), tol)
        assert seg_self.min() >= sc.SELF_MARGIN - tol, (name, r, seg_self.min(), tol)
        assert err_q <= tol_q, (name, r, err_q, tol_q)
        assert (path[r] >= lim.lo).all() and (path[r] <= lim.hi).all() and (got["poly"][r, n:] == 0).all()
    # the same call twice, and the rows given as qpos_start
    again = _np(robot.plan_path(goal, self_collision=True, **kw))
    given = _np(robot.plan_path(goal, qpos_start=torch.as_tensor(c["start"], device=s.device), self_collision=True, **kw))
    for k in got:
        assert got[k].tobytes() == again[k].tobytes() and got[k].tobytes() == given[k].tobytes(), k
    # the planned path passes the swept check of both tests (at the tolerance of its own samples: the waypoints are resampled)
    det = robot.get_path_clearance(torch.as_tensor(got["path"], device=s.device), self_collision=True, ignore_entities=[cube], return_detail=True)
    print(f"[self plan, {name}] the planned waypoints: scene clearance {det['clearance'].cpu().numpy()} self clearance {det['self_clearance'].cpu().numpy()}")


# ---------------------------------------------------------------- statuses and refusals
def test_statuses():
    name = "fold"
    c, s = sc.case(name), _scene(name)
    args = dict(num_waypoints=W, max_nodes=sc.BUDGET["max_nodes"], max_iterations=sc.BUDGET["max_iterations"], resolution=sc.RESOLUTION, step=sc.STEP,
                margin=sc.MARGIN, skip_geoms=c["skip"])
    start, goal = c["start"].copy(), c["goal"].copy()
    start[0] = sc.deepest(name, 0)      # start in itself
    goal[1] = sc.deepest(name, 1)       # goal in itself
    start[2] = sc.IN_BOTH               # start in the ground and in itself: the scene test decides
    goal[3] = sc.IN_BOTH                # goal likewise
    rows = torch.as_tensor(_full_rows(c, start), device=s.device)
    got = _np(s.plan_path(c["probes"], c["links"], c["qadr"], goal, qpos_start=rows, self_model=_self_model(c), **args))
    assert got["status"].tolist() == [S.PLAN_START_IN_SELF_COLLISION, S.PLAN_GOAL_IN_SELF_COLLISION, S.PLAN_START_IN_COLLISION, S.PLAN_GOAL_IN_COLLISION,
                                      S.PLAN_OK], got["status"]
    for k in range(4):
        assert np.array_equal(got["path"][k], np.repeat(start[k][None], W, 0)) and got["n_poly"][k] == 1, "a failed row returns its start W times"
    full = _np(s.plan_path(c["probes"], c["links"], c["qadr"], c["goal"], self_model=_self_model(c), **args))
    assert all(np.array_equal(got[k][4], full[k][4]) for k in got), "a row's plan does not depend on the other rows"
    # without the self test the first two rows go straight through
    blind = _np(s.plan_path(c["probes"][:-c["n_extra"]], c["links"][:-c["n_extra"]], c["qadr"], goal, qpos_start=rows, **args))
    assert blind["status"].tolist() == [0, 0, S.PLAN_START_IN_COLLISION, S.PLAN_GOAL_IN_COLLISION, 0]
    # a self margin above the ends' own clearance (3.9 cm at the start): START_IN_SELF_COLLISION where it was OK
    tight = _np(s.plan_path(c["probes"], c["links"], c["qadr"], c["goal"], self_model=_self_model(c, self_margin=0.06), **args))
    assert (full["status"] == 0).all() and (tight["status"] == S.PLAN_START_IN_SELF_COLLISION).all()
    # ignore_collision switches both tests off
    free = _np(s.plan_path(c["probes"], c["links"], c["qadr"], goal, qpos_start=rows, ignore_collision=True, self_model=_self_model(c), **args))
    assert (free["status"] == 0).all() and (free["n_poly"] == 2).all() and (free["stats"][:, 3] == 0).all()
    # the swept check reports the first segment on which EITHER test fails
    paths = np.stack([c["start"], c["start"], c["goal"]], 1)
    paths[2, 1] = sc.IN_GROUND
    pcl = _np(s.path_clearance(c["probes"], c["links"], c["qadr"], paths, resolution=sc.RESOLUTION, skip_geoms=c["skip"], self_model=_self_model(c)))
    assert pcl["row_first_blocked"].tolist() == [1, 1, 0, 1, 1] and (pcl["seg_self_min"][[0, 1, 3, 4], 1] < -0.01).all() and (pcl["seg_min"][2, 0] < -0.01)
    assert (pcl["seg_self_min"][[0, 1, 3, 4], 0] >= 0.02 - 1e-4).all() and np.array_equal(pcl["row_self_min"], pcl["seg_self_min"].min(1))


def _raw(s, entry, q, sq, probes, links, qadr, goal, out, n_probes=None):
    """a raw call of one of the three entry points -> (return code, error text); `out`: the tensors it may write"""
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    lk = None if links is None else np.ascontiguousarray(links, np.int32)
    lkp = None if lk is None else lk.ctypes.data_as(C.c_void_p)
    qa = np.ascontiguousarray(qadr, np.int32)
    sqp = None if sq is None else C.byref(sq)
    if entry == "plan":
        rc = s.lib.mir_plan_path_self(s.h, C.byref(q), sqp, p(probes), lkp, qa.ctypes.data_as(C.c_void_p), None, 0, None, p(goal), p(out["path"]),
                                      p(out["status"]), None, None, None, s._stream())
    elif entry == "clear":
        rc = s.lib.mir_path_clearance_self(s.h, C.byref(q), sqp, p(probes), lkp, qa.ctypes.data_as(C.c_void_p), None, 0, None, p(out["paths"]), 2,
                                           p(out["seg"]), p(out["seg"]), None, None, None, s._stream())
    else:
        rc = s.lib.mir_self_distance(s.h, sqp, len(links) - (sq.n_extra if sq is not None else 0) if n_probes is None else n_probes, p(probes), lkp, None, 0,
                                     None, p(out["distance"]), None, None, None, s._stream())
    torch.cuda.synchronize()
    return rc, s.lib.mir_last_error()


def test_refusals_launch_nothing():
    name = "fold"
    c, s = sc.case(name), _scene(name)
    NS, E, D = len(c["links"]), c["n_extra"], len(c["qadr"])
    N = NS - E
    probes, goal = torch.as_tensor(c["probes"], device=s.device), torch.as_tensor(c["goal"], device=s.device)
    nan = lambda *shape: torch.full(shape, float("nan"), device=s.device)  # noqa: E731
    out = {"path": nan(B, W, D), "status": torch.full((B,), -7, dtype=torch.int32, device=s.device), "seg": nan(B, 1), "distance": nan(B, NS),
           "paths": torch.as_tensor(np.stack([c["start"], c["goal"]], 1), device=s.device)}
    q = make_plan_query(N, D, W, 128, 512, skip_geoms=c["skip"])
    good = lambda **kw: make_self_query(c["mask"], E, **kw)  # noqa: E731
    launches = s.__dict__.get("plan_launches", 0), s.__dict__.get("self_launches", 0)
    nbody = c["spec"].nbody
    assert nbody < 32
    bad = [None]
    sq = good(); sq.struct_size -= 4; bad.append(sq)
    sq = good(); sq.n_extra = -1; bad.append(sq)
    bad += [good(self_margin=-0.01), good(self_margin=float("nan")), good(self_margin=0.5, max_distance=0.5), good(max_distance=float("inf")),
            good(max_distance=float("nan"))]
    sq = good(); sq.flags = 1; bad.append(sq)
    sq = good(); sq.link_mask[2] |= 1 << 2; bad.append(sq)                      # a diagonal bit
    sq = good(); sq.link_mask[2] |= 1 << 3; bad.append(sq)                      # 2 -> 3 without 3 -> 2 (parent and child: not in the mask)
    sq = good(); sq.link_mask[1] |= 1 << nbody; sq.link_mask[nbody] |= 1 << 1; bad.append(sq)   # symmetric, but a body that does not exist
    for sq in bad:
        for entry, who in (("plan", b"mir_plan_path_self"), ("clear", b"mir_path_clearance_self"), ("distance", b"mir_self_distance")):
            rc, msg = _raw(s, entry, q, sq, probes, c["links"], c["qadr"], goal, out, n_probes=N)
            assert rc == -1 and who in msg, (entry, rc, msg)
    # capacity: more than 1024 probes together; the sphere list on top of trees that fill the LDS on their own
    sq = good(); sq.n_extra = S.DIST_MAX_PROBES + 1 - N
    for entry in ("plan", "clear", "distance"):
        rc, msg = _raw(s, entry, q, sq, probes, None, c["qadr"], goal, out, n_probes=N)
        assert rc == -2 and b"1024" in msg, (entry, rc, msg)
    assert 13856 + 2 * 680 * (4 * D + 2) == 65536    # (680 nodes per tree of 9 dofs fill what the fixed part leaves, to the byte)
    big = make_plan_query(N, D, W, 680, 512, skip_geoms=c["skip"])
    rc, msg = _raw(s, "plan", big, good(), probes, c["links"], c["qadr"], goal, out)
    assert rc == -2 and b"LDS" in msg and b"sphere list" in msg, (rc, msg)
    torch.cuda.synchronize()
    assert torch.isnan(out["path"]).all() and (out["status"] == -7).all() and torch.isnan(out["seg"]).all() and torch.isnan(out["distance"]).all(), \
        "a refused call launches nothing"
    rc = s.lib.mir_plan_path(s.h, C.byref(big), C.c_void_p(probes.data_ptr()), c["links"].ctypes.data_as(C.c_void_p),
                             np.ascontiguousarray(c["qadr"], np.int32).ctypes.data_as(C.c_void_p), None, 0, None, C.c_void_p(goal.data_ptr()),
                             C.c_void_p(out["path"].data_ptr()), C.c_void_p(out["status"].data_ptr()), None, None, None, s._stream())
    torch.cuda.synchronize()
    assert rc == 0 and torch.isfinite(out["path"]).all(), "the same trees without a sphere list fit"
    # the good query launches; between mir_step_begin and mir_step_end nothing does
    out["path"].fill_(float("nan"))
    assert _raw(s, "plan", q, good(), probes, c["links"], c["qadr"], goal, out)[0] == 0 and torch.isfinite(out["path"]).all()
    assert _raw(s, "distance", q, good(), probes, c["links"], c["qadr"], goal, out)[0] == 0 and torch.isfinite(out["distance"]).all()
    assert _raw(s, "clear", q, good(), probes, c["links"], c["qadr"], goal, out)[0] == 0 and torch.isfinite(out["seg"]).all()
    for t in (out["path"], out["seg"], out["distance"]):
        t.fill_(float("nan"))
    bufs = (s.empty(s.agent_dim), s.empty(s.env_dim), s.empty(), s.empty(dtype=torch.uint8))
    state = [x.clone() for x in s.get_state()]
    s.step_begin(None, *bufs)
    pending = [_raw(s, entry, q, good(), probes, c["links"], c["qadr"], goal, out) for entry in ("plan", "clear", "distance")]
    s.step_end()
    s.set_state(*state)   # (the shared scene goes back to the state the other tests compare)
    torch.cuda.synchronize()
    assert all(rc == -1 and b"pending" in msg for rc, msg in pending), pending
    assert torch.isnan(out["path"]).all() and torch.isnan(out["seg"]).all() and torch.isnan(out["distance"]).all()
    assert (s.__dict__.get("plan_launches", 0), s.__dict__.get("self_launches", 0)) == launches, "the wrappers' counters saw none of the raw calls"
    assert C.sizeof(S.MirSelfQuery) == s.lib.mir_self_query_sizeof()


# ---------------------------------------------------------------- invisibility
def test_the_new_calls_change_nothing():
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
    for t in range(12):
        res = [e.step(A[8 * t % acts.shape[0]]) for e in envs]
        own = robot.get_self_clearance()
        path, valid = robot.plan_path(goal, num_waypoints=8, max_iterations=64, ignore_entities=[cube], self_collision=True, return_valid_mask=True)
        clear = robot.get_path_clearance(path, ignore_entities=[cube], self_collision=True)
        for k in ("agent_pos", "environment_state"):
            assert torch.equal(res[0][0][k], res[1][0][k]), (t, k)
        assert torch.equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])
        for x, y in zip(mirs[0].get_state(), mirs[1].get_state()):   # qpos, qvel, targets, warm start
            assert torch.equal(x, y), t
        for x, y in zip(mirs[0].get_diag(points=True), mirs[1].get_diag(points=True)):
            assert torch.equal(x, y), t
        assert mirs[0].state_version - v0[0] == mirs[1].state_version - v0[1]
    assert path.shape == (8, n, 9) and valid.shape == (n,) and torch.isfinite(path).all() and torch.isfinite(clear).all() and torch.isfinite(own).all()
    assert mirs[0].plan_launches == 24 and mirs[0].self_launches == 12
