"""Certified swept clearance on the GPU (include/mirigid.h: mir_certify_path; backend/lib.py: MirScene.certify_path; tasks/views.py:
EntityView.certify_path, path_is_certified_clear).

The cases -- scenes, start rows, paths, sphere model -- are those of tests/cert_cases.py; tests/test_cert_cpu.py holds the conditions
that make the comparisons below fair.  States are SET.  R = 5, K <= 8, N = 57 spheres (deep_tree: 16 bodies, 8 probes), and all five rows
are judged in every case.

The GPU is judged on its OWN leaves, as tests/test_gpu_plan.py judges plans: which leaves a float32 run accepts may differ from the
float64 reference's wherever a test is decided within rounding, and every such tree is a valid run of the rule.
a. With max_leaves large enough: the leaves of every finished segment tile [0, 1]; replayed in float64 on those leaves (cert_ref.replay),
   seg_lower is the minimum of lo over the leaves, seg_upper the minimum of u over every node the rule evaluates for that tree and the
   endpoints, and every leaf's acceptance test holds -- each within tol32.
b. lower <= the dense float64 minimum (2048 samples per segment) + tol32 on every segment of every case: the independent check.
c. Statuses: clear and detour all CLEAR; post_line BLOCKED with upper < margin; budget, depth and nan as the rule says; segments behind a
   BUDGET segment are BUDGET.
d. thin: robot.path_in_collision(path, resolution=0.1) is False and robot.path_is_certified_clear(path) is False, status BLOCKED --
   what the feature buys.
e. Invisibility and addressing: state, state version and a following step are bit-identical with and without a call in between; env_idx
   with repeats; qpos_start given against the current state; a refusal writes no output byte; refused inside an open step.
f. BRACKET on detour: upper - lower <= tol + tol32 on every segment.
Yardstick, the project's rule: tol32 = 4 x max(float32 port against float64 on the same leaves, 2^-23 x L), printed before it is used.
L: the largest magnitude entering a bound -- the largest |coordinate| of a probe centre plus the largest hw v_i.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import cert_cases as cc
import cert_ref
import plan_cases as pc
from gym_genesis.backend import spec as S

pytestmark = pytest.mark.gpu

B = cc.B
MAX_LEAVES = 512
_scenes = {}


def _scene(name):
    if name not in _scenes:
        from gym_genesis.backend.lib import MirScene

        c = cc.case({"post": "detour"}.get(name, name))
        sc = MirScene(c["spec"], B)
        sc.set_state(qpos=c["q"], qvel=np.zeros((B, sc.nv), np.float32))
        _scenes[name] = sc
    return _scenes[name]


def _args(name):
    c = cc.case(name)
    return c, dict(probes=c["probes"], links=c["links"], dof_qadr=c["qadr"], skip_geoms=c["skip"], max_distance=c["max_distance"],
                   max_leaves=MAX_LEAVES, **c["par"])


def _call(name, rows=None, **over):
    """the case through MirScene.certify_path (rows: env indices, the paths of those rows) -> numpy arrays"""
    c, kw = _args(name)
    sc = _scene(c["scene"])
    kw.update(over)
    paths = c["paths"]
    if rows is not None:
        rows = np.asarray(rows)
        paths = paths[rows]
        kw["env_idx"] = torch.as_tensor(rows, device=sc.device)
    return {k: v.cpu().numpy() for k, v in sc.certify_path(paths=paths, **kw).items()}


def _leaves(got, r, s):
    n = int(got["stats"][r, 1])
    assert n <= MAX_LEAVES, "the capacity of the test holds every leaf"
    lv = got["leaves"][r, :n]
    assert (got["leaves"][r, n:] == -1).all(), "entries behind the count are not written"
    return [(int(l), int(k)) for (ss, l, k) in lv if ss == s]


def _judge(name, got, bracket=False):
    """a. and b. on every row and segment of a result -> the largest tol32 used"""
    c = cc.case(name)
    par = c["par"]
    margin, tol, guard = float(np.float32(par["margin"])), float(np.float32(par["tol"])), par["guard"]
    p64, p32 = cc.problem(name), cc.problem(name, np.float32)
    worst_tol, worst = 0.0, dict(lower=0.0, upper=0.0)
    for r in range(B):
        dense = cc.dense(name, r)
        finished = 0
        assert int(got["row_status"][r]) == int(got["seg_status"][r].max())
        notclear = np.flatnonzero(got["seg_status"][r] != 0)
        assert int(got["row_first"][r]) == (int(notclear[0]) if len(notclear) else -1)
        assert float(got["row_lower"][r]) == float(got["seg_lower"][r].min()) and float(got["row_upper"][r]) == float(got["seg_upper"][r].min())
        for s in range(c["paths"].shape[1] - 1):
            st, lo, up = int(got["seg_status"][r, s]), float(got["seg_lower"][r, s]), float(got["seg_upper"][r, s])
            lv = _leaves(got, r, s)
            tol32 = 4.0 * 2.0 ** -23 * 2.0
            if st in (S.CERT_CLEAR, S.CERT_UNDECIDED, S.CERT_DEPTH) or (st == S.CERT_BLOCKED and bracket):
                finished += 1
                assert cert_ref.tiles(lv), (name, r, s, lv)
                n64 = cert_ref.replay(p64, c["q"][r], c["paths"][r], s, lv, guard)
                n32 = cert_ref.replay(p32, c["q"][r], c["paths"][r], s, lv, guard)
                err = max(max(abs(float(x["lo"]) - float(y["lo"])), abs(float(x["u"]) - float(y["u"]))) for x, y in zip(n64, n32))
                L = max(x["L"] + x["reach"] for x in n64)
                tol32 = 4.0 * max(err, 2.0 ** -23 * L)
                lo64 = min(float(x["lo"]) for x in n64 if x["leaf"])
                up64 = float(n64[-1]["upper"])
                worst["lower"], worst["upper"] = max(worst["lower"], abs(lo - lo64)), max(worst["upper"], abs(up - up64))
                assert abs(lo - lo64) <= tol32 and abs(up - up64) <= tol32, (name, r, s, lo, lo64, up, up64, tol32)
                for x in n64:
                    if x["leaf"]:
                        held = (not bracket and x["lo"] >= margin - tol32) or x["lo"] >= x["upper"] - tol - tol32 or x["l"] == par["max_depth"]
                        assert held, (name, r, s, x)
                    assert x["l"] <= par["max_depth"]
                if st == S.CERT_CLEAR:
                    assert lo >= margin
                if st in (S.CERT_CLEAR, S.CERT_UNDECIDED):
                    assert lo >= margin or up - lo <= tol + tol32
            worst_tol = max(worst_tol, tol32)
            assert lo <= dense[s] + tol32, (name, r, s, lo, dense[s])   # b.
        assert int(got["stats"][r, 3]) == finished, (name, r, got["stats"][r], finished)
    print(f"\n[certify, {name}{' bracket' if bracket else ''}] seg_lower / seg_upper against float64 on the GPU's own leaves "
          f"{worst['lower']:.3e} / {worst['upper']:.3e}, largest tol32 {worst_tol:.3e}; evaluations {got['stats'][:, 0]}, leaves {got['stats'][:, 1]}, "
          f"deepest {got['stats'][:, 2]}")
    return worst_tol


@pytest.mark.parametrize("name", cc.NAMES)
def test_bounds_on_the_gpus_own_leaves(name):
    """a., b. and c."""
    got = _call(name)
    _judge(name, got)
    st = got["seg_status"]
    K1 = st.shape[1]
    if name in ("clear", "detour", "deep_tree"):
        assert (st == S.CERT_CLEAR).all() and (got["row_first"] == -1).all() and (got["seg_lower"] >= 0.0).all(), st
    elif name in ("post_line", "thin"):
        assert (st == S.CERT_BLOCKED).all() and (got["seg_upper"] < 0.0).all() and (got["row_first"] == 0).all(), (st, got["seg_upper"])
    elif name == "budget":
        assert (st == S.CERT_BUDGET).all() and (got["stats"][:, 0] == 8).all() and np.isneginf(got["seg_lower"]).all()
        assert np.isposinf(got["seg_upper"][:, 1:]).all() and np.isfinite(got["seg_upper"][:, 0]).all(), "upper keeps what was sampled"
        # a budget that runs out later: the segments in front keep their verdict, everything behind is BUDGET
        later = _call(name, max_evaluations=40)
        for r in range(B):
            row = later["seg_status"][r]
            spent = np.flatnonzero(row == S.CERT_BUDGET)
            if len(spent):
                assert (row[spent[0]:] == S.CERT_BUDGET).all() and (row[:spent[0]] == S.CERT_CLEAR).all() and later["stats"][r, 0] == 40
            else:
                assert later["stats"][r, 0] <= 40
        assert (later["seg_status"] == S.CERT_BUDGET).any() and (later["seg_status"][:, 0] == S.CERT_CLEAR).any()
    elif name == "depth":
        assert (got["row_status"] == S.CERT_DEPTH).all() and (got["stats"][:, 2] == 2).all()
        assert ((st == S.CERT_DEPTH) | (st == S.CERT_CLEAR)).all()
    elif name == "nan":
        want = np.zeros((B, K1), int)
        want[1, :2] = S.CERT_NOT_FINITE
        assert np.array_equal(st, want), st
        assert np.isneginf(got["seg_lower"][1, :2]).all() and np.isposinf(got["seg_upper"][1, :2]).all() and got["row_first"][1] == 0
        clean = _call("detour")
        keep = np.ones((B, K1), bool)
        keep[1, :2] = False
        assert np.array_equal(got["seg_lower"][keep], clean["seg_lower"][keep]), "the other segments and rows are what they were"


def test_bracket_mode_closes_every_bracket():
    """f."""
    got = _call("detour", bracket=True)
    tol32 = _judge("detour", got, bracket=True)
    assert (got["seg_status"] == S.CERT_CLEAR).all()
    assert (got["seg_upper"] - got["seg_lower"] <= np.float32(cc.TOL) + tol32).all(), got["seg_upper"] - got["seg_lower"]
    plain = _call("detour")
    assert (got["stats"][:, 0] >= plain["stats"][:, 0]).all(), "closing every bracket costs at least what deciding the margin costs"


def test_thin_the_sampled_check_passes_and_the_certified_one_does_not():
    """d."""
    c = cc.case("thin")
    sc = _scene("thin")
    robot = pc.arm(c["sb"], sc)
    path = torch.as_tensor(c["paths"], device=sc.device).permute(1, 0, 2)
    sampled = robot.path_in_collision(path, resolution=cc.THIN_RESOLUTION, self_collision=False)
    assert sampled.shape == (B,) and not bool(sampled.any()), sampled
    certified = robot.path_is_certified_clear(path)
    assert certified.shape == (B,) and not bool(certified.any()), certified
    det = robot.certify_path(path, return_detail=True)
    assert (det["status"] == S.CERT_BLOCKED).all() and (det["upper"] < 0.0).all() and (det["first"] == 0).all()
    low = robot.get_path_clearance(path, resolution=cc.THIN_RESOLUTION, self_collision=False)
    print(f"\n[certify, thin] sampled clearance at 0.1 {low.cpu().numpy().round(5)}, certified upper {det['upper'].cpu().numpy().round(5)}")
    assert (low >= 1e-3).all()


def test_entity_view():
    c = cc.case("detour")
    sc = _scene("post")
    robot = pc.arm(c["sb"], sc)
    raw = _call("detour", max_leaves=0)
    path = torch.as_tensor(c["paths"], device=sc.device).permute(1, 0, 2)
    status = robot.certify_path(path)
    assert status.dtype == torch.int32 and np.array_equal(status.cpu().numpy(), raw["row_status"]) and bool(robot.path_is_certified_clear(path).all())
    det = robot.certify_path(path, return_detail=True, bracket=True, max_leaves=4)
    assert det["leaves"].shape == (B, 4, 3) and (det["stats"][:, 1] > 4).all(), "leaves beyond the capacity are counted, not stored"
    assert set(det) == {"status", "first", "lower", "upper", "seg_lower", "seg_upper", "seg_status", "stats", "leaves"}
    margin = robot.certify_path(path, margin=0.05)
    assert (margin != S.CERT_CLEAR).all(), "the detour passes the post nearer than 5 cm"
    ignored = sc.certify_path(paths=c["paths"], ignore_collision=True, **{k: v for k, v in _args("detour")[1].items()})
    assert (ignored["seg_status"] == 0).all() and (ignored["seg_lower"] == 1.0).all() and (ignored["seg_upper"] == 1.0).all()
    assert (ignored["stats"][:, :3] == 0).all() and (ignored["stats"][:, 3] == c["paths"].shape[1] - 1).all()
    with pytest.raises(ValueError, match="sampled only"):
        robot.certify_path(path, self_collision=True)
    with pytest.raises(ValueError, match="sampled only"):
        robot.certify_path(path, attached_entity=robot)
    with pytest.raises(ValueError, match="path must be"):
        robot.certify_path(path[:1])


def test_addressing():
    """e. env_idx with repeats, qpos_start against the current state, one launch of R rows against R launches of one"""
    name = "detour"
    base, again = _call(name), _call(name)
    assert all(np.array_equal(base[k], again[k], equal_nan=True) for k in base), "two identical calls give identical bits"
    idx = np.array([3, 0, 3, 4, 2, 1, 0])
    got = _call(name, rows=idx)
    assert all(np.array_equal(got[k], base[k][idx]) for k in base), "env_idx with repeats: row k is the path of env_idx[k]"
    for r in (0, 4):
        one = _call(name, rows=[r])
        assert all(np.array_equal(one[k][0], base[k][r]) for k in base), "one launch of R rows equals R launches of one row"
    c = cc.case(name)
    rows = _call(name, qpos_start=c["q"])
    assert all(np.array_equal(rows[k], base[k]) for k in base), "qpos_start rows equal to the state give the same bits"
    # start rows that differ from the state: the cube (a tested geom) moved into the arm -> another answer than the state's
    import plan_ref

    pb = cc.problem(name)
    pb.set_row(c["q"][0])
    qa = plan_ref.kin_ref.Model(c["spec"]).qadr[c["sb"].body_index("cube")]
    moved = c["q"].copy()
    moved[:, qa:qa + 3] = pb.centres(c["paths"][0, 0].astype(np.float64))[-1]   # (onto the last sphere of row 0's first waypoint)
    other = _call(name, qpos_start=moved)
    assert not np.array_equal(other["seg_upper"], base["seg_upper"]), "the start rows are read, not the state"
    assert all(np.array_equal(_call(name)[k], base[k]) for k in base)


def test_invisible_to_the_scene_and_refusals_write_nothing():
    """e."""
    from gym_genesis.backend.lib import MirError, _ptr

    c, kw = _args("detour")
    sc = _scene("post")
    state, version = [x.clone() for x in sc.get_state()], sc.state_version
    launches = sc.__dict__.get("cert_launches", 0)
    sc.step(1)
    after_plain = [x.clone() for x in sc.get_state()]
    sc.set_state(*state)
    version = sc.state_version
    out = sc.certify_path(paths=c["paths"], **kw)
    assert (out["row_status"] == 0).all() and sc.__dict__.get("cert_launches", 0) == launches + 1
    assert all(torch.equal(x, y) for x, y in zip(state, sc.get_state())) and sc.state_version == version
    sc.step(1)
    assert all(torch.equal(x, y) for x, y in zip(after_plain, sc.get_state())), "a following step does not see the call"
    sc.set_state(*state)
    # refusals: each names the entry point, launches nothing and writes no output byte
    for bad in (dict(max_depth=21), dict(max_evaluations=0), dict(tol=1e-6), dict(guard=-1.0), dict(margin=-1.0), dict(max_distance=0.0)):
        with pytest.raises(MirError, match="mir_certify_path"):
            sc.certify_path(paths=c["paths"], **{**kw, **bad})
    with pytest.raises(MirError, match="mir_certify_path"):
        sc.certify_path(paths=c["paths"], **{**kw, "skip_geoms": 0})   # the arm's own geoms ride on the planned joints
    K = c["paths"].shape[1]
    q = S.make_cert_query(K, max_depth=21, max_leaves=4)
    pq = S.make_plan_query(len(c["probes"]), len(c["qadr"]), skip_geoms=c["skip"])
    p, lk, qa, idx, R, qs = sc._plan_front(c["probes"], c["links"], c["qadr"], None, None)
    paths = torch.as_tensor(c["paths"], device=sc.device)
    f = lambda *shape: torch.full((B, *shape), -7.0, device=sc.device)  # noqa: E731
    i = lambda *shape: torch.full((B, *shape), -7, dtype=torch.int32, device=sc.device)  # noqa: E731
    bufs = [f(K - 1), f(K - 1), i(K - 1), f(), f(), i(), i(), i(4, 3), i(4)]
    rc = sc.lib.mir_certify_path(sc.h, C.byref(q), C.byref(pq), _ptr(p), lk.ctypes.data_as(C.c_void_p), qa.ctypes.data_as(C.c_void_p), _ptr(idx), R,
                                 _ptr(qs), _ptr(paths), *(_ptr(b) for b in bufs), sc._stream())
    torch.cuda.synchronize()
    assert rc == -1 and all(bool((b == -7).all()) for b in bufs), "a refusal writes no output byte"
    q.max_depth = 12
    rc = sc.lib.mir_certify_path(sc.h, C.byref(q), C.byref(pq), _ptr(p), lk.ctypes.data_as(C.c_void_p), qa.ctypes.data_as(C.c_void_p), _ptr(idx), R,
                                 _ptr(qs), _ptr(paths), *([None] * 9), sc._stream())
    assert rc == -1, "max_leaves > 0 without leaves"
    q.max_leaves = 0
    rc = sc.lib.mir_certify_path(sc.h, C.byref(q), C.byref(pq), _ptr(p), lk.ctypes.data_as(C.c_void_p), qa.ctypes.data_as(C.c_void_p), _ptr(idx), R,
                                 _ptr(qs), _ptr(paths), *([None] * 9), sc._stream())
    assert rc == 0, "every output NULL: MIR_OK, nothing to do"
    none = sc.certify_path(paths=c["paths"][:0], env_idx=torch.zeros(0, dtype=torch.long), **kw)
    assert none["seg_lower"].shape == (0, K - 1) and sc.__dict__.get("cert_launches", 0) == launches + 1, "no rows: no launch"
    assert C.sizeof(S.MirCertQuery) == sc.lib.mir_cert_query_sizeof()
    step_bufs = (sc.empty(sc.agent_dim), sc.empty(sc.env_dim), sc.empty(), sc.empty(dtype=torch.uint8))
    sc.step_begin(None, *step_bufs)
    try:
        with pytest.raises(MirError, match="mir_certify_path"):
            sc.certify_path(paths=c["paths"], **kw)
    finally:
        sc.step_end()
        sc.set_state(*state)
        torch.cuda.synchronize()


def test_the_example_runs(monkeypatch):
    """examples/franka/certify_plan.py at 8 envs: every env plans round the post with a 1 cm margin, and every plan is certified CLEAR at
    margin 0 -- the sampled plan keeps 1 cm at samples 0.05 rad apart, which the paths' true minimum cannot undercut by a centimetre"""
    import importlib.util
    import os
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("certify_plan", os.path.join(root, "examples", "franka", "certify_plan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(sys, "argv", ["certify_plan.py", "--num-envs", "8", "--waypoints", "24"])
    res = mod.main()
    print(f"\n[certify, example] {res}")
    assert res["planned"] == 8 and sum(res["statuses"].values()) == 8 and res["evaluations_median"] >= 24
