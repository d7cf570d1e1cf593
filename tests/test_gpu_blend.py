"""Batched collision-checked corner blending on the GPU (include/mirigid.h: mir_blend_path; backend/lib.py: MirScene.blend_path;
tasks/views.py: EntityView.blend_path).

The cases -- scenes, start rows, polylines, sphere model -- are those of tests/blend_cases.py; tests/test_blend_cpu.py holds the
conditions that make the comparisons below fair.  States are SET.  B = 5, and all five rows are judged in every case.

a. Judged on its own output, float64 as judge: the points of a blended corner lie on B(k / m) of the GPU's own accepted half-length;
   every point lies within max_deviation of the input polyline; the dense polyline keeps the margin; the ends carry the input's bits and
   the columns that do not move the start's; the tail repeats the last point; path = the float64 arc-length resampler of the GPU's own
   points.
b. Against the reference: status, M, n_points, the blended and sharp counts and the halvings per corner are equal (conditions 3 and 4 of
   the CPU tier); blend_len and the points match the float64 reference.
c. Addressing and equivalence: env_idx subsets and permutations, an empty carry and an all-zero self mask, one launch of R rows against
   R launches of one, the state untouched, a call inside an open step refused.
d. Through EntityView.blend_path.
Yardstick, the project's rule: tol = 4 x max(error of the float32 port against float64 on the same case, 2^-23 x L), printed before it is
used.  L: max |q| for configurations, the largest absolute coordinate for clearances.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import blend_cases as bc
import blend_ref
import plan_cases as pc
import plan_ref
import self_ref
from gym_genesis.backend import spec as S

pytestmark = pytest.mark.gpu

B, W, M_ = bc.B, bc.W, bc.M_CHORDS
_scenes = {}


def _scene(name):
    if name not in _scenes:
        from gym_genesis.backend.lib import MirScene

        c = bc.case("carry" if name == "under" else "free_corner")
        sc = MirScene(c["spec"], B)
        sc.set_state(qpos=c["q"], qvel=np.zeros((B, sc.nv), np.float32))
        _scenes[name] = sc
    return _scenes[name]


def _args(name):
    c = bc.case(name)
    kw = dict(probes=c["probes"], links=c["links"], dof_qadr=c["qadr"], skip_geoms=c["skip"], resolution=bc.RESOLUTION, margin=c["margin"],
              num_waypoints=W, ignore_collision=c["ignore"], **c["par"])
    if c["mask"] is not None:
        kw["self_model"] = dict(link_mask=c["mask"], n_extra=c["n_extra"], self_margin=0.0, max_distance=1.0)
    if c["carry"] is not None:
        kw["carry"] = dict(body=c["carry"][0], link=c["carry"][1])
    return c, kw


def _call(name, rows=None, **over):
    """the case through MirScene.blend_path (rows: env indices, the polylines of those rows) -> numpy arrays"""
    c, kw = _args(name)
    sc = _scene(c["scene"])
    kw.update(over)
    poly = c["poly"]
    if rows is not None:
        rows = np.asarray(rows)
        poly = poly[rows]
        kw["env_idx"] = torch.as_tensor(rows, device=sc.device)
    return {k: v.cpu().numpy() for k, v in sc.blend_path(poly=poly, **kw).items()}


def _port_tol(name, r, key="points"):
    """the yardstick of a configuration: 4 x max(float32 port against float64 on this row, 2^-23 L)"""
    a, b = bc.reference(name, r, "float64"), bc.reference(name, r, "float32")
    L = float(np.abs(a["points"]).max())
    err = float(np.abs(np.asarray(b[key], np.float64) - np.asarray(a[key], np.float64)).max()) if np.shape(a[key]) == np.shape(b[key]) else 0.0
    return 4.0 * max(err, 2.0 ** -23 * L), err, L


def _own_curve(c, r, got_len):
    """float64: the dense points the rule gives for the GPU's own half-lengths (blend_len of one row), duplicates dropped"""
    Q, kept, _ = blend_ref.compact(c["poly"][r], None, np.float64)
    pts = [Q[0]]
    ts = np.arange(M_ + 1) / M_
    for i in range(1, len(Q) - 1):
        h = float(got_len[kept[i]])
        if h > 0:
            up = (Q[i] - Q[i - 1]) / np.linalg.norm(Q[i] - Q[i - 1])
            un = (Q[i + 1] - Q[i]) / np.linalg.norm(Q[i + 1] - Q[i])
            pts.extend(blend_ref.corner_curve(Q[i], h, up, un, ts))
        else:
            pts.append(Q[i])
    pts.append(Q[-1])
    out = [pts[0]]
    for p in pts[1:]:
        if not np.array_equal(p.astype(np.float32), out[-1].astype(np.float32)):
            out.append(p)
    return np.stack(out), Q, kept


def _clearances(name, r, pts, dtype=np.float64):
    """the lowest clearance over the margin of the polyline pts under the case's problem, and the samples"""
    c = bc.case(name)
    pb = bc.problem(name, dtype)
    if hasattr(pb, "both"):
        seg, seg_self, samples = self_ref.polyline_clearances(pb, c["q"][r], pts, bc.RESOLUTION)
        return min(float(seg.min()) - c["margin"], float(seg_self.min())), samples
    seg, samples = plan_ref.polyline_clearance(pb, c["q"][r], pts, bc.RESOLUTION)
    return float(seg.min()) - c["margin"], samples


def _clear_tol(name, r, samples):
    """4 x max(float32 port against float64 on these configurations, 2^-23 L) for a clearance (the rule of tests/test_gpu_plan.py)"""
    c = bc.case(name)
    p64, p32 = bc.problem(name), bc.problem(name, np.float32)
    p64.set_row(c["q"][r])
    p32.set_row(c["q"][r])
    err, L = 0.0, 0.0
    for q in samples:
        v64 = p64.both(q) if hasattr(p64, "both") else (p64.clearance(q),)
        v32 = p32.both(np.asarray(q, np.float32)) if hasattr(p32, "both") else (p32.clearance(np.asarray(q, np.float32)),)
        for x, y in zip(v64, v32):
            if np.isfinite(float(x)) and np.isfinite(float(y)):
                err = max(err, abs(float(y) - float(x)))
        L = max(L, float(np.abs(p64.centres(q)).max()))
    return 4.0 * max(err, 2.0 ** -23 * L), err, L


def _judge(name, got, rows=None):
    """a. on every row of a result"""
    c = bc.case(name)
    P = got["points"].shape[1]
    delta = float(np.float32(c["par"]["max_deviation"]))
    for k in range(len(got["status"])):
        r = k if rows is None else int(rows[k])
        n, status = int(got["n_points"][k]), int(got["status"][k])
        pts = got["points"][k].astype(np.float64)
        poly = c["poly"][r]
        assert 1 <= n <= P and got["points"][k, 0].tobytes() == poly[0].tobytes(), "points[0] holds the first node's bits"
        assert (got["points"][k, n:] == got["points"][k, n - 1]).all() or status == blend_ref.NOT_FINITE, "the tail repeats the last point's bits"
        assert got["path"][k, 0].tobytes() == got["points"][k, 0].tobytes() and got["path"][k, -1].tobytes() == got["points"][k, n - 1].tobytes()
        if status != blend_ref.OK:
            assert n == 1 and not got["blend_len"][k].any() and (got["stats"][k, 1:3] == 0).all()
            assert all(got["path"][k, w].tobytes() == poly[0].tobytes() for w in range(W)), "a failed row returns its first node everywhere"
            continue
        assert (got["points"][k, :, 2:] == poly[0, 2:]).all() and (got["path"][k, :, 2:] == poly[0, 2:]).all(), "columns that do not move carry the start's bits"
        own, Q, kept = _own_curve(c, r, got["blend_len"][k])
        assert got["points"][k, n - 1].tobytes() == poly[kept[-1]].tobytes(), "the last point holds the last node's bits"
        tol, perr, L = _port_tol(name, r)
        assert len(own) == n, (name, r, len(own), n)
        err = float(np.abs(pts[:n] - own).max())
        far = max(blend_ref.point_to_polyline(p, Q) for p in pts[:n])
        print(f"[blend, {name}] row {r}: n_points {n}, half-lengths {got['blend_len'][k][got['blend_len'][k] > 0]}; off its own curve {err:.3e} "
              f"(tol {tol:.3e}: port {perr:.3e}, L {L:.3f}); farthest from the polyline {far:.5f} (max_deviation {delta:.3f})")
        assert err <= tol, (name, r, err, tol)
        assert far <= delta + tol, (name, r, far, delta)
        # (remainders_clear False: the caller's remainders are nearer than the margin by design; the chords of the blend alone are judged)
        mine = pts[:n] if c["remainders_clear"] else pts[1:n - 1]
        if not c["ignore"] and len(mine) > 1:
            low, samples = _clearances(name, r, mine)
            ctol, cerr, cL = _clear_tol(name, r, samples)
            print(f"[blend, {name}] row {r}: lowest clearance of the dense polyline over the margin {low:.5f} (tol {ctol:.3e}: port {cerr:.3e}, L {cL:.3f})")
            assert low >= -ctol, (name, r, low, ctol)
        r64, r32 = plan_ref.resample(pts[:n], W, np.float64), plan_ref.resample(pts[:n], W, np.float32)
        Qm = float(np.abs(pts).max())
        port_q = float(np.abs(r32.astype(np.float64) - r64).max())
        tol_q = 4.0 * max(port_q, 2.0 ** -23 * Qm)
        err_q = float(np.abs(got["path"][k] - r64).max())
        print(f"[blend, {name}] row {r}: waypoints against the float64 resampler {err_q:.3e} (tol_q {tol_q:.3e}: port {port_q:.3e}, Q {Qm:.3f})")
        assert err_q <= tol_q, (name, r, err_q, tol_q)


def _against_reference(name, got):
    """b. on every row"""
    c = bc.case(name)
    s = c["par"]["max_shrinks"]
    for r in range(B):
        ref = bc.reference(name, r)
        assert int(got["status"][r]) == ref["status"], (name, r, got["status"][r], ref["status"], got["stats"][r])
        assert int(got["n_points"][r]) == ref["n_points"], (name, r, got["n_points"][r], ref["n_points"])
        if ref["status"] == blend_ref.NOT_FINITE:
            continue
        assert int(got["stats"][r, 0]) == ref["M"] and int(got["stats"][r, 1]) == ref["blended"] and int(got["stats"][r, 2]) == ref["sharp"], (name, r, got["stats"][r])
        if ref["status"] != blend_ref.OK:
            assert int(got["stats"][r, 3]) == ref["checked"], (name, r, got["stats"][r], ref["checked"])
            continue
        halvings = []
        for i, corner in enumerate(ref["corners"], start=1):
            h = float(got["blend_len"][r, ref["kept"][i]])
            halvings.append(int(round(np.log2(float(corner["h0"]) / h))) if h > 0 else s + 1)
        assert halvings == ref["halvings"], (name, r, halvings, ref["halvings"])
        tol, perr, L = _port_tol(name, r)
        tol_h, perr_h, _ = _port_tol(name, r, "blend_len")
        n = ref["n_points"]
        err = float(np.abs(got["points"][r, :n].astype(np.float64) - ref["points"]).max())
        err_h = float(np.abs(got["blend_len"][r, :len(ref["blend_len"])].astype(np.float64) - ref["blend_len"]).max())
        print(f"[blend, {name}] row {r}: points against the float64 reference {err:.3e} (tol {tol:.3e}: port {perr:.3e}, L {L:.3f}); blend_len "
              f"{err_h:.3e} (tol {tol_h:.3e}: port {perr_h:.3e}); halvings {halvings}; checked GPU {int(got['stats'][r, 3])} reference {ref['checked']}")
        assert err <= tol and err_h <= tol_h, (name, r, err, tol, err_h, tol_h)
        assert int(got["stats"][r, 3]) == ref["checked"], (name, r, got["stats"][r], ref["checked"])   # (conditions 3 and 4 of the CPU tier)
        assert not got["blend_len"][r, len(ref["blend_len"]):].any()


@pytest.mark.parametrize("name", ("free_corner", "short_segments", "collinear", "repeats"))
def test_corners_are_blended(name):
    got = _call(name)
    _judge(name, got)
    _against_reference(name, got)
    if name == "short_segments":
        assert (got["n_points"] == 2 + 3 * (M_ + 1) - 2).all() and (got["blend_len"][:, 1:4] == np.float32(0.09375)).all()
    if name == "repeats":
        assert got["status"][0] == blend_ref.NO_MOTION and (got["status"][1:] == 0).all() and (got["blend_len"][1:, 2] > 0).all()


@pytest.mark.parametrize("name", ("corner_at_post", "two_halvings", "stays_sharp", "self_on", "carry"))
def test_blocked_blends_shrink(name):
    got = _call(name)
    assert (got["status"] == 0).all(), (got["status"], got["stats"])
    _judge(name, got)
    _against_reference(name, got)
    if name == "stays_sharp":   # blocked at h, halved, blocked again, given up: the checks of two_halvings without its third
        assert (got["stats"][:, 2] == 1).all() and (got["n_points"] == 3).all() and not got["blend_len"].any()
        assert (got["stats"][:, 3] < _call("two_halvings")["stats"][:, 3]).all() and (got["stats"][:, 3] > 2).all()
    elif name == "two_halvings":
        full = _call(name, ignore_collision=True)["blend_len"][:, 1]
        assert np.allclose(got["blend_len"][:, 1], 0.25 * full, rtol=1e-6), "a quarter of the full blend"
    elif name != "carry":
        full = _call("ignore")["blend_len"][:, 1]
        assert np.allclose(got["blend_len"][:, 1], 0.5 * full, rtol=1e-6), "the halved blend of the full one"


def test_statuses_and_ignore():
    for name in ("too_many", "not_finite", "ignore", "start_blocked"):
        got = _call(name)
        _judge(name, got)
        _against_reference(name, got)
    sb = _call("start_blocked")   # row 1 starts inside the post, row 3 folded onto itself: one configuration checked, nothing moves
    assert list(sb["status"]) == [0, blend_ref.START_IN_COLLISION, 0, blend_ref.START_IN_SELF_COLLISION, 0] and list(sb["stats"][:, 3]) [1::2] == [1, 1]
    assert (_call("too_many")["status"] == blend_ref.TOO_MANY_POINTS).all()
    nf = _call("not_finite")
    assert list(nf["status"]) == [0, 0, blend_ref.NOT_FINITE, 0, 0] and list(nf["n_points"]) == [11, 11, 1, 11, 11]
    ig = _call("ignore")
    assert (ig["stats"][:, 3] == 0).all() and (ig["stats"][:, 1] == 1).all(), "nothing is evaluated, the full blend is taken"
    n_poly = np.array([3, 2, 1, 0, 7], np.int32)   # the count of valid leading nodes: clamped to 1 .. K; 2 nodes: no corner
    part = _call("free_corner", n_poly=n_poly)
    assert list(part["status"]) == [0, 0, blend_ref.NO_MOTION, blend_ref.NO_MOTION, 0] and list(part["n_points"]) == [11, 2, 1, 1, 11]
    assert list(part["stats"][:, 0]) == [3, 2, 1, 1, 3]


def test_addressing_and_equivalence():
    name = "corner_at_post"
    base, again = _call(name), _call(name)
    assert all(np.array_equal(base[k], again[k]) for k in base), "two identical calls give identical bits"
    perm = np.array([3, 0, 4, 2, 1])
    got = _call(name, rows=perm)
    assert all(np.array_equal(got[k], base[k][perm]) for k in base), "an env_idx permutation gives row k the polyline of env_idx[k]"
    sub = _call(name, rows=[4, 1])
    assert all(np.array_equal(sub[k], base[k][[4, 1]]) for k in base), "a subset"
    for r in range(B):
        one = _call(name, rows=[r])
        assert all(np.array_equal(one[k][0], base[k][r]) for k in base), "one launch of R rows equals R launches of one row"
    c = bc.case(name)
    rows = _call(name, qpos_start=c["q"])
    assert all(np.array_equal(rows[k], base[k]) for k in base), "qpos_start rows equal to the state give the same bits"
    zero = _call(name, self_model=dict(link_mask=np.zeros(32, np.uint32), n_extra=0, self_margin=0.0, max_distance=1.0))
    assert all(np.array_equal(zero[k], base[k]) for k in base), "an all-zero self mask returns the bytes of the plain call"
    cc_ = bc.case("carry")
    from carry_cases import case as carry_case
    n_arm = carry_case("under")["n_arm"]
    arm = dict(probes=cc_["probes"][:n_arm], links=cc_["links"][:n_arm], self_model=None)
    empty, plain = _call("carry", **arm), _call("carry", carry=None, **arm)
    assert (empty["status"] == 0).all() and all(np.array_equal(empty[k], plain[k]) for k in empty), "nothing on the carried body: the plain call's bytes"
    assert (plain["blend_len"][:, 1] > _call("carry")["blend_len"][:, 1]).all(), "the arm alone takes the full blend, with the cube the halved one"
    idx = np.arange(65) % B
    many = _call(name, rows=idx)
    assert many["points"].shape[0] == 65 and all(np.array_equal(many[k], base[k][idx]) for k in base), "R = 65 with repeated env indices"


def test_invisible_to_the_scene_and_refused_inside_a_step():
    from gym_genesis.backend.lib import MirError

    c, kw = _args("corner_at_post")
    sc = _scene("post")
    state, version = [x.clone() for x in sc.get_state()], sc.state_version
    launches = sc.__dict__.get("blend_launches", 0)
    out = sc.blend_path(poly=c["poly"], **kw)
    assert (out["status"] == 0).all() and sc.__dict__.get("blend_launches", 0) == launches + 1
    assert all(torch.equal(x, y) for x, y in zip(state, sc.get_state())) and sc.state_version == version
    with pytest.raises(MirError, match="mir_blend_path"):
        sc.blend_path(poly=c["poly"], **{**kw, "max_points": 1})
    with pytest.raises(MirError, match="mir_blend_path"):
        sc.blend_path(poly=c["poly"], **{**kw, "resolution": 0.0})   # what mir_path_clearance refuses
    none = sc.blend_path(poly=c["poly"][:0], env_idx=torch.zeros(0, dtype=torch.long), **kw)
    assert none["points"].shape == (0, 11, len(c["qadr"])) and sc.__dict__.get("blend_launches", 0) == launches + 1, "no rows: no launch"
    assert C.sizeof(S.MirBlendQuery) == sc.lib.mir_blend_query_sizeof()
    bufs = (sc.empty(sc.agent_dim), sc.empty(sc.env_dim), sc.empty(), sc.empty(dtype=torch.uint8))
    sc.step_begin(None, *bufs)
    try:
        with pytest.raises(MirError, match="mir_blend_path"):
            sc.blend_path(poly=c["poly"], **kw)
    finally:
        sc.step_end()
        sc.set_state(*state)
        torch.cuda.synchronize()
    assert sc.__dict__.get("blend_launches", 0) == launches + 1


def test_entity_view():
    """d. EntityView.blend_path: (W, R, n) in the entity's dof order, accepted by retime_path and get_path_clearance unchanged; the
    polyline of plan_path(return_detail=True) goes in as it comes out; an unbatched view has no env axis"""
    from gym_genesis.backend.lib import MirScene

    c, kw = _args("corner_at_post")
    sc = _scene("post")
    robot = pc.arm(c["sb"], sc)
    n = len(c["qadr"])
    raw = _call("corner_at_post")
    poly = torch.as_tensor(c["poly"], device=sc.device)
    off = dict(self_collision=False)
    det = robot.blend_path(poly, max_deviation=0.1, num_waypoints=W, return_detail=True, **off)
    assert det["path"].shape == (W, B, n) and np.array_equal(det["path"].permute(1, 0, 2).cpu().numpy(), raw["path"])
    assert det["valid"].all() and np.array_equal(det["blend_len"].cpu().numpy(), raw["blend_len"])
    dense = robot.blend_path(poly, max_deviation=0.1, **off)
    assert dense.shape == (S.blend_max_points(3, 8), B, n) and np.array_equal(dense.permute(1, 0, 2).cpu().numpy(), raw["points"])
    timed = robot.retime_path(dense, 1.5, 4.0, dt=0.01, return_detail=True)
    assert timed["valid"].all() and (timed["duration"] > 0).all(), timed["status"]
    clear = robot.get_path_clearance(dense, **off)
    assert clear.shape == (B,) and (clear >= 0.0).all(), clear   # (condition 4 of the CPU tier: the dense polyline keeps 0.5 mm)
    planned = robot.plan_path(torch.as_tensor(pc.case("post")["goal"], device=sc.device), num_waypoints=16, max_nodes=128, max_iterations=512,
                              return_detail=True, **off)
    smooth = robot.blend_path(planned["poly"], planned["n_poly"], return_detail=True, **off)
    assert smooth["valid"].all() and smooth["path"].shape[1:] == (B, n)
    assert torch.equal(smooth["path"][0], planned["path"][0]) and torch.equal(smooth["path"][-1], planned["path"][-1])
    # accepted unchanged; its value is printed, not bounded: the blends were checked as curves at samples <= resolution apart per joint,
    # get_path_clearance samples the chords, and between two samples a clearance is as coarse as the planner's edge rule
    low = robot.get_path_clearance(smooth["path"], **off)
    print(f"\n[blend, planned] plan statuses {planned['status'].cpu().numpy()}, nodes {planned['n_poly'].cpu().numpy()}, blended "
          f"{smooth['stats'][:, 1].cpu().numpy()}, sharp {smooth['stats'][:, 2].cpu().numpy()}, clearance {low.cpu().numpy().round(4)}")
    assert low.shape == (B,) and torch.isfinite(low).all()
    assert (smooth["stats"][:, 0] == planned["n_poly"]).all()
    one = MirScene(c["spec"], 1)
    one.set_state(qpos=c["q"][:1], qvel=np.zeros((1, one.nv), np.float32))
    single = pc.arm(c["sb"], one)
    single.unbatched = True
    d1 = single.blend_path(poly[0], max_deviation=0.1, num_waypoints=W, return_detail=True, **off)
    assert d1["path"].shape == (W, n) and d1["valid"].dim() == 0 and d1["blend_len"].shape == (128,) and d1["points"].shape == (11, n)
    assert np.array_equal(d1["path"].cpu().numpy(), raw["path"][0])
    one.close()


def test_the_example_runs(monkeypatch):
    """examples/franka/plan_blend_retime_follow.py at 8 envs: both ways are timed on every env, and the blended targets' largest second
    difference over amax dt^2 (the median over the envs) is below the polyline's at the same waypoint count -- what the CPU tier
    asserts of the float64 reference, here through the three kernels"""
    import importlib.util
    import os
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("plan_blend_retime_follow", os.path.join(root, "examples", "franka", "plan_blend_retime_follow.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(sys, "argv", ["plan_blend_retime_follow.py", "--num-envs", "8", "--waypoints", "200"])
    res = mod.main()
    print(f"\n[blend, example] {res}")
    assert res["polyline"]["timed"] == 8 and res["blended"]["timed"] == 8
    assert res["blended"]["second"] < res["polyline"]["second"], res
