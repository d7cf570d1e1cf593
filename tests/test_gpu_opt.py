"""Batched trajectory optimisation on the GPU (include/mirigid.h: mir_optimize_path; backend/lib.py: MirScene.optimize_path;
tasks/views.py: EntityView.optimize_path).

The cases -- scenes, start rows, seeds, sphere model, parameters -- are those of tests/opt_cases.py; tests/test_opt_cpu.py holds the
conditions that make the comparisons below fair.  States are SET.  B = 5, and all five rows are judged in every case.

1. grad0 and cost[:, :2] at the input against the float64 reference: what catches a wrong Jacobian, normal frame, chain mask,
   reduction or weight.
2. The path after the case's iterations against the float64 reference; status, stop and every entry of stats are equal (condition 3 of
   the CPU tier makes that fair).
3. Properties in the device's own arithmetic, exact: the ends' bits, the limits, U no higher than at the input, an OK row passes
   get_path_clearance of the same arguments, every other row returns its input; ignore is the smoothness arithmetic alone and
   checks nothing; env_idx subsets and permutations, repeated calls, the state untouched.
4. thin; 5. the instantiations with SELF and CARRY; the entity view.
Yardstick, the project's rule (tests/test_gpu_blend.py): tol = 4 x max(error of the float32 port against float64 on the same row,
2^-23 x the largest magnitude in the compared array), printed before it is used.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import opt_cases as oc
import opt_ref
import plan_cases as pc
from gym_genesis.backend import spec as S

pytestmark = pytest.mark.gpu

B = oc.B
_scenes = {}


def _scene(name):
    if name not in _scenes:
        from gym_genesis.backend.lib import MirScene

        c = oc.case({"under": "carry", "thin": "thin", "post": "over_post", "post_free": "free"}[name])
        sc = MirScene(c["spec"], B)
        sc.set_state(qpos=c["q"], qvel=np.zeros((B, sc.nv), np.float32))
        _scenes[name] = sc
    return _scenes[name]


def _scene_of(name):
    c = oc.case(name)
    if c["scene"] in ("under", "thin"):
        return _scene(c["scene"])
    return _scene("post" if name in oc.COLLISION_CASES else "post_free")   # (the collision cases hold row 0's state on every row)


def _args(name):
    c = oc.case(name)
    kw = dict(probes=c["probes"], links=c["links"], dof_qadr=c["qadr"], skip_geoms=c["skip"], resolution=oc.RESOLUTION, margin=c["margin"],
              ignore_collision=c["ignore"], grad0=True, **c["par"])
    if c["mask"] is not None:
        kw["self_model"] = dict(link_mask=c["mask"], n_extra=c["n_extra"], self_margin=0.0, max_distance=1.0)
    if c["carry"] is not None:
        kw["carry"] = dict(body=c["carry"][0], link=c["carry"][1])
    return c, kw


def _call(name, rows=None, **over):
    """the case through MirScene.optimize_path (rows: env indices, the seeds of those rows) -> numpy arrays"""
    c, kw = _args(name)
    sc = _scene_of(name)
    kw.update(over)
    paths = c["paths"]
    if rows is not None:
        rows = np.asarray(rows)
        paths = paths[rows]
        kw["env_idx"] = torch.as_tensor(rows, device=sc.device)
    return {k: v.cpu().numpy() for k, v in sc.optimize_path(paths=paths, **kw).items()}


def _tol(name, r, key, sl=slice(None)):
    """the yardstick of one array of one row: 4 x max(float32 port against float64, 2^-23 x the largest magnitude)"""
    a, b = oc.reference(name, r, "float64"), oc.reference(name, r, "float32")
    x, y = np.asarray(a[key], np.float64)[sl], np.asarray(b[key], np.float64)[sl]
    L = float(np.abs(x).max())
    err = float(np.abs(x - y).max())
    return 4.0 * max(err, 2.0 ** -23 * L), err, L


@pytest.mark.parametrize("name", oc.NAMES)
def test_against_the_reference(name):
    """1. and 2. on every row"""
    got = _call(name)
    for r in range(B):
        ref = oc.reference(name, r)
        assert int(got["status"][r]) == ref["status"], (name, r, got["status"][r], ref["status"], got["stats"][r])
        assert [int(v) for v in got["stats"][r]] == [int(v) for v in ref["stats"]], (name, r, got["stats"][r], ref["stats"])
        if ref["stop"] == opt_ref.STOP_NONE:   # (a failed check: nothing was evaluated)
            assert not got["grad0"][r].any() and not got["cost"][r].any() and np.isinf(got["min_d"][r])
            assert got["path"][r].tobytes() == oc.case(name)["paths"][r].tobytes()
            continue
        tg, pg, Lg = _tol(name, r, "grad0")
        eg = float(np.abs(got["grad0"][r].astype(np.float64) - np.asarray(ref["grad0"], np.float64)).max())
        tc, pcst, Lc = _tol(name, r, "cost", slice(0, 2))
        ec = float(np.abs(got["cost"][r, :2].astype(np.float64) - np.asarray(ref["cost"][:2], np.float64)).max())
        tp, pp, Lp = _tol(name, r, "path")
        ep = float(np.abs(got["path"][r].astype(np.float64) - np.asarray(ref["path"], np.float64)).max())
        tr, pr, Lr = _tol(name, r, "cost", slice(2, 4))
        er = float(np.abs(got["cost"][r, 2:].astype(np.float64) - np.asarray(ref["cost"][2:], np.float64)).max())
        print(f"[opt, {name}] row {r}: grad0 {eg:.3e} (tol {tg:.3e}: port {pg:.3e}, L {Lg:.3f}); cost at the input {ec:.3e} (tol {tc:.3e}: port {pcst:.3e}, "
              f"L {Lc:.4f}); path {ep:.3e} (tol {tp:.3e}: port {pp:.3e}, L {Lp:.3f}); cost reached {er:.3e} (tol {tr:.3e}: port {pr:.3e})")
        assert eg <= tg, (name, r, eg, tg)
        assert ec <= tc, (name, r, ec, tc)
        assert ep <= tp, (name, r, ep, tp)
        assert er <= tr, (name, r, er, tr)
        assert not got["grad0"][r, 0].any() and not got["grad0"][r, -1].any(), "zero rows at the ends"
        if np.isfinite(float(ref["min_d"])):
            tm = 4.0 * max(abs(float(oc.reference(name, r, "float32")["min_d"]) - float(ref["min_d"])), 2.0 ** -23 * 1.0)
            assert abs(float(got["min_d"][r]) - float(ref["min_d"])) <= tm, (name, r, got["min_d"][r], ref["min_d"], tm)


@pytest.mark.parametrize("name", oc.NAMES)
def test_properties_in_the_devices_own_arithmetic(name):
    """3. on every row"""
    c, kw = _args(name)
    sc = _scene_of(name)
    got = _call(name)
    lo, hi = (np.asarray(v, np.float32) for v in (oc.problem(name, np.float32).lo, oc.problem(name, np.float32).hi))
    wo = 0.0 if c["ignore"] else c["par"]["obstacle_weight"]
    clear_kw = {k: kw[k] for k in ("probes", "links", "dof_qadr", "skip_geoms", "resolution", "margin") if k in kw}
    clear_kw.update({k: kw[k] for k in ("self_model", "carry") if k in kw})
    swept = {k: v.cpu().numpy() for k, v in sc.path_clearance(paths=np.where(np.isfinite(got["path"]), got["path"], 0.0), **clear_kw).items()}
    for r in range(B):
        inp, out, status = c["paths"][r], got["path"][r], int(got["status"][r])
        assert out[0].tobytes() == inp[0].tobytes() and out[-1].tobytes() == inp[-1].tobytes(), "the end waypoints keep their input bits"
        if status != 0:
            assert out.tobytes() == inp.tobytes(), (name, r, status, "a row that is not OK returns its input bit for bit")
            continue
        assert ((out[1:-1] >= lo) & (out[1:-1] <= hi)).all(), (name, r, "interior waypoints lie within the limits")
        U0 = np.float32(np.float32(c["par"]["smooth_weight"]) * got["cost"][r, 0]) + np.float32(np.float32(wo) * got["cost"][r, 1])
        U1 = np.float32(np.float32(c["par"]["smooth_weight"]) * got["cost"][r, 2]) + np.float32(np.float32(wo) * got["cost"][r, 3])
        assert U1 <= U0, (name, r, U1, U0)
        if not c["ignore"]:
            assert int(swept["row_first_blocked"][r]) == -1, (name, r, swept["row_first_blocked"][r], swept["row_min"][r])
    again = _call(name)
    assert all(got[k].tobytes() == again[k].tobytes() for k in got), "a second identical call returns identical bits"


def test_ignore_is_the_smoothness_arithmetic_and_checks_nothing():
    """MIR_PLAN_IGNORE_COLLISION: the descent of w_o = 0 on the same bits, nothing evaluated, nothing swept.  Far from everything (free)
    the two calls return the same path; over the post the smoothed path cuts through it: the call with w_o = 0 reaches the same S,
    is swept, BLOCKED and returns its input, the ignoring call returns what it reached"""
    ig, zero = _call("free", ignore_collision=True), _call("free", obstacle_weight=0.0)
    assert (ig["status"] == 0).all() and (zero["status"] == 0).all()
    assert ig["path"].tobytes() == zero["path"].tobytes() and ig["grad0"].tobytes() == zero["grad0"].tobytes()
    assert (ig["stats"][:, [0, 1, 2, 5]] == zero["stats"][:, [0, 1, 2, 5]]).all()
    ig, zero = _call("ignore"), _call("over_post", obstacle_weight=0.0)
    assert (ig["status"] == 0).all() and not ig["stats"][:, 3].any() and not ig["stats"][:, 4].any() and not ig["cost"][:, [1, 3]].any()
    assert ig["grad0"].tobytes() == zero["grad0"].tobytes() and ig["cost"][:, 2].tobytes() == zero["cost"][:, 2].tobytes()
    assert (zero["status"] == opt_ref.BLOCKED).all() and zero["path"].tobytes() == oc.case("over_post")["paths"].tobytes()
    assert (zero["stats"][:, 3] > 0).all() and (zero["stats"][:, 4] > 0).all() and (zero["cost"][:, 3] > zero["cost"][:, 1]).all()
    assert ig["path"].tobytes() != _call("over_post")["path"].tobytes(), "the obstacle term moves the path"


def test_line_is_straight():
    got = _call("line")
    P = got["path"].astype(np.float64)
    K = P.shape[1]
    want = P[:, :1] + (np.arange(K) / (K - 1))[None, :, None] * (P[:, -1:] - P[:, :1])
    assert (got["status"] == 0).all() and np.abs(P - want).max() <= 4e-6, np.abs(P - want).max()


def test_addressing_and_equivalence():
    name = "over_post"
    base = _call(name)
    perm = np.array([3, 0, 4, 1])
    got = _call(name, rows=perm)
    assert all(got[k].tobytes() == base[k][perm].tobytes() for k in base), "an env_idx permutation of a subset equals the matching rows of the full call"
    for r in (0, 4):
        one = _call(name, rows=[r])
        assert all(one[k][0].tobytes() == base[k][r].tobytes() for k in base), "one launch of R rows equals R launches of one row"
    c = oc.case(name)
    rows = _call(name, qpos_start=c["q"])
    assert all(rows[k].tobytes() == base[k].tobytes() for k in base), "qpos_start rows equal to the state give the same bits"
    idx = np.arange(65) % B
    many = _call(name, rows=idx)
    assert many["path"].shape[0] == 65 and all(many[k].tobytes() == base[k][idx].tobytes() for k in base), "R = 65 with repeated env indices"
    none = _call(name, grad0=False)
    assert "grad0" not in none and all(none[k].tobytes() == base[k].tobytes() for k in none), "the test hook changes nothing else"


@pytest.mark.parametrize("K", (3, 128))
def test_the_smallest_and_the_largest_path(K):
    """K = 3 (one interior waypoint: the recurrence is one step) and K = MIR_PLAN_MAX_POLY with the self model (the largest buffers, the
    sphere list behind them), far from everything, one iteration: row 0 against the float64 reference under the yardstick, every row
    by the properties"""
    c, so = oc.case("free"), oc.case("self_on")
    sc = _scene_of("free")
    paths = oc._seed(c["q"][:, c["qadr"]], oc.FREE, K, False)
    par = dict(oc.PAR, max_iterations=1)
    model = dict(link_mask=so["mask"], n_extra=so["n_extra"], self_margin=0.0, max_distance=1.0)
    got = {k: v.cpu().numpy() for k, v in sc.optimize_path(probes=so["probes"], links=so["links"], dof_qadr=c["qadr"], paths=paths, skip_geoms=c["skip"],
                                                           resolution=oc.RESOLUTION, margin=0.0, self_model=model, grad0=True, **par).items()}
    assert (got["status"] == 0).all() and (got["stats"][:, :2] == 1).all() and (got["stats"][:, 3] == 2 * (K - 2)).all(), got["stats"]
    assert (got["cost"][:, 2] < got["cost"][:, 0]).all() and not got["cost"][:, [1, 3]].any()
    assert got["path"][:, [0, -1]].tobytes() == paths[:, [0, -1]].tobytes()
    import self_ref
    ref = []
    for dt in (np.float64, np.float32):
        pb = self_ref.SelfProblem(c["spec"], so["probes"], so["links"], c["qadr"], so["n_extra"], so["mask"], c["skip"], 1.0, 0.0, 1.0, dt)
        ref.append(opt_ref.optimize(pb, c["q"][0], paths[0], margin=0.0, resolution=oc.RESOLUTION, **par))
    a, b = ref
    assert [int(v) for v in got["stats"][0]] == [int(v) for v in a["stats"]] == [int(v) for v in b["stats"]], (got["stats"][0], a["stats"], b["stats"])
    for key in ("path", "grad0"):
        x, y = np.asarray(a[key], np.float64), np.asarray(b[key], np.float64)
        tol = 4.0 * max(float(np.abs(x - y).max()), 2.0 ** -23 * float(np.abs(x).max()))
        err = float(np.abs(got[key][0].astype(np.float64) - x).max())
        print(f"[opt, K = {K}] row 0 {key}: {err:.3e} (tol {tol:.3e})")
        assert err <= tol, (K, key, err, tol)


def test_thin_blocks_and_the_input_comes_back():
    """4."""
    c = oc.case("thin")
    got = _call("thin")
    assert (got["status"] == opt_ref.BLOCKED).all() and got["path"].tobytes() == c["paths"].tobytes(), got["status"]
    assert (got["stats"][:, 1] > 0).all() and (got["cost"][:, 2] < got["cost"][:, 0]).all(), "the descent ran; the sweep refused what it reached"
    free = _call("thin", skip_geoms=c["skip"] | (1 << c["thin_geom"]))
    assert (free["status"] == 0).all() and free["path"].tobytes() != c["paths"].tobytes()
    for r in range(B):
        assert [int(v) for v in free["stats"][r]] == [int(v) for v in oc.reference("thin", r, skip_thin=True)["stats"]]


def test_self_and_carry_instantiations():
    """5."""
    base = _call("over_post")
    so = _call("self_on")
    assert [int(s) for s in so["status"]] == [oc.reference("self_on", r)["status"] for r in range(B)]
    assert so["path"].tobytes() == base["path"].tobytes() and (so["stats"][:, 4] == base["stats"][:, 4]).all(), "the self test is in the sweep only"
    zero = _call("over_post", self_model=dict(link_mask=np.zeros(32, np.uint32), n_extra=0, self_margin=0.0, max_distance=1.0))
    assert all(zero[k].tobytes() == base[k].tobytes() for k in base), "an all-zero self mask returns the bits of the plain call"
    # folded onto itself at both ends of a seed: clear of the scene, inside the arm's own spheres -> BLOCKED_SELF, the input comes back
    import blend_cases as bcs
    c = oc.case("self_on")
    folded = c["paths"].copy()
    folded[:, :, :7] = np.asarray(bcs.START_FOLDED, np.float32)
    folded[:, 1:-1, 0] += np.float32(0.01)
    sc = _scene_of("self_on")
    _, kw = _args("self_on")
    out = {k: v.cpu().numpy() for k, v in sc.optimize_path(paths=folded, **kw).items()}
    ref = opt_ref.optimize(oc.problem("self_on"), c["q"][0], folded[0], margin=c["margin"], resolution=oc.RESOLUTION, **c["par"])
    assert ref["status"] == opt_ref.BLOCKED_SELF and abs(ref["log"]["sweep"][-1][0]) >= 1e-3 and abs(ref["log"]["sweep"][-1][1]) >= 1e-3, ref["log"]["sweep"]
    assert (out["status"] == opt_ref.BLOCKED_SELF).all() and out["path"].tobytes() == folded.tobytes(), out["status"]
    ca = _call("carry")
    assert [int(s) for s in ca["status"]] == [oc.reference("carry", r)["status"] for r in range(B)]
    import carry_cases as cc
    cu, cc_ = cc.case("under"), oc.case("carry")
    n_arm = cu["n_arm"]
    arm = dict(probes=cc_["probes"][:n_arm], links=cc_["links"][:n_arm], self_model=None)
    empty, plain = _call("carry", **arm), _call("carry", carry=None, **arm)
    assert all(empty[k].tobytes() == plain[k].tobytes() for k in empty), "nothing on the carried body: the plain call's bits"
    assert ca["grad0"].tobytes() != plain["grad0"].tobytes(), "the cube's spheres are in the cost"


def test_invisible_to_the_scene_and_refused_inside_a_step():
    from gym_genesis.backend.lib import MirError

    c, kw = _args("over_post")
    sc = _scene_of("over_post")
    state, version = [x.clone() for x in sc.get_state()], sc.state_version
    launches = sc.__dict__.get("opt_launches", 0)
    out = sc.optimize_path(paths=c["paths"], **kw)
    assert (out["status"] == 0).all() and sc.__dict__.get("opt_launches", 0) == launches + 1
    assert all(torch.equal(x, y) for x, y in zip(state, sc.get_state())) and sc.state_version == version
    for bad, text in ((dict(step=0.0), "step must be > 0"), (dict(resolution=0.0), "resolution"), (dict(max_distance=0.04), "max_distance"),
                      (dict(smooth_weight=float("nan")), "not finite")):
        with pytest.raises(MirError, match="mir_optimize_path.*" + text):
            sc.optimize_path(paths=c["paths"], **{**kw, **bad})
    with pytest.raises(MirError, match="num_waypoints outside"):
        sc.optimize_path(paths=c["paths"][:, :2], **kw)
    none = sc.optimize_path(paths=c["paths"][:0], env_idx=torch.zeros(0, dtype=torch.long), **kw)
    assert none["path"].shape == (0, oc.K_OF["over_post"], len(c["qadr"])) and sc.__dict__.get("opt_launches", 0) == launches + 1, "no rows: no launch"
    assert C.sizeof(S.MirOptQuery) == sc.lib.mir_opt_query_sizeof()
    bufs = (sc.empty(sc.agent_dim), sc.empty(sc.env_dim), sc.empty(), sc.empty(dtype=torch.uint8))
    sc.step_begin(None, *bufs)
    try:
        with pytest.raises(MirError, match="mir_optimize_path"):
            sc.optimize_path(paths=c["paths"], **kw)
    finally:
        sc.step_end()
        sc.set_state(*state)
        torch.cuda.synchronize()


def test_entity_view():
    """EntityView.optimize_path: (W, R, n) in the entity's dof order, accepted by retime_path, get_path_clearance and certify_path unchanged;
    an unbatched view has no env axis; grasp_pose is refused"""
    from gym_genesis.backend.lib import MirScene

    c, kw = _args("over_post")
    sc = _scene_of("over_post")
    robot = pc.arm(c["sb"], sc)
    n = len(c["qadr"])
    raw = _call("over_post")
    path = torch.as_tensor(c["paths"], device=sc.device).permute(1, 0, 2).contiguous()
    par = {k: v for k, v in c["par"].items()}
    det = robot.optimize_path(path, return_detail=True, self_collision=False, **par)
    assert det["path"].shape == path.shape and np.array_equal(det["path"].permute(1, 0, 2).cpu().numpy(), raw["path"])
    assert det["valid"].all() and np.array_equal(det["stats"].cpu().numpy(), raw["stats"])
    out = robot.optimize_path(path, self_collision=False)   # the defaults
    assert out.shape == path.shape and torch.equal(out[0], path[0]) and torch.equal(out[-1], path[-1])
    timed = robot.retime_path(out, 1.5, 4.0, dt=0.01, return_detail=True)
    assert timed["valid"].all() and (timed["duration"] > 0).all(), timed["status"]
    clear = robot.get_path_clearance(out, self_collision=False)
    assert clear.shape == (B,) and (clear >= 0.0).all(), clear
    cert = robot.certify_path(out)
    print(f"\n[opt, entity] defaults: clearance {clear.cpu().numpy().round(4)} (the seed's {robot.get_path_clearance(path, self_collision=False).cpu().numpy().round(4)}), "
          f"certify_path {cert.cpu().numpy()}")
    assert cert.shape == (B,)
    with pytest.raises(NotImplementedError, match="grasp_pose"):
        robot.optimize_path(path, grasp_pose=torch.zeros(B, 7))
    one = MirScene(c["spec"], 1)
    one.set_state(qpos=c["q"][:1], qvel=np.zeros((1, one.nv), np.float32))
    single = pc.arm(c["sb"], one)
    single.unbatched = True
    d1 = single.optimize_path(path[:, 0], return_detail=True, self_collision=False, **par)
    assert d1["path"].shape == (path.shape[0], n) and d1["valid"].dim() == 0 and d1["cost"].shape == (4,) and d1["stats"].shape == (6,)
    assert np.array_equal(d1["path"].cpu().numpy(), raw["path"][0])
    one.close()
