"""Batched straight-line end-effector paths on the GPU (include/mirigid.h: mir_cartesian_path; backend/lib.py: MirScene.cartesian_path;
tasks/views.py: EntityView.plan_cartesian_path).

The cases -- scenes, start rows, targets, sphere model -- are those of tests/cart_cases.py; tests/test_cart_cpu.py holds the conditions
that make the comparisons below fair.  States are SET.  B = 5, and all five rows are judged in every case.

a. Judged on its own output, the float64 reference as judge: every returned point puts the link within pos_tol / rot_tol (plus the
   yardstick) of the interpolated target of its sample; consecutive points differ by <= jump_threshold plus two roundings of q; the
   polyline of the points keeps the margin; points lie inside the limits; the columns that do not move carry the start's bits; the tail
   repeats the last accepted point; fraction = (n_points - 1) / S to one rounding; path = the float64 index resampler of the GPU's own
   points.
b. Against the reference: status, S and n_points are equal (conditions 1 - 3 of the CPU tier); in down_side and turn q matches the
   float64 reference at every sample (condition 4).
c. Yardstick, the project's rule: tol = 4 x max(error of the float32 port against float64 on the same samples, 2^-23 x L), printed
   before it is used.  L: the largest absolute coordinate for poses and clearances, max |q| for configurations.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import cart_cases as cs
import cart_ref
import plan_ref
from gym_genesis.backend import spec as S

pytestmark = pytest.mark.gpu

B, W = cs.B, 16
POS_TOL, ROT_TOL = cart_ref.IK_DEFAULTS["pos_tol"], cart_ref.IK_DEFAULTS["rot_tol"]
_scenes = {}


def _scene(name):
    if name not in _scenes:
        from gym_genesis.backend.lib import MirScene

        c = cs.case("carry_lift" if name == "under" else "down_side")
        sc = MirScene(c["spec"], B)
        sc.set_state(qpos=c["q"], qvel=np.zeros((B, sc.nv), np.float32))
        _scenes[name] = sc
    return _scenes[name]


def _args(name):
    c = cs.case(name)
    kw = dict(probes=c["probes"], links=c["links"], dof_qadr=c["qadr"], link_body=c["link"], skip_geoms=c["skip"], resolution=cs.RESOLUTION,
              margin=cs.MARGIN, num_waypoints=W, **c["par"])
    if c["mask"] is not None:
        kw["self_model"] = dict(link_mask=c["mask"], n_extra=c["n_extra"], self_margin=0.0, max_distance=1.0)
    if c["carry"] is not None:
        kw["carry"] = dict(body=c["carry"][0], link=c["carry"][1])
    return c, kw


def _call(name, rows=None, raw=False, **over):
    """the case through MirScene.cartesian_path (rows: env indices, the targets of those rows) -> numpy arrays"""
    c, kw = _args(name)
    sc = _scene(c["scene"])
    kw.update(over)
    tp, tq = c["tpos"], c["tquat"]
    if rows is not None:
        rows = np.asarray(rows)
        tp, tq = tp[rows], None if tq is None else tq[rows]
        kw["env_idx"] = torch.as_tensor(rows, device=sc.device)
    out = sc.cartesian_path(target_pos=tp, target_quat=tq, **kw)
    return out if raw else {k: v.cpu().numpy() for k, v in out.items()}


def _fk_tol(name, row, pts):
    """the yardstick of a pose: 4 x max(float32 forward kinematics against float64 at these configurations, 2^-23 L)"""
    c = cs.case(name)
    p64 = plan_ref.Problem(c["spec"], c["probes"][:1], c["links"][:1], c["qadr"], c["skip"], 1.0, np.float64)
    p32 = plan_ref.Problem(c["spec"], c["probes"][:1], c["links"][:1], c["qadr"], c["skip"], 1.0, np.float32)
    c64, c32 = cart_ref.Chain(p64, c["link"], c["spec"]), cart_ref.Chain(p32, c["link"], c["spec"])
    p64.set_row(c["q"][row])
    p32.set_row(c["q"][row])
    ep = er = L = 0.0
    for q in pts:
        (a, qa), (b, qb) = c64.pose(q), c32.pose(np.asarray(q, np.float32))
        ep = max(ep, float(np.linalg.norm(b.astype(np.float64) - a)))
        er = max(er, float(np.linalg.norm(cart_ref.rot_error(qb.astype(np.float64), qa, np.float64))))
        L = max(L, float(np.abs(a).max()))
    return 4.0 * max(ep, 2.0 ** -23 * L), 4.0 * max(er, 2.0 ** -23 * np.pi), ep, er, L


def _clear_tol(name, row, samples):
    """4 x max(float32 port against float64 on these configurations, 2^-23 L) for a clearance (the rule of tests/test_gpu_plan.py)"""
    c = cs.case(name)
    p64, p32 = cs.problem(name), cs.problem(name, np.float32)
    p64.set_row(c["q"][row])
    p32.set_row(c["q"][row])
    err, L = 0.0, 0.0
    for q in samples:
        c64, c32 = p64.clearance(q), p32.clearance(np.asarray(q, np.float32))
        if np.isfinite(float(c64)) and np.isfinite(float(c32)):
            err = max(err, abs(float(c32) - float(c64)))
        L = max(L, float(np.abs(p64.centres(q)).max()))
    return 4.0 * max(err, 2.0 ** -23 * L), err, L


def _judge(name, got, rows=None):
    """a. on every row of a result"""
    c = cs.case(name)
    lim = plan_ref.Problem(c["spec"], c["probes"][:1], c["links"][:1], c["qadr"], c["skip"], 1.0, np.float32)
    userot = c["tquat"] is not None
    jump, P = c["par"]["jump_threshold"], c["par"]["max_points"]
    for k in range(len(got["status"])):
        r = k if rows is None else int(rows[k])
        n, S_ = int(got["n_points"][k]), int(got["stats"][k, 2])
        pts = got["points"][k].astype(np.float64)
        start = c["q"][r][c["qadr"]]
        assert 1 <= n <= P and np.array_equal(got["points"][k, 0], start), "points[0] holds the start's bits"
        assert (got["points"][k, n:] == got["points"][k, n - 1]).all(), "the tail repeats the last accepted point's bits"
        assert (got["points"][k, :, 7:] == start[7:]).all(), "the fingers carry the start's bits"
        assert (got["points"][k] >= lim.lo).all() and (got["points"][k] <= lim.hi).all(), "inside the joint limits"
        Q = float(np.abs(pts).max())
        steps = np.abs(np.diff(pts[:n], axis=0)).max() if n > 1 else 0.0
        assert steps <= jump + 2.0 * 2.0 ** -23 * Q, (name, r, steps)
        want = np.float32(n - 1) / np.float32(S_) if n > 1 else np.float32(0)
        assert abs(float(got["fraction"][k]) - float(want)) <= 2.0 ** -23 * float(want), (name, r, got["fraction"][k], want)
        if got["status"][k] in (cart_ref.NOT_FINITE, cart_ref.TOO_MANY_POINTS):
            assert n == 1
            continue
        # straightness: the link's float64 pose at the GPU's q against the interpolated target of that sample
        ref = cs.reference(name, r)
        tol_p, tol_r, ep, er, L = _fk_tol(name, r, pts[:n])
        worst_p = worst_r = 0.0
        for a in range(1, n):
            p, q = cs.link_pose(name, r, pts[a])
            tp, tq = ref["targets"][a - 1]
            worst_p = max(worst_p, float(np.linalg.norm(p - tp)))
            if userot:
                worst_r = max(worst_r, float(np.linalg.norm(cart_ref.rot_error(tq, q, np.float64))))
        print(f"[cart, {name}] row {r}: n_points {n} of S {S_}; off the line {worst_p:.3e} m (pos_tol + {tol_p:.3e}: port {ep:.3e}, L {L:.3f}), "
              f"{worst_r:.3e} rad (rot_tol + {tol_r:.3e}: port {er:.3e}); largest joint step {steps:.4f}")
        assert worst_p <= POS_TOL + tol_p and worst_r <= ROT_TOL + tol_r, (name, r, worst_p, worst_r)
        if n > 1:
            seg, samples = plan_ref.polyline_clearance(cs.problem(name), c["q"][r], pts[:n], cs.RESOLUTION)
            tol, err, L = _clear_tol(name, r, samples)
            print(f"[cart, {name}] row {r}: lowest clearance of the points {seg.min():.5f} (tol {tol:.3e}: port {err:.3e}, L {L:.3f})")
            assert seg.min() >= cs.MARGIN - tol, (name, r, seg.min(), tol)
        if "path" in got:
            r64, r32 = cart_ref.resample(pts[:n], W, np.float64), cart_ref.resample(pts[:n], W, np.float32)
            port_q = float(np.abs(r32.astype(np.float64) - r64).max())
            tol_q = 4.0 * max(port_q, 2.0 ** -23 * Q)
            err_q = float(np.abs(got["path"][k] - r64).max())
            print(f"[cart, {name}] row {r}: waypoints against the float64 resampler {err_q:.3e} (tol_q {tol_q:.3e}: port {port_q:.3e}, Q {Q:.3f})")
            assert err_q <= tol_q, (name, r, err_q, tol_q)
            assert np.array_equal(got["path"][k, 0], got["points"][k, 0]) and np.array_equal(got["path"][k, -1], got["points"][k, n - 1])


def _against_reference(name, got, q_too=False):
    """b. status, S and n_points; with q_too the configurations point by point"""
    for r in range(B):
        ref = cs.reference(name, r)
        assert int(got["status"][r]) == ref["status"], (name, r, got["status"][r], ref["status"], got["stats"][r])
        if ref["status"] == cart_ref.NOT_FINITE:
            continue
        assert int(got["stats"][r, 2]) == ref["S"], (name, r, got["stats"][r], ref["S"])
        slack = 0
        if name == "out_of_reach":
            from test_cart_cpu import out_of_reach_same_sample
            slack = 0 if out_of_reach_same_sample() else 1   # (condition 3: where reference and port disagree, one sample either way)
            print(f"[cart, out_of_reach] row {r}: n_points GPU {int(got['n_points'][r])} reference {ref['n_points']} (allowed +-{slack})")
        assert abs(int(got["n_points"][r]) - ref["n_points"]) <= slack, (name, r, got["n_points"][r], ref["n_points"])
        assert int(got["stats"][r, 3]) == ref["failed_segment"]
        if q_too:
            port = cs.reference(name, r, "float32")
            n = ref["n_points"]
            Q = float(np.abs(ref["points"]).max())
            perr = float(np.abs(port["points"].astype(np.float64) - ref["points"]).max())
            tol = 4.0 * max(perr, 2.0 ** -23 * Q)
            err = float(np.abs(got["points"][r, :n].astype(np.float64) - ref["points"]).max())
            print(f"[cart, {name}] row {r}: q against the float64 reference over {n} points {err:.3e} (tol {tol:.3e}: port {perr:.3e}, Q {Q:.3f}); "
                  f"IK iterations GPU {int(got['stats'][r, 0])} reference {sum(ref['iters'])}")
            assert err <= tol, (name, r, err, tol)


@pytest.mark.parametrize("name", ("down_side", "turn", "position_only"))
def test_lines_are_followed(name):
    got = _call(name)
    assert (got["status"] == 0).all() and (got["fraction"] == 1.0).all(), (got["status"], got["stats"])
    _judge(name, got)
    _against_reference(name, got, q_too=name in ("down_side", "turn"))


@pytest.mark.parametrize("name", ("through_post", "out_of_reach"))
def test_rows_keep_what_they_achieved(name):
    got = _call(name)
    assert ((got["fraction"] > 0) & (got["fraction"] < 1)).all(), got["fraction"]
    _judge(name, got)
    _against_reference(name, got)


def test_statuses():
    """jump, too_long and not_finite: the statuses that move nothing, the last one beside ordinary rows"""
    for name in ("jump", "too_long", "not_finite"):
        got = _call(name)
        _judge(name, got)
        _against_reference(name, got)
        moved = got["n_points"] > 1
        if name == "not_finite":
            assert list(moved) == [True, True, False, True, True] and got["fraction"][2] == 0 and (got["fraction"][moved] == 1).all()
        else:
            assert not moved.any() and (got["fraction"] == 0).all()
            assert (got["stats"][:, 3] == (0 if name == "jump" else -1)).all()   # the first sample of segment 0 jumps


def test_self_collision():
    """self_on: the SELF instantiation on a line that is clear gives the points of the call without it; self_fold: BLOCKED_SELF"""
    on, off = _call("self_on"), _call("down_side")
    assert (on["status"] == 0).all() and np.array_equal(on["points"], off["points"]) and np.array_equal(on["path"], off["path"])
    assert (on["stats"][:, 1] == off["stats"][:, 1]).all() and (on["stats"][:, 1] > 0).all()
    _against_reference("self_on", on)
    fold = _call("self_fold")
    assert (fold["status"] == cart_ref.BLOCKED_SELF).all(), fold["status"]
    _judge("self_fold", fold)
    _against_reference("self_fold", fold)


def test_carried_cube():
    """carry_empty: nothing rides on the carried body: the bytes of the call without cq.  carry_lift: blocked, and by the cube's spheres:
    the same call without the carried body (its spheres and the query left out) is clear"""
    c, kw = _args("carry_empty")
    empty = _call("carry_empty")
    plain = _call("carry_empty", carry=None)
    assert (empty["status"] == 0).all() and all(np.array_equal(empty[k], plain[k]) for k in empty), "an empty carry changes nothing"
    lift = _call("carry_lift")
    assert (lift["status"] == cart_ref.BLOCKED).all(), (lift["status"], lift["stats"])
    _judge("carry_lift", lift)
    _against_reference("carry_lift", lift)
    cl = cs.case("carry_lift")
    out = _scene("under").cartesian_path(c["probes"], c["links"], c["qadr"], c["link"], cl["tpos"], cl["tquat"], skip_geoms=c["skip"],
                                         resolution=cs.RESOLUTION, margin=cs.MARGIN, **cl["par"])
    assert (out["status"] == 0).all() and (out["fraction"] == 1).all(), "the arm's own spheres pass the post"


def test_addressing_and_determinism():
    name = "down_side"
    base, again = _call(name), _call(name)
    assert all(np.array_equal(base[k], again[k]) for k in base), "two identical calls give identical bits"
    perm = np.array([3, 0, 4, 2, 1])
    got = _call(name, rows=perm)
    assert all(np.array_equal(got[k], base[k][perm]) for k in base), "an env_idx permutation gives the permuted rows' bits"
    one = _call(name, rows=[3])
    assert all(np.array_equal(one[k][0], base[k][3]) for k in base), "a row computed alone equals the row inside the batch (R = 1)"
    c = cs.case(name)
    rows = _call(name, qpos_start=c["q"])
    assert all(np.array_equal(rows[k], base[k]) for k in base), "qpos_start rows equal to the state give the same bits"
    idx = np.arange(65) % B
    many = _call(name, rows=idx)
    assert many["points"].shape[0] == 65 and all(np.array_equal(many[k], base[k][idx]) for k in base), "R = 65 with repeated env indices"
    blocked = _call("through_post")
    mixed = _call("through_post", rows=[4, 4, 0])
    assert all(np.array_equal(mixed[k], blocked[k][[4, 4, 0]]) for k in blocked)


def test_invisible_to_the_scene():
    """qpos, qvel and the state version are unchanged by a call, and one step after a call gives the bits of the same step without it"""
    from gym_genesis.backend.lib import MirScene

    c = cs.case("down_side")
    scs = [MirScene(c["spec"], B) for _ in range(2)]
    for sc in scs:
        sc.set_state(qpos=c["q"], qvel=np.zeros((B, sc.nv), np.float32))
    _, kw = _args("down_side")
    state, version = [x.clone() for x in scs[0].get_state()], scs[0].state_version
    out = scs[0].cartesian_path(target_pos=c["tpos"], target_quat=c["tquat"], **kw)
    assert (out["status"] == 0).all()
    assert all(torch.equal(x, y) for x, y in zip(state, scs[0].get_state())) and scs[0].state_version == version
    for sc in scs:
        sc.step()
    assert all(torch.equal(x, y) for x, y in zip(scs[0].get_state(), scs[1].get_state())), "the step after a call is the step without it"
    for sc in scs:
        sc.close()


def test_one_sample_is_one_ik_solve():
    """K = 1 and steps so large that S = 1, collisions ignored: the one point against the float64 IK reference from the same seed"""
    c, kw = _args("down_side")
    sc = _scene("post")
    kw.update(max_pos_step=1.0, max_rot_step=4.0, ignore_collision=True, num_waypoints=0)
    tp, tq = c["tpos"][:, :1], c["tquat"][:, :1]
    got = {k: v.cpu().numpy() for k, v in sc.cartesian_path(target_pos=tp, target_quat=tq, **kw).items()}
    assert (got["status"] == 0).all() and (got["n_points"] == 2).all() and (got["stats"][:, 2] == 1).all() and (got["stats"][:, 1] == 0).all()
    assert sc.n_arm == len(c["qadr"])
    ikq = sc.inverse_kinematics(c["link"], np.ascontiguousarray(tp[:, 0]), np.ascontiguousarray(tq[:, 0]), init_qpos=c["q"][:, c["qadr"]]).cpu().numpy()
    for r in range(B):
        out = {}
        for dt in (np.float64, np.float32):
            pb = plan_ref.Problem(c["spec"], c["probes"][:1], c["links"][:1], c["qadr"], c["skip"], 1.0, dt)
            a0 = pb.set_row(c["q"][r])
            out[dt] = cart_ref.ik(cart_ref.Chain(pb, c["link"], c["spec"]), a0, tp[r, 0].astype(dt), tq[r, 0].astype(dt), {}, dt)
        ref, port = out[np.float64][0], out[np.float32][0].astype(np.float64)
        Q = float(np.abs(ref).max())
        perr = float(np.abs(port - ref).max())
        tol = 4.0 * max(perr, 2.0 ** -23 * Q)
        err = float(np.abs(got["points"][r, 1].astype(np.float64) - ref).max())
        same = np.array_equal(got["points"][r, 1, :7], ikq[r, :7])
        print(f"[cart, one sample] row {r}: q against the float64 IK {err:.3e} (tol {tol:.3e}: port {perr:.3e}, Q {Q:.3f}); iterations GPU "
              f"{int(got['stats'][r, 0])} reference {out[np.float64][3]}; bit-equal to inverse_kinematics_rows: {same}")
        assert int(got["stats"][r, 0]) == out[np.float64][3] and err <= tol, (r, err, tol)


def _raw(sc, q, pq, c, out, sq=None, cq=None, tp=None, present=None, opt=None):
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    qa = np.ascontiguousarray(c["qadr"], np.int32)
    lk = np.ascontiguousarray(c["links"], np.int32)
    rc_ = sc.lib.mir_cartesian_path(sc.h, None if q is None else C.byref(q), C.byref(pq), None if sq is None else C.byref(sq),
                                    None if cq is None else C.byref(cq), p(out["probes"]), lk.ctypes.data_as(C.c_void_p), qa.ctypes.data_as(C.c_void_p),
                                    None, B, None, p(tp), None, None if opt is None else C.byref(opt), p(out["points"]), p(out["n_points"]),
                                    p(out["fraction"]), p(out["status"]), None, None, None)
    return rc_, sc.lib.mir_last_error()


def test_refusals_launch_nothing():
    from gym_genesis.backend.lib import MirError

    c = cs.case("position_only")
    sc = _scene("post")
    sc.lib.mir_last_error.restype = C.c_char_p
    N, D, P = len(c["probes"]), len(c["qadr"]), 64
    out = {"probes": torch.as_tensor(c["probes"], device=sc.device), "points": torch.full((B, P, D), float("nan"), device=sc.device),
           "n_points": torch.full((B,), -7, dtype=torch.int32, device=sc.device), "fraction": torch.full((B,), float("nan"), device=sc.device),
           "status": torch.full((B,), -7, dtype=torch.int32, device=sc.device)}
    tp = torch.as_tensor(c["tpos"], device=sc.device)
    good = lambda **kw: S.make_cart_query(kw.pop("link", c["link"]), 2, P, **kw)  # noqa: E731
    pq = lambda **kw: S.make_plan_query(N, D, skip_geoms=c["skip"], **kw)  # noqa: E731
    launches, version = sc.__dict__.get("cart_launches", 0), sc.state_version
    assert _raw(sc, good(), pq(), c, out, tp=tp)[0] == 0 and torch.isfinite(out["points"]).all()
    out["points"].fill_(float("nan"))
    out["status"].fill_(-7)
    out["n_points"].fill_(-7)
    bad = [(_raw(sc, None, pq(), c, out, tp=tp), -1, b"null argument"), (_raw(sc, good(), pq(), c, out, tp=None), -1, b"null argument")]
    bad.append((_raw(sc, good(link=0), pq(), c, out, tp=tp), -1, b"link out of range"))
    bad.append((_raw(sc, good(link=c["spec"].nbody), pq(), c, out, tp=tp), -1, b"link out of range"))
    cube = c["sb"].body_index("cube")
    bad.append((_raw(sc, good(link=cube), pq(), c, out, tp=tp), -1, b"hangs off a free body"))
    bad.append((_raw(sc, good(link=1), pq(), c, out, tp=tp), -1, b"no moving joint"))   # (link0 is bolted: no joint above it)
    bad.append((_raw(sc, good(max_pos_step=0.0), pq(), c, out, tp=tp), -1, b"max_pos_step"))
    bad.append((_raw(sc, good(num_waypoints=1), pq(), c, out, tp=tp), -1, b"num_waypoints"))
    bad.append((_raw(sc, good(), pq(resolution=0.0), c, out, tp=tp), -1, b"resolution"))                  # what mir_path_clearance refuses
    q = pq(); q.struct_size -= 8
    bad.append((_raw(sc, good(), q, c, out, tp=tp), -1, b"sizeof(MirPlanQuery)"))
    sq = S.make_self_query(None); sq.struct_size += 4
    bad.append((_raw(sc, good(), pq(), c, out, sq=sq, tp=tp), -1, b"sizeof(MirSelfQuery)"))
    bad.append((_raw(sc, good(), pq(), c, out, cq=S.make_carry_query(1, c["link"]), tp=tp), -1, b"not a free-joint body"))
    bad.append((_raw(sc, good(), pq(), c, out, tp=tp, opt=S.MirIkOptions(0, 1, 0.05, 5e-4, 5e-3, 0.5)), -1, b"bad options"))
    torch.cuda.synchronize()
    for (rc_, msg), code, text in bad:
        assert rc_ == code and b"mir_cartesian_path" in msg and text in msg, (rc_, msg, text)
    assert torch.isnan(out["points"]).all() and (out["status"] == -7).all() and (out["n_points"] == -7).all(), "a refused call launches nothing"
    assert sc.state_version == version
    with pytest.raises(MirError):
        sc.cartesian_path(c["probes"], c["links"], c["qadr"], c["link"], c["tpos"], max_points=1, skip_geoms=c["skip"])
    assert sc.__dict__.get("cart_launches", 0) == launches
    none = sc.cartesian_path(c["probes"], c["links"], c["qadr"], c["link"], c["tpos"][:0], env_idx=torch.zeros(0, dtype=torch.long), skip_geoms=c["skip"])
    assert none["points"].shape == (0, 256, D) and sc.__dict__.get("cart_launches", 0) == launches, "no rows: no launch"
    assert C.sizeof(S.MirCartQuery) == sc.lib.mir_cart_query_sizeof()


def test_chain_on_the_pick_task():
    """g. plan_cartesian_path -> retime_path -> get_path_clearance through EntityView on 8 envs of the pick task"""
    from gym_genesis.env import GenesisEnv

    n = 8
    env = GenesisEnv(task="cube_pick", robot="franka", num_envs=n, enable_pixels=False)
    env.reset(seed=5)
    task = env._env
    robot, cube, mir = task.franka, task.cube, task._mir
    hand = robot.get_link("hand")
    p0, q0 = hand.get_pos().clone(), hand.get_quat().clone()
    target = p0 + torch.tensor([0.0, 0.0, -0.083], device=mir.device)
    state, version = [x.clone() for x in mir.get_state()], mir.state_version
    det = robot.plan_cartesian_path(hand, target, q0, ignore_entities=[cube], margin=0.002, return_detail=True)
    assert all(torch.equal(x, y) for x, y in zip(state, mir.get_state())) and mir.state_version == version
    assert det["valid"].all() and (det["fraction"] == 1).all() and (det["n_points"] == 10).all(), (det["status"], det["stats"])
    path = det["path"]
    assert path.shape == (256, n, 9) and torch.equal(path[0], robot.get_qpos())
    W_ = 12
    way, frac = robot.plan_cartesian_path(hand, target, q0, ignore_entities=[cube], margin=0.002, num_waypoints=W_, return_fraction=True)
    assert way.shape == (W_, n, 9) and (frac == 1).all() and torch.equal(way[0], path[0]) and torch.equal(way[-1], path[9])
    timed = robot.retime_path(path, 1.0, 4.0, return_detail=True)
    assert timed["valid"].all() and (timed["duration"] > 0).all() and torch.isfinite(timed["samples"]).all(), timed["status"]
    assert torch.equal(timed["samples"][0], path[0]) and torch.equal(timed["samples"][-1], path[-1])
    clear = robot.get_path_clearance(timed["samples"], ignore_entities=[cube])
    dense = robot.get_path_clearance(path[:10], ignore_entities=[cube])
    # the timed samples lie on the polyline of the points: between two checked configurations the clearance moves by at most the
    # probes' travel, bounded by the largest joint step times the arm's reach (1.2 m covers the Panda with its fingers)
    reach, step = 1.2, float((path[1:10] - path[:9]).abs().max())
    tol = reach * step * 7
    print(f"\n[cart, pick] clearance of the points {dense.cpu().numpy().round(4)}; of the timed samples {clear.cpu().numpy().round(4)}; "
          f"largest joint step {step:.4f} rad (tol {tol:.4f} m); durations {timed['duration'].cpu().numpy().round(3)} s")
    assert (dense >= 0.002).all() and (clear >= 0.002 - tol).all()


def test_the_example_runs(monkeypatch):
    """examples/franka/cartesian_approach.py at 8 envs: the hand's lateral deviation from the vertical during the planned descent is
    below pos_tol plus the sag of the joint interpolation between two samples.  The sag bound: between two accepted samples the joints
    move linearly by at most dq = the measured largest joint step; the hand's path in between deviates from the chord by at most
    (1 / 8) x (sum of the 7 joints' |dq|)^2 x reach (the second-order term of the forward kinematics; reach 1.2 m covers the Panda)."""
    import importlib.util
    import os
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("cartesian_approach", os.path.join(root, "examples", "franka", "cartesian_approach.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(sys, "argv", ["cartesian_approach.py", "--num-envs", "8"])
    res = mod.main()
    sag = 0.125 * (7.0 * res["largest_joint_step"]) ** 2 * 1.2
    print(f"\n[cart, example] fractions {res['fractions']}; planned lateral deviation {res['planned_deviation']:.3e} m (pos_tol {POS_TOL} + sag "
          f"{sag:.3e} from the measured joint step {res['largest_joint_step']:.4f} rad); followed {res['followed_deviation']:.3e} m")
    assert all(f == 1.0 for f in res["fractions"]["descent"]) and res["planned_deviation"] <= POS_TOL + sag
