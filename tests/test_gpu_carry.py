"""The carried object on the GPU (include/mirigid.h "carried object": mir_plan_path_carry, mir_path_clearance_carry; tasks/views.py: the
attached_entity= argument of plan_path / get_path_clearance / path_in_collision and get_carried_clearance).

The cases are those of tests/carry_cases.py ("under": the cube in the fingers hangs into a post the hand itself clears; "rod": a 30 cm
rod in the hand sweeps into the arm); tests/test_carry_cpu.py holds the conditions that make "every row finds a plan" fair.  States are
SET.  B = 5.

Yardstick (the rule of tests/test_gpu_plan.py and tests/test_gpu_self.py): tol = 4 x max(error of the float32 port of tests/carry_ref.py
against float64 on the same configurations, 2^-23 x L), L = the largest absolute world coordinate of a probe centre or value on those
configurations; tol_q the same for the resampler with Q = max |q|.  Both are printed before they are used.  The GPU's plans are judged
on their own by the float64 validator, never against the reference's plan.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import carry_cases as cc
import plan_cases as pc
import plan_ref
from carry_ref import self_ref
from gym_genesis.backend import spec as S
from gym_genesis.backend.spec import make_carry_query, make_plan_query, make_self_query

pytestmark = pytest.mark.gpu

B, W = cc.B, cc.BUDGET["W"]
_scenes = {}


def _scene(name):
    """one scene per case ("post": that of tests/plan_cases.py), at the case's start rows"""
    if name not in _scenes:
        from gym_genesis.backend.lib import MirScene

        c = pc.case(name) if name == "post" else cc.case(name)
        s = MirScene(c["spec"], B)
        s.set_state(qpos=c["q"], qvel=np.zeros((B, s.nv), np.float32))
        _scenes[name] = s
    return _scenes[name]


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _budget(c):
    return dict(num_waypoints=W, max_nodes=cc.BUDGET["max_nodes"], max_iterations=cc.BUDGET["max_iterations"], resolution=cc.RESOLUTION, step=cc.STEP,
                margin=cc.MARGIN, skip_geoms=c["skip"])


def _model(c, grasp=None, **kw):
    return dict(self_model=dict(link_mask=c["mask"], n_extra=c["n_extra"], **kw), carry=dict(body=c["body"], link=c["link"], grasp=grasp))


def _tol(name, row, samples, grasp=None):
    """4 x max(float32 port against float64 on these configurations -- both values --, 2^-23 L)"""
    c = cc.case(name)
    p64, p32 = cc.problem(name), cc.problem(name, np.float32)
    p64.grasp = p32.grasp = grasp
    p64.set_row(c["q"][row])
    p32.set_row(c["q"][row])
    err, L = 0.0, 0.0
    for q in samples:
        v64, v32 = p64.both(q), p32.both(np.asarray(q, np.float32))
        err = max(err, abs(float(v32[0]) - float(v64[0])), abs(float(v32[1]) - float(v64[1])))
        L = max(L, float(np.abs(p64.centres(q)).max()), abs(float(v64[0])), abs(float(v64[1])))
    return 4.0 * max(err, 2.0 ** -23 * L), err, L


def _straight(c):
    return np.stack([c["start"], c["goal"]], 1)


# ---------------------------------------------------------------- (a) the grasp each row used
@pytest.mark.parametrize("name", cc.NAMES)
def test_grasp_used(name):
    c, s = cc.case(name), _scene(name)
    kw = dict(resolution=cc.RESOLUTION, skip_geoms=c["skip"])
    got = _np(s.path_clearance(c["probes"], c["links"], c["qadr"], _straight(c), **kw, **_model(c)))["grasp"]
    given = np.concatenate([c["grasp"][:, :3], 3.0 * c["grasp"][:, 3:]], 1).astype(np.float32)   # (quaternions of norm 3)
    got_given = _np(s.path_clearance(c["probes"], c["links"], c["qadr"], _straight(c), **kw, **_model(c, torch.as_tensor(given, device=s.device))))
    plan = _np(s.plan_path(c["probes"], c["links"], c["qadr"], c["goal"], **_budget(c), **_model(c)))["grasp"]
    assert plan.tobytes() == got.tobytes(), "both entry points compute the same G"
    p64, p32 = cc.problem(name), cc.problem(name, np.float32)
    print()
    for r in range(B):
        for label, grasp, g in (("from the start row", None, got[r]), ("given", given[r], got_given["grasp"][r])):
            p64.grasp = p32.grasp = grasp
            p64.set_row(c["q"][r])
            p32.set_row(c["q"][r])
            G64, G32 = p64.grasp_used(), p32.grasp_used()
            L = max(1.0, float(np.abs(p64.xp[[c["link"], c["body"]]]).max()))   # (world coordinates of the two poses; a unit quaternion)
            port = float(np.abs(G32.astype(np.float64) - G64).max())
            tol = 4.0 * max(port, 2.0 ** -23 * L)
            err = float(np.abs(g - G64).max())
            print(f"[grasp, {name}] row {r}, {label}: against float64 {err:.3e} allowed {tol:.3e} (port {port:.3e}, L {L:.3f}); nominal {np.abs(G64 - c['grasp'][r]).max():.3e}")
            assert err <= tol, (name, r, label, err, tol)
        assert np.array_equal(got_given["grasp"][r, :3], given[r, :3]), "a given position is used as it is"
        assert abs(float(np.linalg.norm(got_given["grasp"][r, 3:].astype(np.float64))) - 1.0) <= 4 * 2.0 ** -23


# ---------------------------------------------------------------- (b) the swept check
@pytest.mark.parametrize("name", cc.NAMES)
def test_path_clearance(name):
    c, s = cc.case(name), _scene(name)
    kw = dict(resolution=cc.RESOLUTION, margin=cc.MARGIN, skip_geoms=c["skip"])
    K = 40
    poly = np.stack([plan_ref.resample(cc.reference(name, r)["poly"], K, np.float64) for r in range(B)]).astype(np.float32)
    print()
    for label, paths in (("straight edge", _straight(c)), (f"K = {K} polyline", poly)):
        got = _np(s.path_clearance(c["probes"], c["links"], c["qadr"], paths, **kw, **_model(c)))
        skipped = compared = 0
        for r in range(B):
            seg, seg_self, samples = self_ref.polyline_clearances(cc.problem(name), c["q"][r], paths[r].astype(np.float64), cc.RESOLUTION)
            tol, port, L = _tol(name, r, samples)
            e_scene, e_self = float(np.abs(got["seg_min"][r] - seg).max()), float(np.abs(got["seg_self_min"][r] - seg_self).max())
            print(f"[carry clearance, {name}, {label}] row {r}: seg_min {e_scene:.3e} seg_self_min {e_self:.3e} allowed {tol:.3e} (port {port:.3e}, L {L:.3f}); "
                  f"row_min {got['row_min'][r]:.5f} row_self_min {got['row_self_min'][r]:.5f} first blocked {got['row_first_blocked'][r]}")
            assert e_scene <= tol and e_self <= tol, (name, label, r, e_scene, e_self, tol)
            assert abs(float(got["row_min"][r]) - float(seg.min())) <= tol and abs(float(got["row_self_min"][r]) - float(seg_self.min())) <= tol
            assert got["row_min"][r] == got["seg_min"][r].min() and got["row_self_min"][r] == got["seg_self_min"][r].min()
            # the first blocked segment: equal wherever the deciding values are further than tol from their margins
            sure = (np.abs(seg - cc.MARGIN) > tol) & (np.abs(seg_self - cc.SELF_MARGIN) > tol)
            blocked = (seg < cc.MARGIN) | (seg_self < cc.SELF_MARGIN)
            first = int(np.flatnonzero(blocked)[0]) if blocked.any() else -1
            upto = len(seg) if first < 0 else first + 1
            skipped, compared = skipped + int((~sure[:upto]).sum()), compared + len(seg)
            if sure[:upto].all():
                assert int(got["row_first_blocked"][r]) == first, (name, label, r, got["row_first_blocked"][r], first)
        assert skipped <= 0.05 * compared, (skipped, compared)
        if label == "straight edge":
            alone = _np(s.path_clearance(c["probes"][:c["n_arm"]], c["links"][:c["n_arm"]], c["qadr"], paths, **kw))
            print(f"[carry clearance, {name}] straight edge, the arm alone: row_min {alone['row_min']}")
            if name == "under":
                assert (got["row_min"] < -0.01).all() and (alone["row_min"] >= 0.01).all() and (got["row_self_min"] >= 0.02).all()
            else:
                assert (got["row_self_min"] < -0.01).all() and (alone["row_min"] >= 0.02).all() and (got["row_min"] >= 0.02).all()
            assert (got["row_first_blocked"] == 0).all() and (alone["row_first_blocked"] == -1).all()


# ---------------------------------------------------------------- (c) planning with the object attached
@pytest.mark.parametrize("name", cc.NAMES)
def test_planning_with_the_object_attached(name):
    c, s = cc.case(name), _scene(name)
    got = _np(s.plan_path(c["probes"], c["links"], c["qadr"], c["goal"], **_budget(c), **_model(c)))
    assert (got["status"] == 0).all(), (got["status"], got["stats"])
    assert (got["n_poly"] >= 3).all(), got["n_poly"]
    lim = cc.problem(name, np.float32)
    print()
    for r in range(B):
        n = int(got["n_poly"][r])
        poly = got["poly"][r, :n].astype(np.float64)
        ok0, scene, own, samples = cc.valid_polyline(name, r, poly)
        tol, err, L = _tol(name, r, samples)
        ref64, ref32 = plan_ref.resample(poly, W, np.float64), plan_ref.resample(poly, W, np.float32)
        Q = float(np.abs(poly).max())
        port_q = float(np.abs(ref32.astype(np.float64) - ref64).max())
        tol_q = 4.0 * max(port_q, 2.0 ** -23 * Q)
        err_q = float(np.abs(got["path"][r] - ref64).max())
        print(f"[carry plan, {name}] row {r}: n_poly {n} lowest scene clearance {scene:.5f} carried-against-arm {own:.5f} (tol {tol:.3e}: port {err:.3e}, L {L:.3f}); "
              f"waypoints {err_q:.3e} (tol_q {tol_q:.3e}: port {port_q:.3e}, Q {Q:.3f}); iterations / nodes / checked {got['stats'][r].tolist()}")
        assert np.array_equal(got["poly"][r, 0], c["start"][r]) and np.array_equal(got["poly"][r, n - 1], c["goal"][r])
        assert np.array_equal(got["path"][r, 0], c["start"][r]) and np.array_equal(got["path"][r, -1], c["goal"][r])
        assert scene >= cc.MARGIN - tol, (name, r, scene, tol)
        assert own >= cc.SELF_MARGIN - tol, (name, r, own, tol)
        assert err_q <= tol_q, (name, r, err_q, tol_q)
        assert (got["path"][r] >= lim.lo).all() and (got["path"][r] <= lim.hi).all() and (got["poly"][r, n:] == 0).all()
    # the gap this closes: with the object ignored instead, the plain planner's straight line fails the same validator
    blind = _np(s.plan_path(c["probes"][:c["n_arm"]], c["links"][:c["n_arm"]], c["qadr"], c["goal"], **_budget(c)))
    assert (blind["status"] == 0).all() and (blind["n_poly"] == 2).all() and (blind["stats"][:, 0] == 0).all()
    for r in range(B):
        ok, scene, own, samples = cc.valid_polyline(name, r, blind["poly"][r, :2])
        tol = _tol(name, r, samples)[0]
        assert not ok and min(scene - cc.MARGIN, own - cc.SELF_MARGIN) < -0.01 + tol, (name, r, scene, own)
    # deterministic in the seed, and the seed matters; rows do not depend on one another
    again = _np(s.plan_path(c["probes"], c["links"], c["qadr"], c["goal"], **_budget(c), **_model(c)))
    other = _np(s.plan_path(c["probes"], c["links"], c["qadr"], c["goal"], seed=1, **_budget(c), **_model(c)))
    sub = _np(s.plan_path(c["probes"], c["links"], c["qadr"], c["goal"][[3, 0, 0]], env_idx=torch.tensor([3, 0, 0], device=s.device), **_budget(c), **_model(c)))
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k
        assert np.array_equal(sub[k], got[k][[3, 0, 0]]), k
    assert (other["status"] == 0).all() and other["poly"].tobytes() != got["poly"].tobytes()


# ---------------------------------------------------------------- (d) nothing carried: the bytes of the entry points it extends
def test_nothing_on_the_carried_body_is_the_plain_call():
    c, s = pc.case("post"), _scene("post")
    sb = c["sb"]
    robot = pc.arm(sb)
    probes, links, n_extra, mask = robot.self_collision_model(spacing=pc.SPACING)
    cube = sb.body_index("cube")
    skip = c["skip"] | sum(1 << g for g, geom in enumerate(sb.geoms) if geom["body"] == cube)
    assert not (links == cube).any() and int(mask[cube]) == 0 and not any((int(w) >> cube) & 1 for w in mask)
    args = dict(num_waypoints=W, max_nodes=pc.BUDGET["max_nodes"], max_iterations=pc.BUDGET["max_iterations"], resolution=pc.RESOLUTION, step=pc.STEP,
                margin=pc.MARGIN, skip_geoms=skip)
    carry = dict(body=cube, link=sb.body_index("hand"))
    sm = dict(link_mask=mask, n_extra=n_extra)
    N = len(links) - n_extra
    for label, p, lk, extra in (("self", probes, links, dict(self_model=sm)), ("plain", probes[:N], links[:N], {})):
        plain = _np(s.plan_path(p, lk, c["qadr"], c["goal"], **args, **extra))
        carried = _np(s.plan_path(p, lk, c["qadr"], c["goal"], carry=carry, **args, **extra))
        assert (plain["status"] == 0).all() and (plain["n_poly"] >= 3).all(), label
        for k in plain:
            assert plain[k].tobytes() == carried[k].tobytes(), (label, k)
        assert np.isfinite(carried["grasp"]).all()
        for paths in (np.stack([c["start"], c["goal"]], 1), plain["path"]):
            kw = dict(resolution=pc.RESOLUTION, margin=0.0, skip_geoms=skip)
            a = _np(s.path_clearance(p, lk, c["qadr"], paths, **kw, **extra))
            b = _np(s.path_clearance(p, lk, c["qadr"], paths, carry=carry, **kw, **extra))
            assert set(b) - set(a) == {"grasp"}
            for k in a:
                assert a[k].tobytes() == b[k].tobytes(), (label, k)


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
    att = dict(attached_entity=cube, ee_link_name="hand")
    for t in range(8):
        res = [e.step(A[8 * t % acts.shape[0]]) for e in envs]
        path, valid = robot.plan_path(goal, num_waypoints=8, max_iterations=64, return_valid_mask=True, **att)
        clear = robot.get_path_clearance(path, **att)
        point = robot.get_carried_clearance(**att)
        for k in ("agent_pos", "environment_state"):
            assert torch.equal(res[0][0][k], res[1][0][k]), (t, k)
        assert torch.equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])
        for x, y in zip(mirs[0].get_state(), mirs[1].get_state()):   # qpos, qvel, targets, warm start
            assert torch.equal(x, y), t
        for x, y in zip(mirs[0].get_diag(points=True), mirs[1].get_diag(points=True)):
            assert torch.equal(x, y), t
        assert mirs[0].state_version - v0[0] == mirs[1].state_version - v0[1]
    assert path.shape == (8, n, 9) and valid.shape == (n,) and torch.isfinite(path).all() and not torch.isnan(clear).any()
    assert point["clearance"].shape == (n,) and point["self_clearance"].shape == (n,)
    assert mirs[0].plan_launches == 24


# ---------------------------------------------------------------- (e) blocked rows and refusals
def test_a_bad_grasp_blocks_its_row_only():
    name = "under"
    c, s = cc.case(name), _scene(name)
    good = c["grasp"].astype(np.float32)
    kw = dict(resolution=cc.RESOLUTION, margin=cc.MARGIN, skip_geoms=c["skip"])
    ref_clear = _np(s.path_clearance(c["probes"], c["links"], c["qadr"], _straight(c), **kw, **_model(c, good)))
    ref_plan = _np(s.plan_path(c["probes"], c["links"], c["qadr"], c["goal"], **_budget(c), **_model(c, good)))
    assert (ref_plan["status"] == 0).all()
    keep = [0, 1, 3, 4]
    for label, col, value in (("a NaN position", 1, np.nan), ("an infinite quaternion entry", 4, np.inf), ("a zero quaternion", None, 0.0)):
        bad = good.copy()
        if col is None:
            bad[2, 3:] = 0.0
        else:
            bad[2, col] = value
        clr = _np(s.path_clearance(c["probes"], c["links"], c["qadr"], _straight(c), **kw, **_model(c, bad)))
        pl = _np(s.plan_path(c["probes"], c["links"], c["qadr"], c["goal"], **_budget(c), **_model(c, bad)))
        assert np.isneginf(clr["seg_min"][2]).all() and np.isneginf(clr["row_min"][2]) and np.isneginf(clr["seg_self_min"][2]).all(), label
        assert np.isneginf(clr["row_self_min"][2]) and clr["row_first_blocked"][2] == 0, label
        assert pl["status"][2] == S.PLAN_START_IN_COLLISION and pl["n_poly"][2] == 1 and np.array_equal(pl["path"][2], np.repeat(c["start"][2][None], W, 0)), label
        for k in clr:
            assert clr[k][keep].tobytes() == ref_clear[k][keep].tobytes(), (label, k)
        for k in pl:
            assert pl[k][keep].tobytes() == ref_plan[k][keep].tobytes(), (label, k)


def _raw(s, entry, q, sq, cq, probes, links, qadr, goal, out, self_out=True):
    """a raw call of one of the two entry points -> (return code, error text); `out`: the tensors it may write"""
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    lk = np.ascontiguousarray(links, np.int32)
    qa = np.ascontiguousarray(qadr, np.int32)
    ref = lambda x: None if x is None else C.byref(x)  # noqa: E731
    if entry == "plan":
        rc = s.lib.mir_plan_path_carry(s.h, C.byref(q), ref(sq), ref(cq), p(probes), lk.ctypes.data_as(C.c_void_p), qa.ctypes.data_as(C.c_void_p), None, 0,
                                       None, None, p(goal), p(out["path"]), p(out["status"]), None, None, None, p(out["grasp"]), s._stream())
    else:
        rc = s.lib.mir_path_clearance_carry(s.h, C.byref(q), ref(sq), ref(cq), p(probes), lk.ctypes.data_as(C.c_void_p), qa.ctypes.data_as(C.c_void_p), None,
                                            0, None, None, p(out["paths"]), 2, p(out["seg"]), p(out["seg"]) if self_out else None, None, None, None,
                                            p(out["grasp"]), s._stream())
    torch.cuda.synchronize()
    return rc, s.lib.mir_last_error()


def test_refusals_launch_nothing():
    from gym_genesis.backend.lib import MirScene

    name = "under"
    c, s = cc.case(name), _scene(name)
    NS, E, D = len(c["links"]), c["n_extra"], len(c["qadr"])
    N = NS - E
    probes, goal = torch.as_tensor(c["probes"], device=s.device), torch.as_tensor(c["goal"], device=s.device)
    nan = lambda *shape: torch.full(shape, float("nan"), device=s.device)  # noqa: E731
    out = {"path": nan(B, W, D), "status": torch.full((B,), -7, dtype=torch.int32, device=s.device), "seg": nan(B, 1), "grasp": nan(B, 7),
           "paths": torch.as_tensor(_straight(c), device=s.device)}
    q = make_plan_query(N, D, W, 128, 512, skip_geoms=c["skip"])
    sq = make_self_query(c["mask"], E)
    nbody, Cb, Lk = c["spec"].nbody, c["body"], c["link"]
    launches = s.__dict__.get("plan_launches", 0)
    bad = [None]
    cq = make_carry_query(Cb, Lk); cq.struct_size += 4; bad.append(cq)
    cq = make_carry_query(Cb, Lk); cq.flags = 1; bad.append(cq)
    bad += [make_carry_query(Lk, Cb), make_carry_query(0, Lk), make_carry_query(-1, Lk), make_carry_query(nbody, Lk)]   # C is not a free-joint body
    bad += [make_carry_query(Cb, -1), make_carry_query(Cb, nbody), make_carry_query(Cb, Cb)]                           # Lk outside the bodies, Lk == C
    for cq in bad:
        for entry, who in (("plan", b"mir_plan_path_carry"), ("clear", b"mir_path_clearance_carry")):
            for with_sq in (sq, None):
                rc, msg = _raw(s, entry, q, with_sq, cq, probes, c["links"], c["qadr"], goal, out, self_out=with_sq is not None)
                assert rc == -1 and who in msg, (entry, rc, msg)
    # a geom of C that is not skipped; self outputs without a self query; what the extended entry points refuse stays refused
    cube_geoms = sum(1 << g for g, geom in enumerate(c["sb"].geoms) if geom["body"] == Cb)
    open_q = make_plan_query(N, D, W, 128, 512, skip_geoms=c["skip"] & ~cube_geoms)
    bad_q = make_plan_query(N, D, W, 128, 512, resolution=0.0, skip_geoms=c["skip"])
    bad_sq = make_self_query(c["mask"], E, self_margin=-0.01)
    for entry in ("plan", "clear"):
        rc, msg = _raw(s, entry, open_q, sq, make_carry_query(Cb, Lk), probes, c["links"], c["qadr"], goal, out)
        assert rc == -1 and b"carried body is not skipped" in msg, (entry, rc, msg)
        assert _raw(s, entry, bad_q, sq, make_carry_query(Cb, Lk), probes, c["links"], c["qadr"], goal, out)[0] == -1
        assert _raw(s, entry, q, bad_sq, make_carry_query(Cb, Lk), probes, c["links"], c["qadr"], goal, out)[0] == -1
    rc, msg = _raw(s, "clear", q, None, make_carry_query(Cb, Lk), probes, c["links"][:N], c["qadr"], goal, out, self_out=True)
    assert rc == -1 and b"without a MirSelfQuery" in msg, (rc, msg)
    # C has a child body: the same scene with a tag bolted to the cube
    sb = cc.builder(name)
    sb.add_body("tag", "cube", pos=(0.0, 0.0, 0.03), mass=0.001, inertia=(1e-8, 1e-8, 1e-8, 0, 0, 0))
    s2 = MirScene(sb.build(), B)
    q2 = np.zeros((B, s2.nq), np.float32)
    q2[:, :c["q"].shape[1]] = c["q"]
    s2.set_state(qpos=q2, qvel=np.zeros((B, s2.nv), np.float32))
    for entry in ("plan", "clear"):
        rc, msg = _raw(s2, entry, q, sq, make_carry_query(Cb, Lk), probes, c["links"], c["qadr"], goal, out)
        assert rc == -1 and b"child body" in msg, (entry, rc, msg)
    torch.cuda.synchronize()
    assert torch.isnan(out["path"]).all() and (out["status"] == -7).all() and torch.isnan(out["seg"]).all() and torch.isnan(out["grasp"]).all(), \
        "a refused call launches nothing"
    # the good query launches, with and without a self query
    for with_sq in (sq, None):
        for t in (out["path"], out["seg"], out["grasp"]):
            t.fill_(float("nan"))
        lk = c["links"] if with_sq is not None else c["links"][:N]
        assert _raw(s, "plan", q, with_sq, make_carry_query(Cb, Lk), probes, lk, c["qadr"], goal, out)[0] == 0
        assert torch.isfinite(out["path"]).all() and torch.isfinite(out["grasp"]).all()
        out["grasp"].fill_(float("nan"))
        assert _raw(s, "clear", q, with_sq, make_carry_query(Cb, Lk), probes, lk, c["qadr"], goal, out, self_out=with_sq is not None)[0] == 0
        assert torch.isfinite(out["seg"]).all() and torch.isfinite(out["grasp"]).all()
    assert s.__dict__.get("plan_launches", 0) == launches, "the wrappers' counters saw none of the raw calls"
    assert C.sizeof(S.MirCarryQuery) == s.lib.mir_carry_query_sizeof()


# ---------------------------------------------------------------- (f) the entity's calls
@pytest.mark.parametrize("name", cc.NAMES)
def test_entity_calls_are_the_same_launch(name):
    c, s = cc.case(name), _scene(name)
    robot, obj, cube = cc.views(name, c["sb"], s)
    others = [cube] if name == "rod" else []
    goal = torch.as_tensor(c["goal"], device=s.device)
    att = dict(attached_entity=obj, ee_link_name="hand", self_collision=False, ignore_entities=others)
    kw = dict(num_waypoints=W, max_nodes=cc.BUDGET["max_nodes"], max_iterations=cc.BUDGET["max_iterations"], resolution=cc.RESOLUTION, step=cc.STEP,
              margin=cc.MARGIN)
    raw = _np(s.plan_path(c["probes"], c["links"], c["qadr"], c["goal"], **_budget(c), **_model(c)))
    det = _np(robot.plan_path(goal, return_detail=True, **kw, **att))
    assert det["valid"].all() and det["path"].shape == (W, B, len(c["qadr"]))
    assert det["path"].transpose(1, 0, 2).tobytes() == raw["path"].tobytes()
    for k in ("status", "poly", "n_poly", "stats", "grasp"):
        assert det[k].tobytes() == raw[k].tobytes(), k
    # the object ignored instead: the straight line, which the swept check with the object attached rejects
    blind = robot.plan_path(goal, ignore_entities=[obj] + others, **kw)
    assert robot.path_in_collision(blind, **att).all() and not robot.path_in_collision(blind, ignore_entities=[obj] + others).any()
    d = robot.get_path_clearance(blind, return_detail=True, **att)
    two = _np(s.path_clearance(c["probes"], c["links"], c["qadr"], blind.permute(1, 0, 2).contiguous(), resolution=cc.RESOLUTION, skip_geoms=c["skip"], **_model(c)))
    assert np.array_equal(d["clearance"].cpu().numpy(), two["row_min"]) and np.array_equal(d["self_clearance"].cpu().numpy(), two["row_self_min"])
    assert np.array_equal(d["grasp"].cpu().numpy(), raw["grasp"]) and np.array_equal(d["first_blocked"].cpu().numpy(), two["row_first_blocked"])
    # a given grasp, broadcast from (7,) or per row
    g = torch.as_tensor(c["grasp"].astype(np.float32), device=s.device)
    per_row = robot.plan_path(goal, grasp_pose=g, return_detail=True, **kw, **att)
    assert per_row["valid"].all() and np.array_equal(per_row["grasp"][:, :3].cpu().numpy(), c["grasp"][:, :3].astype(np.float32))
    one = robot.get_path_clearance(blind, grasp_pose=g[0], return_detail=True, **att)["grasp"]
    assert torch.equal(one, one[:1].expand(B, 7))
    # the point query: the two-point trajectory [q, q]
    mid = torch.as_tensor(0.5 * (c["start"] + c["goal"]), device=s.device)
    point = robot.get_carried_clearance(qpos=mid, attached_entity=obj, ee_link_name="hand", self_collision=False, ignore_entities=others)
    full = c["q"].copy()
    full[:, c["qadr"]] = mid.cpu().numpy()
    twice = _np(s.path_clearance(c["probes"], c["links"], c["qadr"], torch.stack([mid, mid], 1), qpos_start=torch.as_tensor(full, device=s.device),
                                 skip_geoms=c["skip"], **_model(c)))
    assert np.array_equal(point["clearance"].cpu().numpy(), twice["row_min"]) and np.array_equal(point["self_clearance"].cpu().numpy(), twice["row_self_min"])
    at_state = robot.get_carried_clearance(attached_entity=obj, ee_link_name="hand", self_collision=False, ignore_entities=others)
    assert (at_state["clearance"] >= 0.02).all() and (at_state["self_clearance"] >= 0.02).all(), "the start rows are clear"
    # no test against the arm: the self value is the cap
    off = robot.get_carried_clearance(qpos=mid, attached_entity=obj, ee_link_name="hand", attached_links=[], self_collision=False, ignore_entities=others)
    assert (off["self_clearance"] == 1.0).all() and torch.equal(off["clearance"], point["clearance"])


def test_an_unbatched_view_drops_the_env_axis():
    from gym_genesis.backend.lib import MirScene

    name = "under"
    c = cc.case(name)
    s = MirScene(c["spec"], 1)
    s.set_state(qpos=c["q"][:1], qvel=np.zeros((1, s.nv), np.float32))
    robot, obj, _ = cc.views(name, c["sb"], s)
    robot.unbatched = True
    att = dict(attached_entity=obj, ee_link_name="hand", self_collision=False)
    det = robot.plan_path(torch.as_tensor(c["goal"][0], device=s.device), num_waypoints=W, max_nodes=cc.BUDGET["max_nodes"],
                          max_iterations=cc.BUDGET["max_iterations"], return_detail=True, **att)
    assert det["path"].shape == (W, len(c["qadr"])) and det["grasp"].shape == (7,) and det["valid"].dim() == 0 and bool(det["valid"])
    batched = _np(_scene(name).plan_path(c["probes"], c["links"], c["qadr"], c["goal"], **_budget(c), **_model(c)))
    assert np.array_equal(det["path"].cpu().numpy(), batched["path"][0]) and np.array_equal(det["grasp"].cpu().numpy(), batched["grasp"][0])
    d = robot.get_path_clearance(det["path"], return_detail=True, **att)
    assert d["clearance"].dim() == 0 and d["self_clearance"].dim() == 0 and d["seg_min"].shape == (W - 1,) and d["grasp"].shape == (7,)
    assert robot.path_in_collision(det["path"], **att).dim() == 0
    point = robot.get_carried_clearance(**att)
    assert point["clearance"].dim() == 0 and point["self_clearance"].dim() == 0
