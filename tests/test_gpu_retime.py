"""Batched time parameterisation on the GPU (include/mirigid.h: mir_retime_path; tasks/views.py: EntityView.retime_path).

The cases -- paths, limits, extra rows, T -- are those of tests/retime_cases.py: R = 5 rows, (D, E) in {(1, 0), (9, 0), (9, 9), (16, 16)}
(the last fills all 64 lanes), K in {3, 16, 65, 100}, T no multiple of 64.  tests/test_retime_cpu.py holds the conditions that make the
comparisons fair (the float64 reference keeps every promise of the specification; its float32 port fails no row; the torque rows bind).

The GPU's result is judged on its own, in float64: its (x, u) satisfy every row and cap; t, the samples and the velocities are steps 8
and 9 applied in float64 to the GPU's own x; n_samples is that of its own duration.  Then against the reference: x, t and the duration
(the LP optimum is unique in value, so no branch can differ).

Yardstick, printed before it is used: tol = 4 x max(float32 port in the same comparison on the same inputs, 2^-23 x scale); the scale is
the largest x, the duration (for t too), the largest |q| (samples), the largest velocity, or -- for an overshoot relative to a row's
limit or to the cap -- 1.  What is judged on the GPU's own x takes the port judged on the port's own x.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import retime_cases as rc
import retime_ref as rr
from gym_genesis.backend import models
from gym_genesis.backend import spec as S

pytestmark = pytest.mark.gpu

R = rc.R
_sc = []


def _scene():
    if not _sc:
        from gym_genesis.backend.lib import MirScene

        _sc.append(MirScene(models.franka_cube_pick_scene().build(), 4))
    return _sc[0]


def _retime(paths, vmax, amax, T, extra=None, velocity=True, dt=rc.DT):
    out = _scene().retime_path(paths, vmax, amax, dt, num_samples=T, extra=extra, velocity=velocity)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _case(name, rows=None):
    c = rc.case(name)
    sel = slice(None) if rows is None else list(rows)
    ex = None if c["extra"] is None else tuple(e[sel] for e in c["extra"])
    return _retime(c["paths"][sel], c["vmax"], c["amax"], rc.capacity(name), ex)


def _own_float64(P, x, dt, T):
    """steps 8 and 9 in float64 on an x in the caller's indexing -> the dict of retime_ref.finish"""
    kept = rr.compact(P)
    xk = np.asarray(x, np.float64)[kept]
    return rr.finish({"status": rr.OK}, P, kept, xk, rr.times_from_x(xk), np.float64(np.float32(dt)), T), kept


def _n_samples_ok(got, duration, dt):
    """n_samples against the float64 value of the GPU's own duration; the neighbouring integer when duration / dt is within 2^-20
    relative of an integer"""
    ratio = float(duration) / float(np.float32(dt))
    want = int(np.ceil(ratio)) + 1
    near = abs(ratio - round(ratio)) <= 2.0 ** -20 * ratio
    return got == want or (near and abs(got - want) == 1)


def _own_errors(c, res, T, margin):
    """A result (the GPU's or the port's) against steps 8 and 9 applied in float64 to ITS OWN x: the largest difference of t (and the
    duration), of the samples, and of the velocities at the samples that keep `margin` from every t_i (velocities jump from one
    interval to the next) -> dict(t, q, v)"""
    worst = dict(t=0.0, q=0.0, v=0.0)
    tau = np.arange(T) * np.float64(np.float32(rc.DT))
    for r in range(R):
        own, kept = _own_float64(c["paths"][r], res["x"][r], rc.DT, T)
        worst["t"] = max(worst["t"], float(np.abs(res["t"][r] - own["t"]).max()), abs(float(res["duration"][r]) - float(own["duration"])))
        worst["q"] = max(worst["q"], float(np.abs(res["samples"][r] - own["samples"]).max()))
        clear = np.abs(tau[:, None] - own["t"][None, kept]).min(1) > margin
        worst["v"] = max(worst["v"], float(np.abs(res["sample_vel"][r][clear] - own["sample_vel"][clear]).max()))
    return worst


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_cases(name):
    c, ref, port = rc.case(name), rc.reference(name), rc.reference(name, "float32")
    T = rc.capacity(name)
    got = _case(name)
    tol, line = rc.yardstick(name)
    # the yardsticks of what is judged on its own, each the port's figure in the same comparison: its overshoot of a row or of the cap,
    # and its t, samples and velocities against steps 8 and 9 applied in float64 to the PORT's own x
    over = [rr.row_violation(c["paths"][r], port["x"][r], c["vmax"], c["amax"], 1.0 / rc.DT, None if c["extra"] is None else tuple(e[r] for e in c["extra"]))
            for r in range(R)]
    tol_row = 4.0 * max(max(max(o) for o in over), 2.0 ** -23)
    scale = dict(t=float(ref["duration"].max()), q=float(np.abs(c["paths"]).max()), v=float(np.abs(ref["sample_vel"]).max()))
    margin = 4.0 * 2.0 ** -23 * scale["t"] * c["paths"].shape[1]   # (a t_i is a float32 sum of at most K terms of at most the duration)
    port_own = _own_errors(c, port, T, margin)
    tol_own = {k: 4.0 * max(port_own[k], 2.0 ** -23 * scale[k]) for k in port_own}
    print("\n" + line + f"; rows and cap {tol_row:.3e} (relative); on its own x: " +
          "; ".join(f"{k}: port {port_own[k]:.3e} scale {scale[k]:.3e} tol {tol_own[k]:.3e}" for k in port_own))
    assert (got["status"] == rr.OK).all(), got["status"]
    assert got["samples"].shape == got["sample_vel"].shape == (R, T, c["paths"].shape[2]) and T % 64 != 0
    rows = cap = 0.0
    for r in range(R):
        P = c["paths"][r]
        ex = None if c["extra"] is None else tuple(e[r] for e in c["extra"])
        o = rr.row_violation(P, got["x"][r], c["vmax"], c["amax"], 1.0 / rc.DT, ex)
        rows, cap = max(rows, o[0]), max(cap, o[1])
        assert got["x"][r][0] == 0 and got["x"][r][-1] == 0 and got["t"][r][0] == 0 and got["duration"][r] == got["t"][r][-1]
        assert _n_samples_ok(int(got["n_samples"][r]), got["duration"][r], rc.DT), (r, got["n_samples"][r], got["duration"][r])
        assert np.array_equal(got["samples"][r][0], P[0]) and (got["samples"][r][got["n_samples"][r]:] == P[-1]).all()
        assert (got["sample_vel"][r][0] == 0).all() and (got["sample_vel"][r][got["n_samples"][r]:] == 0).all()
    worst = _own_errors(c, got, T, margin)
    print(f"[retime, {name}] on its own: rows {rows:.3e} cap {cap:.3e} allowed {tol_row:.3e}; " +
          "; ".join(f"{k} {worst[k]:.3e} allowed {tol_own[k]:.3e}" for k in worst))
    assert rows <= tol_row and cap <= tol_row and all(worst[k] <= tol_own[k] for k in worst)
    err = {k: float(np.abs(got[k].astype(np.float64) - ref[k]).max()) for k in ("x", "t", "duration")}
    print(f"[retime, {name}] against the reference: " + "; ".join(f"{k} {err[k]:.3e} allowed {tol[k]:.3e}" for k in err))
    assert all(err[k] <= tol[k] for k in err)
    assert (np.abs(got["n_samples"] - ref["n_samples"]) <= 1).all()


@pytest.mark.parametrize("K", sorted(rc.KNOWN))
def test_known_answers(K):
    ref, port = rc.known(K), rc.known(K, "float32")
    tol = 4.0 * max(abs(float(port["duration"]) - float(ref["duration"])), 2.0 ** -23 * rc.KNOWN[K])
    got = _retime(np.tile(rc.known_path(K, np.float32)[None], (2, 1, 1)), [1.0], [2.5], 160, velocity=False)
    err = np.abs(got["duration"].astype(np.float64) - rc.KNOWN[K]).max()
    print(f"\n[retime, known K = {K}] duration {got['duration'][0]!r} against {rc.KNOWN[K]}: {err:.3e} allowed {tol:.3e}")
    assert (got["status"] == rr.OK).all() and err <= tol and got["duration"][0] == got["duration"][1]
    fd = np.abs(np.diff(got["samples"][0][:, 0].astype(np.float64))) / np.float64(np.float32(rc.DT))
    assert fd.max() <= 1.0 + 2.0 ** -22 * 1.0 / rc.DT, "two roundings of q"


def _status_call():
    """K = 12, D = 9, E = 1: row 0 ordinary, 1 NO_MOTION, 2 TOO_FEW_WAYPOINTS, 3 NOT_FINITE (path), 4 INFEASIBLE (an extra row with lo = 0),
    5 NOT_FINITE (an extra row at a kept waypoint), 6 ordinary with repeated waypoints whose extra rows are NaN"""
    c = rc.case("acc")
    P = np.stack([c["paths"][r % R][:12] for r in range(7)]).copy()
    P[1] = P[1][:1]
    P[2][1:6], P[2][6:] = P[2][0], P[2][11]
    P[3][7, 3] = np.inf
    P[6] = np.concatenate([P[0][:1], P[0][:5], P[0][4:5], P[0][5:10]])   # waypoints 1 and 6 repeat the one in front of them
    ex = [np.full((7, 12, 1), v, np.float32) for v in (0.3, 0.01, -50.0, 50.0)]
    ex[2][4, 5] = 0.0
    ex[1][5, 9] = np.nan
    for e in ex:
        e[6, [1, 6]] = np.nan
    return c, P, tuple(ex)


def test_statuses_share_a_call_with_an_ordinary_row():
    c, P, ex = _status_call()
    T = 333
    got = _retime(P, c["vmax"], c["amax"], T, ex)
    assert list(got["status"]) == [rr.OK, rr.NO_MOTION, rr.TOO_FEW_WAYPOINTS, rr.NOT_FINITE, rr.INFEASIBLE, rr.NOT_FINITE, rr.OK], got["status"]
    for r in (1, 2, 3, 4, 5):
        assert got["duration"][r] == 0 and got["n_samples"][r] == 1 and (got["x"][r] == 0).all() and (got["t"][r] == 0).all()
        assert np.array_equal(got["samples"][r].view(np.uint32), np.tile(P[r][0], (T, 1)).view(np.uint32)) and (got["sample_vel"][r] == 0).all()
    alone = _retime(P[:1], c["vmax"], c["amax"], T, tuple(e[:1] for e in ex))
    for k in got:
        assert np.array_equal(got[k][0], alone[k][0]), k
    # row 6 is row 0's first ten waypoints with two of them repeated: the x, t and samples of the path without them
    short = _retime(P[0:1, :10], c["vmax"], c["amax"], T, tuple(e[0:1, :10] for e in ex))
    kept = rr.compact(P[6])
    assert len(kept) == 10 and np.array_equal(got["x"][6][kept], short["x"][0]) and np.array_equal(got["t"][6][kept], short["t"][0])
    assert np.array_equal(got["samples"][6], short["samples"][0]) and got["x"][6][1] == got["x"][6][0] and got["t"][6][6] == got["t"][6][5]
    # a small T: TRUNCATED, x, t and the duration stay, the first T samples are written
    cut = _retime(P[[0, 1]], c["vmax"], c["amax"], 17, tuple(e[[0, 1]] for e in ex))
    assert list(cut["status"]) == [rr.TRUNCATED, rr.NO_MOTION] and cut["n_samples"][0] == got["n_samples"][0] > 17
    assert np.array_equal(cut["samples"][0], got["samples"][0][:17]) and np.array_equal(cut["x"][0], got["x"][0]) and cut["duration"][0] == got["duration"][0]
    ref = rr.retime(P, c["vmax"], c["amax"], rc.DT, T, None, ex)
    assert np.array_equal(ref["status"], got["status"])


def test_determinism_independence_and_state():
    sc = _scene()
    state = [x.clone() for x in sc.get_state()]
    version, launches = sc.state_version, sc.__dict__.get("retime_launches", 0)
    a, b = _case("extra"), _case("extra")
    sub = _case("extra", rows=(3, 1))
    for k in a:
        assert np.array_equal(a[k], b[k]), f"{k}: the same call twice"
        assert np.array_equal(sub[k], a[k][[3, 1]]), f"{k}: a row's bits do not depend on the other rows of the call"
    assert all(torch.equal(x, y) for x, y in zip(state, sc.get_state())) and sc.state_version == version
    assert sc.retime_launches == launches + 3
    none = sc.retime_path(torch.zeros((0, 5, 9), device=sc.device), 2.0, 3.0, rc.DT, num_samples=4)
    assert none["samples"].shape == (0, 4, 9) and sc.retime_launches == launches + 3


def _raw(sc, q, paths, out, extra=(None,) * 4, n_rows=R, samples=True, handle=True, vel=None):
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    rc_ = sc.lib.mir_retime_path(sc.h if handle else None, None if q is None else C.byref(q), n_rows, p(paths), *(p(e) for e in extra), p(out["x"]), p(out["t"]),
                                 p(out["duration"]), p(out["status"]), p(out["n_samples"]), p(out["samples"]) if samples else None, p(vel), sc._stream())
    torch.cuda.synchronize()
    return rc_, sc.lib.mir_last_error()


def test_refusals_launch_nothing():
    sc, c = _scene(), rc.case("three")
    K, D, T = 3, 9, 40
    paths = torch.as_tensor(c["paths"], device=sc.device)
    nan = lambda *s: torch.full(s, float("nan"), device=sc.device)  # noqa: E731
    out = {"x": nan(R, K), "t": nan(R, K), "duration": nan(R), "samples": nan(R, T, D),
           "status": torch.full((R,), -7, dtype=torch.int32, device=sc.device), "n_samples": torch.full((R,), -7, dtype=torch.int32, device=sc.device)}
    good = lambda **kw: S.make_retime_query(D, K, 2.0, 3.0, rc.DT, kw.pop("T", T), None, kw.pop("E", 0))  # noqa: E731
    assert _raw(sc, good(T=600), paths, dict(out, samples=nan(R, 600, D)))[0] == 0 and (out["status"] == 0).all() and torch.isfinite(out["x"]).all()
    for v in out.values():
        v.fill_(float("nan") if v.dtype == torch.float32 else -7)
    bad = [_raw(sc, None, paths, out), _raw(sc, good(), None, out), _raw(sc, good(), paths, dict(out, duration=None))]
    q = good(); q.struct_size += 4; bad.append(_raw(sc, q, paths, out))
    q = good(); q.n_dofs = 17; bad.append(_raw(sc, q, paths, out))
    q = good(); q.num_waypoints = 1; bad.append(_raw(sc, q, paths, out))
    q = good(); q.flags = 4; bad.append(_raw(sc, q, paths, out))
    q = good(); q.amax[3] = float("nan"); bad.append(_raw(sc, q, paths, out))
    q = good(); q.dt = 0.0; bad.append(_raw(sc, q, paths, out))
    bad.append(_raw(sc, good(T=0), paths, out))
    bad.append(_raw(sc, good(T=0), paths, out, samples=False, vel=out["samples"]))   # sample_vel alone with T < 1
    bad.append(_raw(sc, good(E=1), paths, out))   # E > 0 with null extra arrays
    bad.append(_raw(sc, good(), paths, out, handle=False))
    bad.append(_raw(sc, good(), paths, out, n_rows=-1))
    q = good(); q.n_extra = -1; bad.append(_raw(sc, q, paths, out))
    q = good(); q.num_samples = -1; bad.append(_raw(sc, q, paths, out, samples=False))
    for v in (0.0, float("inf")):
        q = good(); q.vmax[8] = v; bad.append(_raw(sc, q, paths, out))
        q = good(); q.max_path_speed = v; bad.append(_raw(sc, q, paths, out))
    for rc_, msg in bad:
        assert rc_ == -1 and b"mir_retime_path" in msg, (rc_, msg)
    e = torch.zeros((R, K, 24), device=sc.device)
    cap = [_raw(sc, good(E=24), paths, out, extra=(e,) * 4)]
    q = good(); q.num_waypoints = S.RETIME_MAX_WAYPOINTS + 1; cap.append(_raw(sc, q, paths, out))
    cap.append(_raw(sc, good(T=2 ** 28), paths, out, n_rows=R, samples=False))
    for rc_, msg in cap:
        assert rc_ == -2 and b"mir_retime_path" in msg, (rc_, msg)
    bufs = (sc.empty(sc.agent_dim), sc.empty(sc.env_dim), sc.empty(), sc.empty(dtype=torch.uint8))
    state = [x.clone() for x in sc.get_state()]
    sc.step_begin(None, *bufs)
    rc_, msg = _raw(sc, good(), paths, out)
    sc.step_end()
    sc.set_state(*state)
    torch.cuda.synchronize()
    assert rc_ == -1 and b"mir_retime_path" in msg and b"pending" in msg
    assert all(torch.isnan(out[k]).all() for k in ("x", "t", "duration", "samples")) and (out["status"] == -7).all() and (out["n_samples"] == -7).all()
    assert C.sizeof(S.MirRetimeQuery) == sc.lib.mir_retime_query_sizeof()


def test_plan_then_retime_on_the_pick_task():
    from gym_genesis.env import GenesisEnv

    n, W, vmax, amax = 5, 32, 2.0, 20.0
    env = GenesisEnv(task="cube_pick", robot="franka", num_envs=n, enable_pixels=False)
    env.reset(seed=5)
    task = env._env
    robot, cube, mir = task.franka, task.cube, task._mir
    q0 = robot.get_qpos().clone()
    goal = torch.tensor((0.9, -0.35, 0.05, -2.1, 0.0, 1.9, 0.7, 0.04, 0.04), device=mir.device).expand(n, 9).clone()
    goal[:, :7] += torch.as_tensor(np.random.default_rng(3).uniform(-0.1, 0.1, (n, 7)).astype(np.float32), device=mir.device)
    goal[2] = q0[2]   # a row that stays where it is (planned or refused, it holds its start W times)
    path, valid = robot.plan_path(goal, num_waypoints=W, ignore_entities=[cube], return_valid_mask=True)
    assert valid[[0, 1, 3, 4]].all() and (path[:, 2] == q0[2]).all()
    grav = robot.inverse_dynamics(torch.zeros((n * W, 9), device=mir.device), qpos=path.permute(1, 0, 2).reshape(n * W, 9),
                                  qvel=torch.zeros((n * W, 9), device=mir.device), envs_idx=torch.arange(n, device=mir.device).repeat_interleave(W))
    tmax = 1.05 * float(grav.abs().max())   # (little is left for accelerating the joint that carries the arm: the rows bind)
    state, version = [x.clone() for x in mir.get_state()], mir.state_version
    det = robot.retime_path(path, vmax, amax, torque_limits=torch.full((9,), tmax, device=mir.device), return_detail=True)
    free = robot.retime_path(path, vmax, amax, return_detail=True)
    assert all(torch.equal(x, y) for x, y in zip(state, mir.get_state())) and mir.state_version == version
    status = det["status"].cpu().numpy()
    assert list(status) == [rr.OK, rr.OK, rr.NO_MOTION, rr.OK, rr.OK] and det["valid"].all()
    smp, dt = det["samples"].cpu().numpy().astype(np.float64), float(np.float32(robot._b.opt["dt"]))
    T = smp.shape[0]
    assert T == int(det["n_samples"].max()) and smp.shape == (T, n, 9)
    assert torch.equal(det["samples"][0], path[0]) and torch.equal(det["samples"][-1], path[-1]) and (det["samples"][:, 2] == q0[2]).all()
    fd = np.abs(np.diff(smp, axis=0)).max() / dt
    allowed = vmax + 2.0 ** -22 * float(np.abs(smp).max()) / dt
    print(f"\n[retime, pick] durations {det['duration'].cpu().numpy()} s with the torque rows, {free['duration'].cpu().numpy()} s without; "
          f"finite-difference velocity {fd:.6f} allowed {allowed:.6f}")
    moving = [0, 1, 3, 4]
    assert fd <= allowed and (det["duration"][moving] > free["duration"][moving]).all(), "the torque rows bind"
    # the collocated torque at (Q_i, m_i sqrt(x_i), m_i u_i + c_i x_i), by the scene's own inverse dynamics
    P = path.permute(1, 0, 2).cpu().numpy()
    x = det["x"].cpu().numpy().astype(np.float64)
    qv, qa = np.zeros((n, W, 9)), np.zeros((n, W, 9))
    for r in range(n):
        kept = rr.compact(P[r])
        m, c = rr.compact_differences(P[r])
        xk = x[r][kept]
        u = np.zeros(len(kept))
        u[:-1] = 0.5 * np.diff(xk)
        qv[r], qa[r] = m * np.sqrt(x[r])[:, None], m * rr.expand(u, kept, W)[:, None] + c * x[r][:, None]
    dev = lambda a: torch.as_tensor(a.reshape(n * W, 9).astype(np.float32), device=mir.device)  # noqa: E731
    tau = robot.inverse_dynamics(dev(qa), qpos=dev(P), qvel=dev(qv), envs_idx=torch.arange(n, device=mir.device).repeat_interleave(W)).abs().max().item()
    # yardstick, on the same inputs: the rows the call above was given (rebuilt here: the same arithmetic on the same path) through the
    # float32 port on the CPU, and the port's overshoot of a row relative to its limit
    rows = path.permute(1, 0, 2).contiguous()
    ext = [e.cpu().numpy() for e in robot._torque_rows(rows, None, n, torch.full((9,), tmax, device=mir.device))]
    over = 0.0
    for r in moving:
        ex = tuple(e[r] for e in ext)
        port = rr.retime_row(P[r], [vmax] * 9, [amax] * 9, dt, 0, None, ex, np.float32, False)
        assert port["status"] == rr.OK
        over = max(over, rr.row_violation(P[r], port["x"], [vmax] * 9, [amax] * 9, 1.0 / dt, ex)[0])
    tol = 4.0 * max(over, 2.0 ** -23) * tmax
    print(f"[retime, pick] collocated torque {tau:.6f} N m against tmax {tmax:.6f}: over by {tau - tmax:.3e}, allowed {tol:.3e} "
          f"(port's relative row overshoot {over:.3e})")
    assert tau <= tmax + tol


def test_the_example_runs(monkeypatch):
    """examples/franka/plan_retime_follow.py end to end (how closely either set of targets is followed is the controller's business:
    printed, not asserted)"""
    import importlib.util
    import os
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("plan_retime_follow", os.path.join(root, "examples", "franka", "plan_retime_follow.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(sys, "argv", ["plan_retime_follow.py", "--num-envs", "16", "--waypoints", "30"])
    retimed, stepped = mod.main()
    assert np.isfinite(retimed) and np.isfinite(stepped), (retimed, stepped)
