"""CPU tier of the time parameterisation (include/mirigid.h: mir_retime_path; tasks/views.py: EntityView.retime_path).

What is checked here, without a device:
  - the float64 reference (tests/retime_ref.py) on the known answers and, on every case of tests/retime_cases.py, by the properties
    the specification promises (every row of step 5 holds at (x_i, u_i), x_i <= cap_i, t increases, rest at both ends, every sample on
    a segment of the path, the finite difference of the samples within vmax);
  - statuses and compaction;
  - the conditions the GPU tier leans on: the float32 port fails no row the reference times, its distance from the reference (the
    yardstick, printed) stays small against the outputs' scale, and the torque rows of the torque case bind;
  - EntityView.retime_path against a stub scene that answers with the reference: layouts, refine, the two-launch sizing, the torque
    rows over the kept waypoints, the ValueErrors, the unbatched form;
  - every refusal of the entry point through the g++ build of gym-genesis_amd/csrc/mir_retime_front.h (`make retime-host`).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import retime_cases as rc
import retime_ref as rr
from gym_genesis.backend import models
from gym_genesis.backend import spec as S
from gym_genesis.tasks.views import EntityView

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- known answers
@pytest.mark.parametrize("K", sorted(rc.KNOWN))
def test_known_answers(K):
    o = rc.known(K)
    err = abs(float(o["duration"]) - rc.KNOWN[K])
    print(f"\n[retime, known K = {K}] duration {o['duration']!r} against {rc.KNOWN[K]}: {err:.2e}")
    assert o["status"] == rr.OK and err <= 1e-13
    x = o["x"]
    peak = 1.0e4 if K == 101 else 2.5 * 0.1 / 1e-4   # (v / d)^2; the triangle peaks at v^2 = a L
    assert abs(x.max() - peak) <= 1e-9 * peak and x[0] == 0 and x[-1] == 0
    assert o["n_samples"] == int(np.ceil(rc.KNOWN[K] / np.float64(np.float32(rc.DT)) - 1e-9)) + 1   # (dt is the float32 nearest 0.01, a little below it)


# ---- properties of the float64 reference on every case
def _on_polyline(S_, P):
    """the largest distance of a sample from the polyline P (K, D), float64"""
    a, d = P[:-1], P[1:] - P[:-1]
    f = np.clip(np.einsum("tkd,kd->tk", S_[:, None, :] - a[None], d) / np.maximum((d * d).sum(1), 1e-300), 0.0, 1.0)
    dist = np.linalg.norm(S_[:, None, :] - (a[None] + f[..., None] * d[None]), axis=2)
    return float(dist.min(1).max())


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_reference_properties(name):
    c, ref = rc.case(name), rc.reference(name)
    T = rc.capacity(name)
    assert T % 64 != 0 and (ref["status"] == rr.OK).all() and (ref["n_samples"] <= T).all()
    for r in range(rc.R):
        P = c["paths"][r]
        ex = None if c["extra"] is None else tuple(e[r] for e in c["extra"])
        rows, cap = rr.row_violation(P, ref["x"][r], c["vmax"], c["amax"], 1.0 / rc.DT, ex)
        assert rows <= 1e-12 and cap <= 1e-12, (name, r, rows, cap)
        x, t = ref["x"][r], ref["t"][r]
        assert x[0] == 0 and x[-1] == 0 and t[0] == 0 and (np.diff(t) > 0).all() and t[-1] == ref["duration"][r]
        smp = ref["samples"][r]
        assert np.array_equal(smp[0], P[0]) and np.array_equal(smp[ref["n_samples"][r] - 1:], np.tile(P[-1], (T - ref["n_samples"][r] + 1, 1)))
        assert _on_polyline(smp, P.astype(np.float64)) <= 1e-12 * 1.5 * np.sqrt(P.shape[1])
        fd = np.abs(np.diff(smp, axis=0)) / np.float64(np.float32(rc.DT))
        assert (fd <= c["vmax"].astype(np.float64) * (1 + 1e-12)).all(), (name, r, float((fd / c["vmax"]).max()))
        assert (ref["sample_vel"][r][0] == 0).all() and (ref["sample_vel"][r][ref["n_samples"][r] - 1:] == 0).all()


# ---- statuses and compaction
def test_repeated_waypoints_are_dropped():
    c = rc.case("acc")
    P = c["paths"][0][:20]
    rep = np.concatenate([P[:1], P[:1], P[:7], P[6:7], P[6:7], P[6:], P[-1:]])   # the start twice more, waypoint 6 three times, the end twice
    a = rr.retime_row(P, c["vmax"], c["amax"], rc.DT, 300)
    b = rr.retime_row(rep, c["vmax"], c["amax"], rc.DT, 300)
    kept = rr.compact(rep)
    assert len(kept) == 20 and a["status"] == b["status"] == rr.OK
    assert np.array_equal(b["x"][kept], a["x"]) and np.array_equal(b["t"][kept], a["t"]) and b["duration"] == a["duration"]
    assert np.array_equal(b["samples"], a["samples"]) and np.array_equal(b["sample_vel"], a["sample_vel"])
    assert b["x"][1] == b["x"][0] and b["t"][10] == b["t"][8] and b["t"][-1] == b["t"][-2], "a dropped waypoint repeats the waypoint kept before it"
    # extra rows of dropped waypoints are ignored, NaN included
    E = 2
    ex = [np.full((len(rep), E), v, np.float32) for v in (0.3, 0.01, -5.0, 5.0)]
    exk = tuple(e[kept] for e in ex)
    for e in ex:
        e[[1, 2, 10]] = np.nan
    assert 1 not in kept and 2 not in kept and 10 not in kept
    with_nan = rr.retime_row(rep, c["vmax"], c["amax"], rc.DT, 0, None, tuple(ex), want_samples=False)
    clean = rr.retime_row(P, c["vmax"], c["amax"], rc.DT, 0, None, exk, want_samples=False)
    assert with_nan["status"] == rr.OK and with_nan["duration"] == clean["duration"]


def test_statuses():
    c = rc.case("acc")
    P = c["paths"][1][:12].copy()
    lim = (c["vmax"], c["amax"], rc.DT)
    still = rr.retime_row(np.tile(P[:1], (6, 1)), *lim, 5)
    assert still["status"] == rr.NO_MOTION and still["duration"] == 0 and still["n_samples"] == 1 and np.array_equal(still["samples"], np.tile(P[0], (5, 1)))
    two = rr.retime_row(np.concatenate([P[:1], P[:1], P[5:6]]), *lim, 5)
    assert two["status"] == rr.TOO_FEW_WAYPOINTS and two["duration"] == 0 and np.array_equal(two["samples"], np.tile(P[0], (5, 1))) and (two["x"] == 0).all()
    for bad in (np.nan, np.inf):
        Q = P.copy()
        Q[7, 3] = bad
        o = rr.retime_row(Q, *lim, 5)
        assert o["status"] == rr.NOT_FINITE and np.array_equal(o["samples"], np.tile(P[0], (5, 1)))
    ex = [np.full((12, 1), v, np.float32) for v in (0.3, 0.01, -5.0, 5.0)]
    ex[2][4] = 0.0   # lo >= 0: rest is not strictly feasible
    assert rr.retime_row(P, *lim, 5, None, tuple(ex))["status"] == rr.INFEASIBLE
    ex[2][4] = np.nan
    assert rr.retime_row(P, *lim, 5, None, tuple(ex))["status"] == rr.NOT_FINITE
    full = rr.retime_row(P, *lim, 400)
    cut = rr.retime_row(P, *lim, 17)
    assert full["status"] == rr.OK and cut["status"] == rr.TRUNCATED and cut["n_samples"] == full["n_samples"] > 17
    assert np.array_equal(cut["samples"], full["samples"][:17]) and np.array_equal(cut["x"], full["x"]) and cut["duration"] == full["duration"]


# ---- the conditions the GPU tier leans on
@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_float32_port_stays_near_the_reference(name):
    ref, port = rc.reference(name), rc.reference(name, "float32")
    tol, line = rc.yardstick(name)
    print("\n" + line)
    assert np.array_equal(ref["status"], port["status"]) and (np.abs(ref["n_samples"] - port["n_samples"]) <= 1).all()
    # a yardstick of the outputs' own size would show nothing: the port's error stays below 1e-4 of the scale (float32 carries 6e-8;
    # a chain of 100 intervals and a square root at a waypoint where the path nearly stops leave three orders of magnitude)
    assert tol["x"] <= 4e-4 * ref["x"].max() and tol["duration"] <= 4e-4 * ref["duration"].max() and tol["t"] <= 4e-4 * ref["duration"].max()
    c = rc.case(name)
    for r in range(rc.R):
        ex = None if c["extra"] is None else tuple(e[r] for e in c["extra"])
        rows, cap = rr.row_violation(c["paths"][r], port["x"][r], c["vmax"], c["amax"], 1.0 / rc.DT, ex)
        assert rows <= 1e-5 and cap <= 1e-5, (name, r, rows, cap)
    for K, want in rc.KNOWN.items():
        assert abs(float(rc.known(K, "float32")["duration"]) - want) <= 1e-5


def test_torque_rows_bind():
    P, ex, tmax = rc.torque_rows()
    lim = ([rc.TORQUE_VMAX] * 9, [rc.TORQUE_AMAX] * 9, rc.DT)
    free = rr.retime_row(P, *lim, want_samples=False)
    bound = rr.retime_row(P, *lim, 0, None, ex, want_samples=False)
    print(f"\n[retime, torque] tmax {tmax:.2f} N m: duration {free['duration']:.4f} s without the rows, {bound['duration']:.4f} s with them")
    assert free["status"] == bound["status"] == rr.OK and bound["duration"] >= 1.05 * free["duration"]
    assert (ex[2] < 0).all() and (ex[3] > 0).all(), "gravity alone stays inside the limits"
    rows, _ = rr.row_violation(P, bound["x"], *lim[:2], 1.0 / rc.DT, ex)
    assert rows <= 1e-12


# ---- EntityView.retime_path against a stub scene
class StubScene:
    """what EntityView.retime_path reads of a MirScene, answered by the reference; dynamics() is a made-up linear model,
    tau = 2 qacc + 3 qvel^2 + 5 qpos over the first nv columns (linear in the acceleration, quadratic in the velocity, as inverse dynamics are), so that the torque rows show which m and c they were built from"""

    def __init__(self, B, dtype=np.float64):
        self.num_envs, self.device, self.nv, self.nq, self.calls, self.dtype = B, torch.device("cpu"), 15, 16, [], dtype
        self.q0 = torch.arange(B * 16, dtype=torch.float32).reshape(B, 16) * 0.01

    def get_state(self):
        return self.q0, torch.zeros((self.num_envs, self.nv)), None, None

    def dynamics(self, env_idx=None, dof0=0, n_dofs=None, qacc=None, qpos=None, qvel=None, **flags):
        assert flags.get("tau") and not flags.get("mass")
        tau = 2.0 * qacc + 3.0 * qvel * qvel + 5.0 * qpos[:, :self.nv]
        return {"tau": tau[:, dof0:dof0 + n_dofs]}

    def retime_path(self, paths, vmax, amax, dt, num_samples=0, max_path_speed=None, extra=None, velocity=False):
        self.calls.append(dict(paths=paths.clone(), vmax=vmax, amax=amax, dt=dt, T=num_samples, extra=extra, velocity=velocity))
        ex = None if extra is None else tuple(e.numpy() for e in extra)
        o = rr.retime(paths.numpy(), vmax, amax, dt, num_samples, max_path_speed, ex, self.dtype, num_samples > 0)
        out = {k: torch.as_tensor(np.asarray(o[k], np.int32 if k in ("status", "n_samples") else np.float32)) for k in ("x", "t", "duration", "status", "n_samples")}
        if num_samples > 0:
            out["samples"] = torch.as_tensor(o["samples"].astype(np.float32))
            if velocity:
                out["sample_vel"] = torch.as_tensor(o["sample_vel"].astype(np.float32))
        return out


def _robot(B):
    sb = models.franka_cube_pick_scene()
    sc = StubScene(B)
    return EntityView(sc, sb, "link0", models.FRANKA_JOINTS), sc, sb


def test_entity_view_layouts_and_sizing():
    c = rc.case("acc")
    robot, sc, sb = _robot(rc.R)
    paths = c["paths"][:, :24]
    path = torch.as_tensor(paths.transpose(1, 0, 2).copy())   # (K, R, n), as plan_path returns it
    out = robot.retime_path(path, 2.0, np.full(9, 3.0))
    first, second = sc.calls
    assert first["T"] == 0 and np.array_equal(first["paths"].numpy(), paths) and first["vmax"] == [2.0] * 9 and first["amax"] == [3.0] * 9
    assert first["dt"] == sb.opt["dt"] and first["extra"] is None
    ref = rr.retime(paths, c["vmax"], c["amax"], sb.opt["dt"], 0, want_samples=False)
    T = int(ref["n_samples"].max())
    assert second["T"] == T and tuple(out.shape) == (T, rc.R, 9), "the second launch is sized to the longest row"
    assert torch.equal(out[0], path[0]) and torch.equal(out[-1], path[-1])
    det = robot.retime_path(path, 2.0, 3.0, dt=0.02, num_samples=50, return_detail=True)
    assert len(sc.calls) == 3 and sc.calls[-1]["T"] == 50 and sc.calls[-1]["velocity"] and sc.calls[-1]["dt"] == 0.02, "an explicit num_samples is one launch"
    assert sorted(det) == ["duration", "n_samples", "samples", "status", "t", "valid", "velocity", "x"]
    assert det["samples"].shape == det["velocity"].shape == (50, rc.R, 9) and det["t"].shape == (rc.R, 24) and det["valid"].dtype == torch.bool
    assert (det["status"] == rr.TRUNCATED).all() and not det["valid"].any()
    # envs_idx: the rows of the call
    sub = robot.retime_path(path[:, [3, 1]], 2.0, 3.0, envs_idx=[3, 1], num_samples=T)
    assert torch.equal(sub, out[:, [3, 1]])
    # a row that does not move comes back as its start, and is valid
    still = path.clone()
    still[:, 2] = still[0, 2]
    d = robot.retime_path(still, 2.0, 3.0, return_detail=True)
    assert d["status"][2] == rr.NO_MOTION and d["valid"].all() and (d["samples"][:, 2] == still[0, 2]).all() and d["duration"][2] == 0


def test_entity_view_refine():
    c = rc.case("acc")
    robot, sc, _ = _robot(rc.R)
    path = torch.as_tensor(c["paths"][:, :5].transpose(1, 0, 2).copy())
    robot.retime_path(path, 2.0, 3.0, refine=3, num_samples=10)
    sent = sc.calls[-1]["paths"].numpy()
    assert sent.shape == (rc.R, 13, 9)
    for r in range(rc.R):
        assert np.array_equal(sent[r], rr.refine(c["paths"][r, :5], 3))
    assert np.array_equal(sent[:, ::3], c["paths"][:, :5]), "the caller's waypoints keep their bits"
    two = path[[0, 4]]
    with pytest.raises(ValueError, match="refine"):
        robot.retime_path(two, 2.0, 3.0)
    d = robot.retime_path(two, 2.0, 3.0, refine=2, return_detail=True)
    assert d["valid"].all() and d["t"].shape == (rc.R, 3)


def test_entity_view_torque_rows_use_the_kept_waypoints():
    c = rc.case("acc")
    robot, sc, _ = _robot(2)
    P = c["paths"][0][:8]
    rep = np.concatenate([P[:1], P[:4], P[3:4], P[3:], P[-1:]])   # K = 12 with three repeated waypoints
    path = torch.as_tensor(np.stack([rep, np.concatenate([c["paths"][1][:11], c["paths"][1][10:11]])], 1))
    tmax = np.linspace(20.0, 60.0, 9).astype(np.float32)
    robot.retime_path(path, 2.0, 3.0, torque_limits=tmax, num_samples=10, envs_idx=[1, 0])
    ea, eb, elo, ehi = (e.numpy().astype(np.float64) for e in sc.calls[-1]["extra"])
    for r, env in enumerate((1, 0)):
        Pr = path[:, r].numpy()
        kept = rr.compact(Pr)
        m, cc = rr.compact_differences(Pr)
        g = 5.0 * Pr.astype(np.float64)   # the stub's ID(q, 0, 0) over the arm's columns (qpos columns 0 .. 8 are the arm's)
        assert np.abs(ea[r][kept] - 2.0 * m[kept]).max() <= 1e-5 and np.abs(eb[r][kept] - (2.0 * cc + 3.0 * m * m)[kept]).max() <= 1e-5
        assert np.abs(elo[r] - (-tmax - g)).max() <= 1e-4 and np.abs(ehi[r] - (tmax - g)).max() <= 1e-4
    assert all(np.isfinite(e).all() for e in (ea, eb, elo, ehi))
    lo, hi = robot.get_dofs_force_range()
    assert lo.shape == hi.shape == (9,) and (lo < 0).all() and torch.equal(hi, -lo)
    assert torch.equal(robot.get_dofs_force_range([7, 0])[1], hi[[7, 0]])
    robot.retime_path(path, 2.0, 3.0, torque_limits=True, num_samples=10, envs_idx=[1, 0])
    assert np.allclose(sc.calls[-1]["extra"][3].numpy()[0], hi.numpy()[None] - 5.0 * path[:, 0].numpy(), atol=1e-4)


def test_entity_view_refusals_and_unbatched():
    c = rc.case("acc")
    robot, sc, _ = _robot(rc.R)
    path = torch.as_tensor(c["paths"][:, :6].transpose(1, 0, 2).copy())
    for kw in (dict(max_velocity=0.0), dict(max_velocity=[1.0, 2.0]), dict(max_acceleration=float("nan")), dict(dt=0.0), dict(refine=0),
               dict(num_samples=0), dict(torque_limits=[1.0, 2.0])):
        args = dict(max_velocity=2.0, max_acceleration=3.0)
        args.update(kw)
        with pytest.raises(ValueError):
            robot.retime_path(path, **args)
    for bad in (path[:, :3], path[:, :, :8], path[:1]):
        with pytest.raises(ValueError, match="path must be"):
            robot.retime_path(bad, 2.0, 3.0)
    with pytest.raises(IndexError):
        robot.retime_path(path[:, :1], 2.0, 3.0, envs_idx=[rc.R])
    slow = robot.retime_path   # a row so slow that the sized result would not fit: refused before it is allocated
    sc.retime_path = lambda paths, **kw: {"n_samples": torch.full((rc.R,), 2_000_000_001, dtype=torch.int32)}
    with pytest.raises(ValueError, match="2\\^31"):
        slow(path, 2.0, 3.0)
    del sc.retime_path
    cube = EntityView(sc, models.franka_cube_pick_scene(), "cube", ())
    with pytest.raises(NotImplementedError):
        cube.retime_path(path, 2.0, 3.0)
    single, s1, _ = _robot(1)
    single.unbatched = True
    got = single.retime_path(path[:, 0], 2.0, 3.0)
    det = single.retime_path(path[:, 0], 2.0, 3.0, return_detail=True)
    assert got.dim() == 2 and got.shape[1] == 9 and torch.equal(got, det["samples"]) and det["duration"].dim() == 0 and det["t"].shape == (6,)
    assert bool(det["valid"]) and det["velocity"].shape == got.shape


# ---- the host checks, through the g++ build
@pytest.fixture(scope="module")
def host():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "gym-genesis_amd", "csrc"), "retime-host"], stdout=subprocess.DEVNULL)
    lib = C.CDLL(os.path.join(ROOT, "tests", "_build", "libmirretime.so"))
    lib.retime_host_check.argtypes = [C.POINTER(S.MirRetimeQuery), C.c_int, C.c_uint, C.c_int, C.c_char_p]
    return lib


ALL, NO_SAMPLES, NO_EXTRA = 0x1fff, 0x7ff, 0x1fff & ~0x3c   # the `present` bits of tests/retime_host.cpp


def _check(host, q, n_rows=5, present=ALL, step_open=0):
    what = C.create_string_buffer(128)
    rc_ = host.retime_host_check(None if q is None else C.byref(q), n_rows, present, step_open, what)
    return rc_, what.value.decode()


def test_host_checks(host):
    INVALID, CAPACITY = -1, -2
    good = lambda **kw: S.make_retime_query(kw.pop("D", 9), kw.pop("K", 100), kw.pop("vmax", 2.0), kw.pop("amax", 3.0), kw.pop("dt", 0.01),  # noqa: E731
                                            kw.pop("T", 500), kw.pop("vs", None), kw.pop("E", 9))
    assert host.retime_host_query_sizeof() == C.sizeof(S.MirRetimeQuery)
    assert _check(host, good()) == (0, "") and _check(host, good(E=0), present=NO_EXTRA) == (0, "")
    assert _check(host, good(T=0), present=NO_SAMPLES) == (0, "") and _check(host, good(D=16, E=16)) == (0, "") and _check(host, good(), n_rows=0) == (0, "")
    assert _check(host, good(K=S.RETIME_MAX_WAYPOINTS, T=1)) == (0, "")
    assert _check(host, None) == (INVALID, "null argument")
    for bit in (0, 1, 6, 7, 8, 9, 10):   # handle, paths, x, t, duration, status, n_samples
        assert _check(host, good(), present=ALL & ~(1 << bit)) == (INVALID, "null argument"), bit
    for bit in (2, 3, 4, 5):
        assert _check(host, good(), present=ALL & ~(1 << bit)) == (INVALID, "n_extra > 0 with a null extra array"), bit
    q = good(); q.struct_size -= 4
    assert _check(host, q)[0] == INVALID and "struct_size" in _check(host, q)[1]
    assert _check(host, good(K=1)) == (INVALID, "num_waypoints < 2")
    for D in (0, 17, -1):
        q = good(); q.n_dofs = D
        assert _check(host, q) == (INVALID, "n_dofs outside 1 .. 16")
    q = good(); q.n_extra = -1
    assert _check(host, q) == (INVALID, "negative n_extra")
    assert _check(host, good(), n_rows=-1) == (INVALID, "negative n_rows")
    q = good(); q.num_samples = -1
    assert _check(host, q) == (INVALID, "negative num_samples")
    q = good(); q.flags = 1
    assert _check(host, q) == (INVALID, "unknown flag bit")
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        q = good(); q.vmax[8] = bad
        assert _check(host, q) == (INVALID, "vmax must be finite and > 0"), bad
        q = good(); q.amax[0] = bad
        assert _check(host, q) == (INVALID, "amax must be finite and > 0"), bad
        q = good(); q.dt = bad
        assert _check(host, q) == (INVALID, "dt must be finite and > 0"), bad
        q = good(); q.max_path_speed = bad
        assert _check(host, q) == (INVALID, "max_path_speed must be finite and > 0"), bad
    q = good(); q.vmax[9] = -1.0   # (behind the first D: not read)
    assert _check(host, q) == (0, "")
    for present in (ALL, ALL & ~(1 << 11), ALL & ~(1 << 12)):
        assert _check(host, good(T=0), present=present) == (INVALID, "samples or sample_vel with num_samples < 1")
    assert _check(host, good(), step_open=1) == (INVALID, "a step is pending (mir_step_end first)")
    for D, E in ((16, 17), (9, 24), (1, 32)):
        rc_, what = _check(host, good(D=D, E=E))
        assert rc_ == CAPACITY and "64" in what, (D, E)
    assert _check(host, good(D=1, E=31)) == (0, "")
    rc_, what = _check(host, good(K=S.RETIME_MAX_WAYPOINTS + 1))
    assert rc_ == CAPACITY and "MIR_RETIME_MAX_WAYPOINTS" in what
    assert _check(host, good(D=16, E=0, T=2 ** 20), n_rows=127, present=NO_EXTRA) == (0, "")      # 127 x 2^20 x 16 = 2^31 - 2^24
    rc_, what = _check(host, good(D=16, E=0, T=2 ** 20), n_rows=128, present=NO_EXTRA)             # 2^31
    assert rc_ == CAPACITY and "2^31" in what
    assert S.RETIME_STATUS == rr.STATUS and S.RETIME_MAX_WAYPOINTS == rr.MAX_WAYPOINTS
