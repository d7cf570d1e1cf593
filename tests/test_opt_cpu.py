"""Trajectory optimisation without a device (include/mirigid.h: mir_optimize_path): known answers of the float64 reference
(tests/opt_ref.py), the scalar half of the entry point (gym-genesis_amd/csrc/mir_opt_front.h through `make opt-host`) bit for bit
against the float32 port, the conditions the GPU tests of tests/test_gpu_opt.py lean on, and what the optimiser buys over the detour
round the post.  If a condition fails for an input, the input changes, not the condition.

1. Known answers: `line` is the straight line at equal spacing; c and c' are continuous at 0 and at eps; the analytic dc_p / dq_j agrees
   with central differences of plan_ref.Problem.centres; the gradient of U agrees with central differences of U; U never rises from
   one accepted iterate to the next; the ends never move.
2. The host half, bit for bit: the constants and the pivot table, c, c', the Thomas recurrence, the cost and gradient assembly, the
   accept and stop decisions, every refusal with its text.
3. The conditions, for reference and port alike, on every row of every case: a probe inside the band has its runner-up geom >= 1 mm
   behind the winner; every decision of the line search is decided by >= 1e-4 of U or by >= 1e-4 rad; every swept configuration by
   >= 1 mm; every quotient under a ceil lies >= 1e-3 from an integer; reference and port agree on status, stop and every count.
4. What it buys, float64: the planner's path, the same blended, the same optimised.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import blend_ref
import opt_cases as oc
import opt_ref
import plan_cases as pc
import plan_ref
import retime_ref
from gym_genesis.backend import spec as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = range(oc.B)
f32 = np.float32


def _pair(name, r, **kw):
    return oc.reference(name, r, "float64", **kw), oc.reference(name, r, "float32", **kw)


# ---- 1. known answers
def test_line_is_the_straight_line_at_equal_spacing():
    for r in ROWS:
        for o in _pair("line", r):
            P = np.asarray(o["path"], np.float64)
            K = len(P)
            want = P[0] + (np.arange(K) / (K - 1))[:, None] * (P[-1] - P[0])
            assert o["status"] == opt_ref.OK and tuple(o["stats"][:3]) == (1, 1, 0), o["stats"]
            assert np.abs(P - want).max() <= (1e-12 if P.dtype == np.float64 and o["reached"].dtype == np.float64 else 4e-6), np.abs(P - want).max()
            assert abs(float(o["cost"][2]) - 0.5 * ((P[-1] - P[0]) ** 2).sum()) <= 1e-6, "S of a straight line is |b - a|^2 / 2 whatever K"


def test_cost_is_c1():
    """c and c' are continuous at 0 and at eps: the one-sided values an ulp-sized step apart differ by no more than the slope allows"""
    eps = 0.05
    for dt, h, tol in ((np.float64, 1e-9, 1e-12), (np.float32, 1e-6, 1e-6)):
        for x, cv, dv in ((0.0, eps / 2, -1.0), (eps, 0.0, 0.0)):
            for s in (-h, 0.0, h):
                assert abs(float(opt_ref.c(x + s, eps, dt)) - cv) <= 2 * h + tol, (dt, x, s)
                assert abs(float(opt_ref.dc(x + s, eps, dt)) - dv) <= 2 * h / eps + tol, (dt, x, s)
        assert float(opt_ref.c(2 * eps, eps, dt)) == 0.0 and float(opt_ref.dc(2 * eps, eps, dt)) == 0.0
        assert abs(float(opt_ref.c(eps / 2, eps, dt)) - eps / 8) <= tol and abs(float(opt_ref.dc(eps / 2, eps, dt)) + 0.5) <= 10 * tol
        assert abs(float(opt_ref.c(-0.01, eps, dt)) - (0.01 + eps / 2)) <= tol and float(opt_ref.dc(-0.01, eps, dt)) == -1.0


def test_jacobian_agrees_with_central_differences():
    rng = np.random.default_rng(5)
    for name in ("over_post", "carry"):
        c = oc.case(name)
        pb = oc.problem(name)
        pb.set_row(c["q"][0])
        ch = opt_ref.Chains(pb)
        N = getattr(pb, "N", len(pb.probes))
        worst = 0.0
        for _ in range(3):
            q = np.array([rng.uniform(lo + 0.1 * (hi - lo), hi - 0.1 * (hi - lo)) for lo, hi in zip(pb.lo, pb.hi)])
            pw = pb.centres(q).copy()
            J = opt_ref.jacobians(pb, ch, pw[:N]).copy()
            for j in range(pb.D):
                e = np.zeros(pb.D)
                e[j] = 1e-6
                fd = (pb.centres(q + e)[:N] - pb.centres(q - e)[:N]) / 2e-6
                worst = max(worst, float(np.abs(fd - J[:, j]).max()))
        print(f"[opt, {name}] analytic Jacobian against central differences: {worst:.3e}")
        assert worst <= 1e-8, (name, worst)


def _U(pb, ch, P, par, k):
    return float(opt_ref.evaluate(pb, ch, P, par, k)["U"])


@pytest.mark.parametrize("name", ("pushed_out", "carry"))
def test_gradient_agrees_with_central_differences(name):
    c = oc.case(name)
    pb = oc.problem(name)
    pb.set_row(c["q"][0])
    ch = opt_ref.Chains(pb)
    P = c["paths"][0].astype(np.float64)
    K, D = P.shape
    par = dict(margin=np.float64(f32(c["margin"])), smooth_weight=1.0, obstacle_weight=c["par"]["obstacle_weight"], activation=np.float64(f32(c["par"]["activation"])),
               ignore=False)
    k = opt_ref.consts(K, np.float64)
    log = dict(gap=np.inf)
    base = opt_ref.evaluate(pb, ch, P, par, k, log)
    assert log["gap"] >= 1e-4 and float(base["O"]) > 0, (log, base["O"])
    worst, big = 0.0, float(np.abs(base["g"]).max())
    for i in range(1, K - 1):
        for j in range(7):
            e = np.zeros((K, D))
            e[i, j] = 1e-6
            fd = (_U(pb, ch, P + e, par, k) - _U(pb, ch, P - e, par, k)) / 2e-6
            worst = max(worst, abs(fd - float(base["g"][i, j])))
    print(f"[opt, {name}] gradient of U against central differences: {worst:.3e} (largest |g| {big:.3f})")
    assert worst <= 1e-5 * max(big, 1.0), (name, worst, big)
    assert not base["g"][0].any() and not base["g"][-1].any()


@pytest.mark.parametrize("name", oc.NAMES)
def test_U_never_rises_and_the_ends_never_move(name):
    c = oc.case(name)
    for r in ROWS:
        for o in _pair(name, r):
            U = [float(u) for u in o["U"]]
            assert all(b < a for a, b in zip(U[:-1], U[1:])), (name, r, U)
            for P in (o["path"], o["reached"]):
                assert np.array_equal(np.asarray(P[[0, -1]], f32), c["paths"][r][[0, -1]]) or o["status"] == opt_ref.NOT_FINITE
            if o["status"] != opt_ref.OK:
                assert np.asarray(o["path"], f32).tobytes() == c["paths"][r].tobytes(), "a row that is not OK returns its input"
            elif o["stats"][1] > 0:
                lo, hi = oc.problem(name).lo, oc.problem(name).hi
                assert ((o["path"][1:-1] >= lo) & (o["path"][1:-1] <= hi)).all()
                assert float(o["cost"][2]) + c["par"]["obstacle_weight"] * float(o["cost"][3]) < float(o["cost"][0]) + c["par"]["obstacle_weight"] * float(o["cost"][1])


# ---- 2. the host half
@functools.lru_cache(maxsize=None)
def _host():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "gym-genesis_amd", "csrc"), "opt-host"], stdout=subprocess.DEVNULL)
    lib = C.CDLL(os.path.join(ROOT, "tests", "_build", "libmiropt.so"))
    f, fp = C.c_float, C.POINTER(C.c_float)
    lib.opt_host_check.argtypes = [C.POINTER(S.MirOptQuery), C.c_uint, C.c_int, f, f, C.c_longlong, C.c_int, C.c_char_p]
    lib.opt_host_consts.argtypes = [C.c_int, fp, fp]
    lib.opt_host_consts.restype = None
    for name, n in (("c", 2), ("dc", 2), ("s_add", 3), ("U", 6), ("grad", 8)):
        fn = getattr(lib, "opt_host_" + name)
        fn.argtypes, fn.restype = [f] * n, f
    for name, n in (("outside", 3), ("accept", 2), ("converged", 3)):
        getattr(lib, "opt_host_" + name).argtypes = [f] * n
    lib.opt_host_column.argtypes = [fp, fp, C.c_int, f, fp]
    lib.opt_host_column.restype = None
    return lib


def _bits(x):
    return np.asarray(x, f32).tobytes()


def test_host_constants_and_scalar_rules_match_the_port_bit_for_bit():
    host = _host()
    assert host.opt_host_query_sizeof() == C.sizeof(S.MirOptQuery)
    fp = C.POINTER(C.c_float)
    for K in (3, 4, 8, 12, 16, 127, 128):
        out3, rp = np.zeros(3, f32), np.zeros(max(K - 2, 1), f32)
        host.opt_host_consts(K, out3.ctypes.data_as(fp), rp.ctypes.data_as(fp))
        k = opt_ref.consts(K, f32)
        assert _bits(out3) == _bits([k["km1"], k["hk"], k["ik"]]) and _bits(rp[:K - 2]) == _bits(k["rpiv"]), K
        assert _bits(k["rpiv"]) == _bits([i / (i + 1) for i in range(1, K - 1)]), "the pivots of tridiag(-1, 2, -1) are (i + 1) / i"
    rng = np.random.default_rng(11)
    for eps in (0.05, 0.1, 0.013):
        for d in np.concatenate([rng.uniform(-0.2, 0.3, 200), [0.0, eps, -0.0, float(f32(eps)), np.nextafter(f32(eps), f32(1))]]).astype(f32):
            assert _bits(host.opt_host_c(d, eps)) == _bits(opt_ref.c(d, f32(eps), f32)), (d, eps)
            assert _bits(host.opt_host_dc(d, eps)) == _bits(opt_ref.dc(d, f32(eps), f32)), (d, eps)
    for K in (3, 5, 12, 128):
        n = K - 2
        k = opt_ref.consts(K, f32)
        for _ in range(5):
            g, q, alpha = rng.normal(0, 3, n).astype(f32), rng.uniform(-2, 2, n).astype(f32), f32(rng.uniform(0.01, 2))
            out = np.zeros(n, f32)
            host.opt_host_column(g.ctypes.data_as(fp), q.ctypes.data_as(fp), K, alpha, out.ctypes.data_as(fp))
            assert _bits(out) == _bits(opt_ref.candidate_column(g, q, k, alpha, f32)), K
            # the recurrence solves M delta = g in float64 to rounding
            M = (K - 1) * (2 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1))
            want = q.astype(np.float64) - float(alpha) * np.linalg.solve(M, g.astype(np.float64))
            assert np.abs(opt_ref.candidate_column(g, q, opt_ref.consts(K, np.float64), alpha, np.float64) - want).max() <= 1e-9
        v = rng.normal(0, 1, (40, 8)).astype(f32)
        for a in v:
            args = [float(x) for x in a]
            assert _bits(host.opt_host_grad(*args[:4], args[4], args[5], float(k["km1"]), float(k["ik"]))) == _bits(
                opt_ref.grad_value(a[0], a[1], a[2], a[3], a[4], a[5], k, f32))
            assert _bits(host.opt_host_s_add(*args[:3])) == _bits(f32(a[0] + f32(f32(a[1] - a[2]) * f32(a[1] - a[2]))))
            S_, O_ = f32(k["hk"] * abs(a[0])), f32(k["ik"] * abs(a[1]))
            assert _bits(host.opt_host_U(abs(args[2]), float(k["hk"]), abs(args[0]), abs(args[3]), float(k["ik"]), abs(args[1]))) == _bits(
                opt_ref.total(abs(a[2]), S_, abs(a[3]), O_, f32))
    for U, Un, ftol in ((1.0, 0.5, 0.1), (1.0, 0.95, 0.1), (1.0, 1.0, 0.0), (1.0, np.nextafter(f32(1), f32(0)), 0.0), (1.0, np.inf, 0.0), (1.0, np.nan, 0.0),
                        (np.inf, 1.0, 0.0), (2.0, 1.9999, 1e-4)):
        assert bool(host.opt_host_accept(Un, U)) == opt_ref.accept(f32(Un), f32(U)), (U, Un)
        if np.isfinite(Un):
            assert bool(host.opt_host_converged(U, Un, ftol)) == opt_ref.converged(f32(U), f32(Un), ftol, f32), (U, Un, ftol)
    assert host.opt_host_outside(1.0, 0.0, 1.0) == 0 and host.opt_host_outside(float(np.nextafter(f32(1), f32(2))), 0.0, 1.0) == 1
    assert host.opt_host_outside(float("nan"), 0.0, 1.0) == 1 and host.opt_host_outside(-1e-9, 0.0, 1.0) == 1


def test_every_refusal_with_its_text():
    host = _host()
    ALL = 0x7f

    def check(q, present=ALL, K=None, margin=0.0, max_distance=1.0, n=57, self_=0):
        what = C.create_string_buffer(128)
        rc = host.opt_host_check(C.byref(q) if q is not None else None, present, q.num_waypoints if K is None and q is not None else (K or 0), margin,
                                 max_distance, n, self_, what)
        return rc, what.value.decode()

    good = lambda K=12, **kw: S.make_opt_query(K, **kw)  # noqa: E731
    assert check(good()) == (0, "")
    assert check(good(3)) == (0, "") and check(good(128)) == (0, "")
    for bit in range(7):
        assert check(good(), ALL & ~(1 << bit)) == (-1, "null argument"), bit
    assert check(None, K=12) == (-1, "null argument")
    q = good()
    q.struct_size += 4
    assert check(q) == (-1, "struct_size is not sizeof(MirOptQuery)")
    for K in (2, 0, -1, 129):
        assert check(good(K)) == (-1, "num_waypoints outside 3 .. MIR_PLAN_MAX_POLY"), K
    assert check(good(12), K=11) == (-1, "K is not num_waypoints")
    q = good()
    q.flags = 1
    assert check(q) == (-1, "unknown flag bit in MirOptQuery")
    for key in ("smooth_weight", "obstacle_weight", "step", "activation", "ftol"):
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert check(good(**{key: bad})) == (-1, "a weight, step, activation or ftol is not finite"), (key, bad)
    assert check(good(smooth_weight=0.0)) == (-1, "smooth_weight must be > 0") == check(good(smooth_weight=-1.0))
    assert check(good(obstacle_weight=-1e-3)) == (-1, "obstacle_weight must be >= 0") and check(good(obstacle_weight=0.0)) == (0, "")
    assert check(good(step=0.0)) == (-1, "step must be > 0") == check(good(step=-0.5))
    assert check(good(activation=0.0)) == (-1, "activation must be > 0")
    assert check(good(ftol=-1e-6)) == (-1, "ftol must be >= 0") and check(good(ftol=0.0)) == (0, "")
    assert check(good(max_iterations=-1)) == (-1, "negative max_iterations or max_halvings") == check(good(max_halvings=-1))
    assert check(good(max_iterations=0, max_halvings=0)) == (0, "")
    assert check(good(activation=0.05), margin=0.96, max_distance=1.0) == (-1, "max_distance < margin + activation")
    assert check(good(activation=0.05), margin=0.95, max_distance=1.0 + 1e-6) == (0, "")
    text = "the path and gradient buffers and the sphere list do not fit 64 KB of LDS (num_waypoints, n_probes + n_extra)"
    assert check(good(128), n=1024, self_=1) == (0, "")     # 14368 + 24576 + 16384 bytes
    assert check(good(128), n=1700, self_=1) == (-2, text) and check(good(128), n=1700, self_=0) == (0, "")


def test_the_entity_view_spells_out_the_defaults():
    import inspect

    from gym_genesis.tasks.views import EntityView

    sig = inspect.signature(EntityView.optimize_path)
    assert all(sig.parameters[k].default == v for k, v in S.OPT_DEFAULTS.items()), S.OPT_DEFAULTS
    q = S.make_opt_query(16)
    assert (q.num_waypoints, q.max_iterations, q.max_halvings) == (16, S.OPT_DEFAULTS["max_iterations"], S.OPT_DEFAULTS["max_halvings"])
    assert S.OPT_STATUS[S.OPT_BLOCKED] == "BLOCKED" and S.OPT_STOP[S.OPT_STOP_STALLED] == "STALLED"


# ---- 3. the conditions the GPU tier leans on
@pytest.mark.parametrize("name", oc.NAMES)
def test_conditions_of_the_gpu_tier(name):
    c = oc.case(name)
    for r in ROWS:
        a, b = _pair(name, r)
        assert a["status"] == b["status"] and a["stop"] == b["stop"] and list(a["stats"]) == list(b["stats"]), (name, r, a["stats"], b["stats"])
        for o in (a, b):
            lg = o["log"]
            assert lg["gap"] >= 1e-3, (name, r, lg["gap"])
            for d in lg["decisions"]:
                assert d[1] >= 1e-4, (name, r, d)
                if d[0] != "limit":
                    assert d[2] >= 1e-4, (name, r, d, "an evaluated candidate lies inside the limits by 1e-4 rad")
            for sc, sf in lg["sweep"]:
                assert abs(sc) >= 1e-3 and abs(sf) >= 1e-3, (name, r, sc, sf)
            for qt in lg["quotients"]:
                assert min(qt - np.floor(qt), np.ceil(qt) - qt) >= 1e-3 or qt == 0.0, (name, r, qt)
    ref = [oc.reference(name, r) for r in ROWS]
    status = [o["status"] for o in ref]
    print(f"[opt, {name}] status {status} stop {[o['stop'] for o in ref]} stats {[[int(v) for v in o['stats'][:5]] for o in ref]}")
    want = {"not_finite": [0, 0, opt_ref.NOT_FINITE, 0, 0], "no_motion": [opt_ref.NO_MOTION, 0, 0, 0, 0], "out_of_limits": [0, 0, 0, opt_ref.OUT_OF_LIMITS, 0],
            "thin": [opt_ref.BLOCKED] * 5}.get(name, [0] * 5)
    assert status == want, (name, status)
    if name == "free":
        assert all(o["stop"] == opt_ref.STOP_CONVERGED and float(o["cost"][1]) == 0.0 == float(o["cost"][3]) for o in ref)
        assert all(np.array_equal(o["grad0"], opt_ref.evaluate(oc.problem(name), opt_ref.Chains(oc.problem(name)), c["paths"][r].astype(np.float64),
                                                               dict(margin=0.0, smooth_weight=1.0, obstacle_weight=0.0, activation=0.05, ignore=True),
                                                               opt_ref.consts(oc.K_OF[name], np.float64))["g"]) for r, o in enumerate(ref)), "the smoothness term alone"
    elif name == "limits":
        assert all(o["log"]["decisions"][0][0] == "limit" and o["log"]["decisions"][1][0] == "accept" for o in ref)
    elif name == "pushed_out":
        for r, o in enumerate(ref):
            pb = oc.problem(name)
            pb.set_row(c["q"][r])
            low = min(float(pb.clearance(w.astype(np.float64))) for w in c["paths"][r][1:-1]) - c["margin"]
            assert -5e-3 <= low <= -1e-3 and float(o["min_d"]) >= 1e-3, (r, low, o["min_d"])
    elif name == "thin":
        for r in ROWS:
            for o in _pair(name, r, skip_thin=True):
                assert o["status"] == opt_ref.OK and all(abs(sc) >= 1e-3 for sc, _ in o["log"]["sweep"]), (r, o["status"])
    elif name == "ignore":
        for r, o in enumerate(ref):
            assert o["stats"][3] == 0 and o["stats"][4] == 0 and float(o["cost"][1]) == 0.0
    elif name in ("over_post", "self_on", "carry"):
        assert all(float(o["cost"][1]) > 0 and o["stats"][1] >= 2 for o in ref), "the obstacle cost is in play and steps are accepted"


# ---- 4. what it buys
PAYOFF = dict(W=16, margin=0.01, vmax=1.5, amax=4.0, dt=0.01, max_path_speed=1e5)


@functools.lru_cache(maxsize=None)
def payoff():
    """float64, the detour round the post (row 0 of plan_cases "post", the fingers at 0.02): the planner's polyline resampled to W
    waypoints, the same blended (blend_ref, the defaults), the same optimised (opt_ref, spec.OPT_DEFAULTS), all at one margin ->
    per path dict(S, clearance: the lowest sampled clearance, duration: retime_ref, ratio: the second-difference ratio)"""
    c = pc.case("post")
    q = c["q"][0].copy()
    q[c["qadr"][7:]] = oc.FINGERS
    goal = c["goal"][0].astype(np.float64)
    goal[7:] = oc.FINGERS
    pb = pc.problem("post")
    W, m = PAYOFF["W"], PAYOFF["margin"]
    plan = plan_ref.plan(pb, q, goal, 0, W=W, max_nodes=128, max_iterations=512, smooth_passes=64, seed=0, resolution=oc.RESOLUTION, step=pc.STEP, margin=m)
    assert plan["status"] == plan_ref.OK and len(plan["poly"]) >= 3
    blended = blend_ref.blend(pb, q, plan["poly"].astype(f32), num_waypoints=W, resolution=oc.RESOLUTION, margin=m)
    assert blended["status"] == blend_ref.OK and blended["blended"] >= 1
    opt = opt_ref.optimize(pb, q, plan["path"].astype(f32), margin=m, resolution=oc.RESOLUTION, **S.OPT_DEFAULTS)
    out = {}
    for name, path in (("polyline", plan["path"]), ("blended", blended["path"]), ("optimised", opt["path"])):
        path = np.asarray(path, np.float64)
        D = path.shape[1]
        timed = retime_ref.retime_row(path, [PAYOFF["vmax"]] * D, [PAYOFF["amax"]] * D, PAYOFF["dt"], 0, PAYOFF["max_path_speed"], want_samples=False)
        out[name] = dict(S=opt_ref.S_of(path), clearance=float(plan_ref.polyline_clearance(pb, q, path, oc.RESOLUTION)[0].min()),
                         duration=float(timed["duration"]), ratio=opt_ref.second_difference_ratio(path), length=plan_ref.polyline_length(path))
    out["opt"] = opt
    return out


def test_the_optimised_path_is_smoother_and_no_nearer_than_the_blended_one():
    p = payoff()
    o = p["opt"]
    for name in ("polyline", "blended", "optimised"):
        v = p[name]
        print(f"[opt, payoff] {name:9s}: S {v['S']:.4f}, length {v['length']:.4f} rad, lowest sampled clearance {v['clearance'] * 1e3:.1f} mm, retimed duration "
              f"{v['duration']:.3f} s, second-difference ratio {v['ratio']:.3f}")
    first = next(i for i, d in enumerate(o["log"]["decisions"]) if d[0] == "accept")
    print(f"[opt, payoff] status {o['status']} stop {o['stop']} stats {list(o['stats'])}; candidates before the first accepted one: {first}")
    assert o["status"] == opt_ref.OK and o["stats"][1] >= 3 and first <= 3, "the defaults do not stall in the first iterations"
    assert p["optimised"]["S"] < p["polyline"]["S"], p
    assert p["optimised"]["clearance"] >= p["blended"]["clearance"], p
