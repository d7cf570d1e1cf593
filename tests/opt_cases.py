"""The cases of the trajectory-optimisation tests, shared by tests/test_opt_cpu.py (which holds the conditions the GPU tests lean on) and
tests/test_gpu_opt.py.  A helper, no test.  B = 5 rows on the scenes of plan_cases ("post": the Franka of the pick scene, the ground,
the cube and one fixed post) and carry_cases ("under": a lower post and the cube in the fingers), the same coarse sphere model (SPACING
0.12); states are SET.  A seed gives joints 1 and 2 (columns 0 and 1) as absolute values on a polyline that is resampled to K waypoints
at equal arc length; the other seven columns never move in the seed (the descent may move them).  The two finger columns of every
seed are 0.02, mid-range: a dof that sits ON its limit with the obstacle gradient pointing outward is rejected at every step length
(the rule has no projection), which is a property of the rule and not what these cases are about.  In the cases without an obstacle
the other columns are those of the row's own start (rows 1 - 4 carry the jitter of plan_cases).  In the collision cases they are those of
row 0's start on every row, the state included -- the jitter of the other rows moves the post's shadow by centimetres, and the cases
are decided by millimetres -- and row r shifts joint 1 of every waypoint by (r - 2) x 0.004 rad, so the rows still differ.

In the plane of joints 1 and 2 the post blocks a region about joint 1 = 0 below a ceiling in joint 2 (the arm must be raised to pass).

    free           one right-angle corner far from everything: O = 0, the gradient is the smoothness term alone; ftol 0.05: CONVERGED
    line           the same corner with w_o = 0, alpha w_s = 1, one iteration: the straight line at equal spacing
    over_post      the float64 planner's own path for row 0 of "post" (fingers at 0.02), which grazes the post at margin 0
    pushed_out     a straight pass over the post at the height at which the lowest waypoint is 3 mm inside a margin of 2 cm
    self_on        over_post with the self test on (the entity's self model)
    carry          "under", the cube in the fingers, margin 0.01: the turn of blend_cases over the lower post
    thin           a long sweep about the base at K = 8 with a 1 cm sphere (cert_cases "thin") 6 mm inside a sphere of the arm at a sample
                   BETWEEN two waypoints of the result, from the direction that leaves the waypoints the most room (5 mm: the descent
                   sees it in its band and leans away, but the cost looks at the waypoints only): the sweep blocks by more than 1 mm,
                   the input comes back; with the sphere skipped the rows are OK (rows shifted by 1 mrad)
    limits         a seed whose ends lie 1 cm from joint 2's lower limit, alpha w_s = 1.9: the first candidate overshoots the straight
                   line through the limit, the halved one is accepted
    not_finite     free with a NaN in row 2;  no_motion: row 0 holds its first waypoint K times;  out_of_limits: row 3 has an interior
                   waypoint beyond joint 1's upper limit;  ignore: over_post with MIR_PLAN_IGNORE_COLLISION
"""
from __future__ import annotations

import functools

import numpy as np

import blend_cases as bcs
import carry_cases as cc
import opt_ref
import plan_cases as pc
import plan_ref
import self_ref
from gym_genesis.backend import spec as S

B = pc.B
RESOLUTION = pc.RESOLUTION
FINGERS = 0.02
ROW_SHIFT = 0.004
NAMES = ("free", "line", "over_post", "pushed_out", "self_on", "carry", "thin", "limits", "not_finite", "no_motion", "out_of_limits", "ignore")
COLLISION_CASES = ("over_post", "pushed_out", "self_on", "carry", "thin", "ignore")
# the parameters of the cases: at most 12 iterations
PAR = dict(smooth_weight=1.0, obstacle_weight=1.0, activation=0.05, step=0.25, max_iterations=4, max_halvings=5, ftol=0.0)
FREE = ((-1.0, -0.9), (-1.31, -0.9), (-1.31, -0.52))   # far from everything (blend_cases' corner, off the dyadic values)
PUSHED_MARGIN, PUSHED_DEPTH, PUSHED_ENDS = 0.02, 0.003, (-0.9, 0.87)
CARRY_MARGIN = bcs.CARRY_MARGIN
LIMIT_NODES = ((-1.0, -1.7528), (-1.3, -1.45), (-1.6, -1.7528))   # joint 2's lower limit is -1.7628
THIN_RADIUS, THIN_DEPTH, THIN_SHIFT = 0.01, 0.006, 0.001
THIN_NODES = ((-2.4, -0.9), (-1.5, -0.9), (-1.5, -0.3))   # a long sweep about the base, far from the post: 13 cm between two waypoints
FREE_FTOL = 0.05   # free stops CONVERGED: its fifth accepted step lowers U by less than 5 %
K_OF = dict(free=8, line=10, over_post=12, pushed_out=10, self_on=12, carry=12, thin=8, limits=9, not_finite=8, no_motion=8, out_of_limits=8, ignore=12)


def _resampled(nodes_full, K):
    return plan_ref.resample(np.asarray(nodes_full, np.float64), K, np.float64).astype(np.float32)


def _seed(start, nodes, K, collision, shift=ROW_SHIFT):
    """(B, K, D) float32: the nodes' two columns on the other columns of `start` (B, D), resampled to K waypoints"""
    start = np.asarray(start, np.float64).copy()
    start[:, 7:] = FINGERS
    if collision:
        start = np.repeat(start[:1], B, axis=0)
    out = []
    for r in range(B):
        poly = np.repeat(start[r][None], len(nodes), 0)
        poly[:, :2] = np.asarray(nodes, np.float64)
        out.append(_resampled(poly, K))
    out = np.stack(out)
    if collision:
        out[:, :, 0] += (np.float32(shift) * (np.arange(B, dtype=np.float32) - 2))[:, None]
    return out


def _rows(base, collision):
    """the start rows of the state: the fingers at 0.02; in the collision cases row 0's on every row"""
    q = base["q"].copy()
    q[:, base["qadr"][7:]] = FINGERS
    return np.repeat(q[:1], B, axis=0) if collision else q


@functools.lru_cache(maxsize=None)
def planner_seed():
    """(K, D) float32: plan_ref.plan (float64) for row 0 of "post" with the fingers at 0.02, resampled to 12 waypoints"""
    c = pc.case("post")
    q = _rows(c, True)[0]
    goal = c["goal"][0].astype(np.float64)
    goal[7:] = FINGERS
    r = plan_ref.plan(pc.problem("post"), q, goal, 0, W=K_OF["over_post"], max_nodes=pc.BUDGET["max_nodes"], max_iterations=pc.BUDGET["max_iterations"],
                      smooth_passes=64, seed=0, resolution=RESOLUTION, step=pc.STEP, margin=0.0)
    assert r["status"] == plan_ref.OK and len(r["poly"]) >= 3
    return r["path"].astype(np.float32), r["poly"]


@functools.lru_cache(maxsize=None)
def pushed_height():
    """joint 2 of the straight pass over the post at which the lowest waypoint of row 2's seed lies PUSHED_DEPTH inside PUSHED_MARGIN
    (float64, bisection: raising the arm, joint 2 falling, clears the post)"""
    c = pc.case("post")
    pb = pc.problem("post")
    q = _rows(c, True)
    pb.set_row(q[0])

    def lowest(h):
        seed = _seed(q[:, c["qadr"]], ((PUSHED_ENDS[0], h), (PUSHED_ENDS[1], h)), K_OF["pushed_out"], True)[2]
        return min(float(pb.clearance(w.astype(np.float64))) for w in seed[1:-1])

    lo, hi = -0.9, -0.3   # (clear, blocked)
    assert lowest(lo) > PUSHED_MARGIN and lowest(hi) < PUSHED_MARGIN - PUSHED_DEPTH
    for _ in range(30):
        mid = 0.5 * (lo + hi)
        if lowest(mid) > PUSHED_MARGIN - PUSHED_DEPTH:
            lo = mid
        else:
            hi = mid
    return float(np.float32(lo))


def _thin_paths():
    c = pc.case("post")
    return _seed(_rows(c, True)[:, c["qadr"]], THIN_NODES, K_OF["thin"], True, THIN_SHIFT)


@functools.lru_cache(maxsize=None)
def thin_sphere():
    """(the centre of the small sphere, the room it leaves the waypoints), float64: the sphere sits THIN_DEPTH inside a sphere of the arm
    at the middle sample of the longest edge of what row 2's seed becomes WITHOUT it, pushed in from the direction that leaves the
    spheres at the waypoints of that result the most room (over every probe and 400 directions, off the ground)"""
    c = pc.case("post")
    pb = pc.problem("post")
    q = _rows(c, True)[2]
    P = opt_ref.optimize(pb, q, _thin_paths()[2], margin=0.0, resolution=RESOLUTION, **PAR)["reached"]
    pb.set_row(q)
    i = int(np.abs(P[1:] - P[:-1]).max(1).argmax())
    n = plan_ref.n_sub(P[i], P[i + 1], RESOLUTION, np.float64)
    assert n >= 2
    mid = pb.centres(plan_ref.edge_samples(P[i], P[i + 1], RESOLUTION, np.float64)[n // 2 - 1]).copy()
    at = np.stack([pb.centres(w).copy() for w in P])
    rad = np.asarray(pb.probes[:, 3], np.float64)
    k = np.arange(400) + 0.5
    z, phi = 1.0 - 2.0 * k / 400, np.pi * (1.0 + 5.0 ** 0.5) * k
    dirs = np.stack([np.sqrt(1.0 - z * z) * np.cos(phi), np.sqrt(1.0 - z * z) * np.sin(phi), z], 1)
    best = None
    for p in range(len(mid)):
        o = mid[p][None] + dirs * (rad[p] + THIN_RADIUS - THIN_DEPTH)
        room = (np.linalg.norm(at[None] - o[:, None, None], axis=3) - rad[None, None]).min((1, 2)) - THIN_RADIUS
        room = np.where(o[:, 2] > 0.1, room, -1.0)
        w = int(room.argmax())
        if best is None or room[w] > best[1]:
            best = (o[w], float(room[w]))
    return best


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(scene, sb, spec, probes, links, n_extra, mask (or None), carry (body, link) or None, skip, qadr, q (B, nq) float32,
    paths (B, K, D) float32, ignore, margin, par: the keywords of the call)"""
    scene = "under" if name == "carry" else "post"
    base = cc.case("under") if scene == "under" else pc.case("post")
    collision = name in COLLISION_CASES
    out = dict(scene=scene, sb=base["sb"], spec=base["spec"], probes=base["probes"], links=base["links"], n_extra=0, mask=None, carry=None,
               skip=base["skip"], qadr=base["qadr"], q=_rows(base, collision), ignore=name == "ignore", margin=0.0, par=dict(PAR))
    K = K_OF[name]
    start = out["q"][:, base["qadr"]]
    if name in ("over_post", "self_on", "ignore"):
        seed = planner_seed()[0]
        paths = np.repeat(seed[None], B, 0)
        paths[:, :, 0] += (np.float32(ROW_SHIFT) * (np.arange(B, dtype=np.float32) - 2))[:, None]
        out["par"].update(step=0.5)   # (the first candidates of its iterations are rejected: by a finger's limit, by U)
    elif name == "pushed_out":
        h = pushed_height()
        paths = _seed(start, ((PUSHED_ENDS[0], h), (PUSHED_ENDS[1], h)), K, True)
        out["margin"] = PUSHED_MARGIN
    elif name == "carry":
        paths = _seed(start, bcs.CARRY_TURN, K, True)
        out.update(n_extra=base["n_extra"], mask=base["mask"], carry=(base["body"], base["link"]), margin=CARRY_MARGIN)
    elif name == "limits":
        paths = _seed(start, LIMIT_NODES, K, False)
        out["par"].update(step=1.9, max_iterations=2)
    elif name == "thin":
        paths = _thin_paths()
    else:
        paths = _seed(start, FREE, K, False)
    if name == "free":
        out["par"].update(ftol=FREE_FTOL, max_iterations=6)
    elif name == "line":
        out["par"].update(obstacle_weight=0.0, step=1.0, max_iterations=1)
    elif name == "thin":
        sb = pc.builder("post")
        sb.add_geom(0, S.GEOM_SPHERE, size=(THIN_RADIUS, 0.0, 0.0), pos=tuple(float(v) for v in thin_sphere()[0]), rgb=(0.9, 0.2, 0.2))
        out.update(sb=sb, spec=sb.build(), scene="thin", thin_geom=base["spec"].ngeom)
    elif name == "not_finite":
        paths[2, 3, 1] = np.nan
    elif name == "no_motion":
        paths[0] = paths[0, 0]
    elif name == "out_of_limits":
        paths[3, 4, 0] = 2.95   # joint 1's upper limit is 2.8973
    if name == "self_on":
        probes, links, n_extra, mask = pc.arm(base["sb"]).self_collision_model(spacing=pc.SPACING)
        out.update(probes=probes, links=links, n_extra=n_extra, mask=mask)
    out["paths"] = np.ascontiguousarray(paths, np.float32)
    return out


def problem(name, dtype=np.float64, skip=None):
    c = case(name)
    skip = c["skip"] if skip is None else skip
    if name == "carry":
        return cc.problem("under", dtype)
    if c["mask"] is not None:
        return self_ref.SelfProblem(c["spec"], c["probes"], c["links"], c["qadr"], c["n_extra"], c["mask"], skip, 1.0, 0.0, 1.0, dtype)
    return plan_ref.Problem(c["spec"], c["probes"], c["links"], c["qadr"], skip, 1.0, dtype)


@functools.lru_cache(maxsize=None)
def reference(name, row, dtname="float64", skip_thin=False):
    """opt_ref.optimize of one row of a case (computed once, shared; nobody writes into it)"""
    c = case(name)
    skip = c["skip"] | (1 << c["thin_geom"]) if skip_thin else None
    return opt_ref.optimize(problem(name, np.dtype(dtname).type, skip), c["q"][row], c["paths"][row], margin=c["margin"], resolution=RESOLUTION,
                            ignore_collision=c["ignore"], **c["par"])
