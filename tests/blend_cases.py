"""The cases of the corner-blending tests, shared by tests/test_blend_cpu.py (which holds the conditions the GPU tests lean on) and
tests/test_gpu_blend.py.  A helper, no test.  B = 5 rows on the scenes of plan_cases ("post": the Franka of the pick scene, the ground,
the cube and one fixed post) and carry_cases ("under": a lower post and the cube in the fingers), the same coarse sphere model (SPACING
0.12); states are SET.  A polyline gives joints 1 and 2 (columns 0 and 1) as absolute values; the other seven columns never move.  In
the cases without an obstacle they are those of the row's own start (rows 1 - 4 carry the jitter of those cases) and the two columns
are the same on every row.  In the collision cases they are those of row 0's start on every row -- the jitter of the other rows moves
the post's shadow in this plane by centimetres, and the cases are decided by millimetres -- and row r shifts joint 1 of every node by
(r - 2) x 0.004 rad, so the rows still differ.  m = 8 chords per blend, W = 32 waypoints, max_deviation 0.05 and 4 halvings unless a
case says otherwise.

In the plane of joints 1 and 2 the post blocks a region about joint 1 = 0 below a ceiling in joint 2 (the arm must be raised to pass
over it).  The collision cases climb towards that ceiling from the side and turn along it: the blend cuts the corner towards the region.

    free_corner     one right-angle corner far from everything; h from max_deviation (0.1414 against L / 2 = 0.15 and 0.2)
    short_segments  a staircase of five nodes with segments of 0.1875 on dyadic values: h = L / 2 = 0.09375 at all three corners, neighbouring
                    blends meet mid-segment with equal bits, and the two duplicates are dropped
    collinear       three nodes on one line in joint 1, dyadic (segments of 0.1875 and 0.375): du = 0 exactly, h = L / 2, the blend lies on the line
    repeats         row 0: its start six times (a failed plan: NO_MOTION); rows 1 - 4: a, a, b, b, b, c
    corner_at_post  max_deviation 0.1: the full blend (h = L / 2 = 0.38) is blocked by the post, the halved one is clear
    two_halvings    a polyline planned at margin 0 handed over with margin 0.05 (RAISED_TURN): the segment behind the corner passes over
                    the post nearer than that, the corner itself keeps it: blocked at h = 0.2625 and at h / 2, clear at h / 4.  The
                    straight remainders are the caller's and stay nearer than the margin (`remainders_clear` False)
    stays_sharp     two_halvings with max_shrinks 1: blocked at h, halved, blocked again, left sharp (2 = max_shrinks + 1)
    self_on         corner_at_post with the self test on (the entity's self model)
    carry           "under", the cube in the fingers, margin 0.01: the same turn over the lower post, blocked by the cube's spheres
    too_many        free_corner with max_points 8 (it needs 11)
    not_finite      free_corner with a NaN in row 2
    ignore          corner_at_post with MIR_PLAN_IGNORE_COLLISION: the full blend
    start_blocked   free_corner with the self test on; row 1 starts inside the post (START_IN_COLLISION), row 3 folded onto itself
                    (START_IN_SELF_COLLISION)
"""
from __future__ import annotations

import functools

import numpy as np

import blend_ref
import carry_cases as cc
import plan_cases as pc
import plan_ref
import self_ref

B = pc.B
RESOLUTION, MARGIN = pc.RESOLUTION, 0.0
M_CHORDS, W = 8, 32
DEFAULTS = dict(max_deviation=0.05, blend_points=M_CHORDS, max_shrinks=4, max_points=None)
NAMES = ("free_corner", "short_segments", "collinear", "repeats", "corner_at_post", "two_halvings", "stays_sharp", "self_on", "carry", "too_many", "not_finite",
         "ignore", "start_blocked")
COLLISION_CASES = ("corner_at_post", "two_halvings", "stays_sharp", "self_on", "carry")
# (joint 1, joint 2) per node
FREE = ((-1.0, -0.9), (-1.3, -0.9), (-1.3, -0.5))
STAIRS = ((-1.0, -1.0), (-1.1875, -1.0), (-1.1875, -0.8125), (-1.375, -0.8125), (-1.375, -1.0))
LINE = ((-1.0, -0.9), (-1.1875, -0.9), (-1.5625, -0.9))
POST_TURN = ((-0.9, -0.2), (-0.22, -0.55), (0.9, -0.55))
CARRY_TURN = ((-0.9, -0.1), (-0.20, -0.49), (0.9, -0.49))
CARRY_MARGIN = 0.01
START_IN_POST = (0.0, -0.3)                                   # joints 1 and 2: the forearm 5 cm inside the post
START_FOLDED = (0.59, 1.07, 0.74, -2.98, -0.07, 0.23, 1.93)   # all seven: 12 cm clear of the scene, 10 cm inside the arm's own spheres
# a polyline that is clear at margin 0 (its second segment passes 1 cm over the post) handed over with a margin of 5 cm: the corner,
# 0.28 rad before the post's shadow, keeps 6 cm, the segment behind it does not
RAISED_TURN = ((-0.9, -0.2), (-0.50, -0.54), (0.9, -0.54))
RAISED_MARGIN = 0.05
ROW_SHIFT = 0.004
# the halvings each collision case takes at its one corner (max_shrinks + 1: left sharp)
HALVINGS = {"corner_at_post": 1, "two_halvings": 2, "stays_sharp": 2, "self_on": 1, "carry": 1}


def _poly(base, nodes, collision=False):
    """(B, K, D) float32: the nodes' two columns, the other columns from each row's start (collision: from row 0's, joint 1 shifted)"""
    start = base["q"][:, base["qadr"]]
    if collision:
        start = np.repeat(start[:1], B, axis=0)
    out = np.repeat(start[:, None, :], len(nodes), axis=1).astype(np.float32)
    out[:, :, :2] = np.asarray(nodes, np.float32)[None]
    if collision:
        out[:, :, 0] += (np.float32(ROW_SHIFT) * (np.arange(B, dtype=np.float32) - 2))[:, None]
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(scene, sb, spec, probes, links, n_extra, mask (or None), carry (body, link) or None, skip, qadr, q (B, nq) float32,
    poly (B, K, D) float32, n_poly (B,) int32 or None, ignore, margin, remainders_clear (False: the polyline's own segments are
    nearer than the margin by design, only the blend's chords are judged for clearance), par: the keywords of the call beyond the defaults)"""
    scene = "under" if name == "carry" else "post"
    base = cc.case("under") if scene == "under" else pc.case("post")
    out = dict(scene=scene, sb=base["sb"], spec=base["spec"], probes=base["probes"], links=base["links"], n_extra=0, mask=None, carry=None,
               skip=base["skip"], qadr=base["qadr"], q=base["q"], n_poly=None, ignore=False, margin=MARGIN, remainders_clear=True,
               par=dict(DEFAULTS))
    nodes = FREE
    if name == "short_segments":
        nodes = STAIRS
    elif name == "collinear":
        nodes = LINE
    elif name in ("corner_at_post", "self_on", "ignore"):
        nodes = POST_TURN
        out["par"].update(max_deviation=0.1)
        out["ignore"] = name == "ignore"
    elif name in ("two_halvings", "stays_sharp"):
        nodes = RAISED_TURN
        out["par"].update(max_deviation=0.2, max_shrinks=4 if name == "two_halvings" else 1)
        out.update(margin=RAISED_MARGIN, remainders_clear=False)
    elif name == "carry":
        nodes = CARRY_TURN
        out["par"].update(max_deviation=0.1)
        out.update(n_extra=base["n_extra"], mask=base["mask"], carry=(base["body"], base["link"]), margin=CARRY_MARGIN)
    elif name == "too_many":
        out["par"].update(max_points=8)
    poly = _poly(base, nodes, name in COLLISION_CASES or name == "ignore")
    if name == "repeats":
        a, b, c = (poly[:, k] for k in range(3))
        poly = np.stack([a, a, b, b, b, c], axis=1)
        poly[0] = base["q"][0, base["qadr"]]
    elif name == "not_finite":
        poly[2, 1, 1] = np.nan
    elif name == "start_blocked":
        poly[1, 0, :2] = START_IN_POST
        poly[3, 0, :7] = START_FOLDED
    if name in ("self_on", "start_blocked"):
        probes, links, n_extra, mask = pc.arm(base["sb"]).self_collision_model(spacing=pc.SPACING)
        out.update(probes=probes, links=links, n_extra=n_extra, mask=mask)
    out["poly"] = np.ascontiguousarray(poly, np.float32)
    return out


def problem(name, dtype=np.float64):
    c = case(name)
    if name == "carry":
        return cc.problem("under", dtype)
    if c["mask"] is not None:
        return self_ref.SelfProblem(c["spec"], c["probes"], c["links"], c["qadr"], c["n_extra"], c["mask"], c["skip"], 1.0, 0.0, 1.0, dtype)
    return plan_ref.Problem(c["spec"], c["probes"], c["links"], c["qadr"], c["skip"], 1.0, dtype)


@functools.lru_cache(maxsize=None)
def reference(name, row, dtname="float64", num_waypoints=W):
    """blend_ref.blend of one row of a case (computed once, shared; nobody writes into it)"""
    c = case(name)
    return blend_ref.blend(problem(name, np.dtype(dtname).type), c["q"][row], c["poly"][row], None if c["n_poly"] is None else c["n_poly"][row],
                           resolution=RESOLUTION, margin=c["margin"], num_waypoints=num_waypoints, ignore_collision=c["ignore"], **c["par"])
