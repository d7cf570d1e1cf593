"""The goal sets of the goal-set planning tests, shared by tests/test_goal_cpu.py (which holds the conditions the GPU tests lean on) and
tests/test_gpu_goal.py.  A helper, no test.  B = 5 rows; the scene ("post" and "clear" of tests/plan_cases.py are ONE scene with ONE set
of start rows and two goals), the sphere model, the budgets and the jitter are those of plan_cases.

    "near_far"     [GOAL (needs the detour round the post), CLEAR_GOAL (a clear straight edge)]; "far_near" is the other order.
    "two_detours"  [GOAL, GOAL jittered once more by the case rng]: neither has a clear edge.
    "bad_first"    [the midpoint of START - GOAL (inside the post), GOAL with planned dof 0 (joint 1) 0.1 rad above its limit, GOAL].
    "all_bad"      the first two of those.
    "twice"        [CLEAR_GOAL, CLEAR_GOAL]: equal distances, the lower g wins.
    "blocked_near" [GOAL (valid, nearer, its edge blocked by the post), a clear goal beyond CLEAR_GOAL on the same line, farther than GOAL]:
                   the second pick of the direct-edge order.

Pose targets (link "hand"): "pose_far" / "pose_near" = the float64 pose of the hand at GOAL / CLEAR_GOAL per row, so a solution exists
by construction; "pose_away" = a point 2 m from the base: unreachable; "pose_post" = the post's centre, position only: every solution
collides.
"""
from __future__ import annotations

import functools

import numpy as np

import goal_ref
import plan_cases as pc

B = pc.B
NAMES = ("near_far", "far_near", "two_detours", "bad_first", "all_bad", "twice", "blocked_near")
POSES = ("pose_far", "pose_near", "pose_away", "pose_post")
BEYOND = 3.0   # "blocked_near": start + BEYOND (CLEAR_GOAL - start) in the arm joints


@functools.lru_cache(maxsize=None)
def goals(name):
    """-> (B, G, D) float32"""
    post, clear = pc.case("post"), pc.case("clear")
    assert np.array_equal(post["q"], clear["q"]), "one scene, one set of start rows"
    far, near = post["goal"], clear["goal"]
    if name == "near_far":
        return np.stack([far, near], 1)
    if name == "far_near":
        return np.stack([near, far], 1)
    if name == "two_detours":
        jit = np.zeros((B, 9))
        jit[:, :7] = np.random.default_rng(171).uniform(-0.04, 0.04, (B, 7))
        return np.stack([far, (far.astype(np.float64) + jit).astype(np.float32)], 1)
    if name == "twice":
        return np.stack([near, near], 1)
    if name == "blocked_near":
        beyond = near.copy()
        st = post["start"].astype(np.float64)
        beyond[:, :7] = (st[:, :7] + BEYOND * (near.astype(np.float64)[:, :7] - st[:, :7])).astype(np.float32)
        return np.stack([far, beyond], 1)
    mid = (0.5 * (post["start"].astype(np.float64) + far.astype(np.float64))).astype(np.float32)
    out = far.copy()
    out[:, 0] = np.float32(pc.problem("post", np.float32).hi[0]) + np.float32(0.1)
    if name == "bad_first":
        return np.stack([mid, out, far], 1)
    if name == "all_bad":
        return np.stack([mid, out], 1)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name, row, seed=0, dtname="float64", n_goals=None):
    """goal_ref.plan_goals of one row of a goal set at the test budgets (computed once, shared)"""
    c = pc.case("post")
    return goal_ref.plan_goals(pc.problem("post", np.dtype(dtname).type), c["q"][row], goals(name)[row], row, n_goals=n_goals, W=pc.BUDGET["W"],
                               max_nodes=pc.BUDGET["max_nodes"], max_iterations=pc.BUDGET["max_iterations"], seed=seed, resolution=pc.RESOLUTION,
                               step=pc.STEP, margin=pc.MARGIN)


def valid_polyline(row, poly, goal, margin=pc.MARGIN, tol=0.0):
    """the float64 validator of plan_cases with the row's goal given: every edge keeps margin - tol, the ends are the start's and the
    goal's bits -> (ok, lowest clearance, the samples)"""
    c = pc.case("post")
    poly = np.asarray(poly, np.float64)
    seg, samples = pc.plan_ref.polyline_clearance(pc.problem("post"), c["q"][row], poly, pc.RESOLUTION)
    ends = np.array_equal(poly[0].astype(np.float32), c["start"][row]) and np.array_equal(poly[-1].astype(np.float32), np.asarray(goal, np.float32))
    return bool(ends and seg.min() >= margin - tol), float(seg.min()), samples


def hand():
    return pc.case("post")["sb"].body_index("hand")


@functools.lru_cache(maxsize=None)
def pose(name):
    """-> (pos (B, 3) float32, quat (B, 4) float32 or None)"""
    c = pc.case("post")
    if name == "pose_away":
        return np.tile(np.array([2.0, 0.0, 0.5], np.float32), (B, 1)), np.tile(np.array([0.0, 1.0, 0.0, 0.0], np.float32), (B, 1))
    if name == "pose_post":
        return np.tile(np.array(pc.POST["pos"], np.float32), (B, 1)), None
    cfgs = {"pose_far": c["goal"], "pose_near": pc.case("clear")["goal"]}[name]
    pb = pc.problem("post")
    ch = goal_ref.cart_ref.Chain(pb, hand(), c["spec"])
    P, Q = [], []
    for r in range(B):
        pb.set_row(c["q"][r])
        p, q = ch.pose(cfgs[r].astype(np.float64))
        P.append(p)
        Q.append(q)
    return np.stack(P).astype(np.float32), np.stack(Q).astype(np.float32)


@functools.lru_cache(maxsize=None)
def pose_reference(name, row, seed=0, dtname="float64", position_only=False):
    """goal_ref.plan_pose of one row of a pose case at the test budgets, max_goals 4, max_samples 16 (computed once, shared)"""
    c = pc.case("post")
    tp, tq = pose(name)
    return goal_ref.plan_pose(pc.problem("post", np.dtype(dtname).type), c["spec"], hand(), c["q"][row], tp[row], None if tq is None or position_only else tq[row],
                              row, max_goals=4, max_samples=16, W=pc.BUDGET["W"], max_nodes=pc.BUDGET["max_nodes"],
                              max_iterations=pc.BUDGET["max_iterations"], seed=seed, resolution=pc.RESOLUTION, step=pc.STEP, margin=pc.MARGIN)
