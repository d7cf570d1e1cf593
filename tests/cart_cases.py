"""The cases of the Cartesian-path tests, shared by tests/test_cart_cpu.py (which holds the conditions the GPU tests lean on) and
tests/test_gpu_cartesian.py.  A helper, no test.  B = 5 rows on the scenes of plan_cases ("post": the Franka of the pick scene, the
ground, the cube and one fixed post) and carry_cases ("under": a lower post and the cube in the fingers), the same coarse sphere model
(SPACING 0.12); states are SET; the link is the hand.  Row 0 starts at plan_cases.START, rows 1 - 4 carry the jitter of those cases.
Targets are built in float64 from the hand's pose at each start row and rounded to float32: what every solver is given.

    down_side      0.153 m down, then 0.097 m along +y (K = 2), orientation held; max_step 0.01: S = 16 + 10.  (0.15 and 0.10 put the
                   quotients under the ceil on integers: condition 1 of tests/test_cart_cpu.py moved the lengths, not the bound.)
    turn           one segment: 0.083 m along +x and 0.52 rad about the world z axis; max_rot_step sets the count (10.4 against 8.3).
    position_only  down_side without target_quat.
    through_post   one segment to (0.45, 0.12, 0.40), orientation held: the fingers run into the post.
    out_of_reach   one segment to (0, -1.2, 0.5), position only, max_step 0.03: the arm runs out of reach.
    jump           down_side with jump_threshold 1e-3.
    too_long       down_side with max_points 8.
    not_finite     down_side with a NaN in row 2's second target.
    self_on        down_side with the self test on (the entity's self model: the base's spheres behind the arm's).
    self_fold      one segment to (0, 0, 0.45), position only, self test on: the hand folds onto the arm's base.
    carry_lift     "under": the cube in the fingers, one segment to (0.48, 0.12, 0.57), orientation held: the arm's own spheres
                   pass over the post, the cube's do not.
    carry_empty    the arm's spheres alone with a MirCarryQuery that names the cube: nothing rides on it.
"""
from __future__ import annotations

import functools

import numpy as np

import carry_cases as cc
import cart_ref
import plan_cases as pc
import plan_ref
import self_ref

B = pc.B
RESOLUTION, MARGIN = pc.RESOLUTION, 0.0
DOWN, SIDE, TURN_X, TURN_ANGLE = 0.153, 0.097, 0.083, 0.52
POST_TARGET, REACH_TARGET, FOLD_TARGET = (0.45, 0.12, 0.40), (0.0, -1.2, 0.5), (0.0, 0.0, 0.45)
CARRY_TARGET = (0.48, 0.12, 0.57)
DEFAULTS = dict(max_pos_step=0.01, max_rot_step=0.05, jump_threshold=0.5, max_points=64)
NAMES = ("down_side", "turn", "position_only", "through_post", "out_of_reach", "jump", "too_long", "not_finite", "self_on", "self_fold",
         "carry_lift", "carry_empty")
OK_CASES = ("down_side", "turn", "position_only", "self_on")
EXPECT = {"down_side": cart_ref.OK, "turn": cart_ref.OK, "position_only": cart_ref.OK, "self_on": cart_ref.OK, "through_post": cart_ref.BLOCKED,
          "out_of_reach": cart_ref.IK_FAILED, "jump": cart_ref.JOINT_JUMP, "too_long": cart_ref.TOO_MANY_POINTS, "self_fold": cart_ref.BLOCKED_SELF,
          "carry_lift": cart_ref.BLOCKED, "carry_empty": cart_ref.OK}


def _hand_poses(base):
    """the hand's float64 pose at each start row of a scene case"""
    hand = base["sb"].body_index("hand")
    pb = plan_ref.Problem(base["spec"], base["probes"][:1], base["links"][:1], base["qadr"], base["skip"], 1.0, np.float64)
    ch = cart_ref.Chain(pb, hand, base["spec"])
    out = []
    for r in range(B):
        out.append(ch.pose(pb.set_row(base["q"][r])))
    return hand, np.stack([p for p, _ in out]), np.stack([q for _, q in out])


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(scene, sb, spec, probes, links, n_extra, mask (or None), carry (body, link) or None, skip, qadr, q (B, nq) float32, link,
    tpos (B, K, 3) float32, tquat (B, K, 4) float32 or None, par: the keywords of the call beyond the defaults)"""
    scene = "under" if name.startswith("carry") else "post"
    base = cc.case("under") if scene == "under" else pc.case("post")
    hand, hp, hq = _hand_poses(base)
    out = dict(scene=scene, sb=base["sb"], spec=base["spec"], probes=base["probes"], links=base["links"], n_extra=0, mask=None, carry=None,
               skip=base["skip"], qadr=base["qadr"], q=base["q"], link=hand, par=dict(DEFAULTS))
    hold = np.repeat(hq[:, None, :], 2, axis=1)
    down_side = np.stack([hp + [0, 0, -DOWN], hp + [0, SIDE, -DOWN]], axis=1)
    tpos, tquat = down_side, hold
    if name == "turn":
        h = 0.5 * TURN_ANGLE
        qz = np.array([np.cos(h), 0.0, 0.0, np.sin(h)])
        tpos, tquat = (hp + [TURN_X, 0, 0])[:, None, :], np.stack([plan_ref._qmul(qz, q) for q in hq])[:, None, :]
    elif name == "position_only":
        tquat = None
    elif name == "through_post":
        tpos, tquat = np.tile(np.array(POST_TARGET), (B, 1, 1)), hq[:, None, :]
    elif name == "out_of_reach":
        tpos, tquat = np.tile(np.array(REACH_TARGET), (B, 1, 1)), None
        out["par"].update(max_pos_step=0.03)
    elif name == "jump":
        out["par"].update(jump_threshold=1e-3)
    elif name == "too_long":
        out["par"].update(max_points=8)
    elif name == "not_finite":
        tpos = tpos.copy()
        tpos[2, 1, 1] = np.nan
    elif name == "self_fold":
        tpos, tquat = np.tile(np.array(FOLD_TARGET), (B, 1, 1)), None
    elif name == "carry_lift":
        tpos, tquat = np.tile(np.array(CARRY_TARGET), (B, 1, 1)), hq[:, None, :]
        out.update(n_extra=base["n_extra"], mask=base["mask"], carry=(base["body"], base["link"]))
    elif name == "carry_empty":
        out.update(probes=base["probes"][:base["n_arm"]], links=base["links"][:base["n_arm"]], carry=(base["body"], base["link"]))
    if name in ("self_on", "self_fold"):
        probes, links, n_extra, mask = pc.arm(base["sb"]).self_collision_model(spacing=pc.SPACING)
        out.update(probes=probes, links=links, n_extra=n_extra, mask=mask)
    out["tpos"] = tpos.astype(np.float32)
    out["tquat"] = None if tquat is None else tquat.astype(np.float32)
    return out


def problem(name, dtype=np.float64):
    c = case(name)
    if name == "carry_lift":
        return cc.problem("under", dtype)
    if c["mask"] is not None:
        return self_ref.SelfProblem(c["spec"], c["probes"], c["links"], c["qadr"], c["n_extra"], c["mask"], c["skip"], 1.0, 0.0, 1.0, dtype)
    return plan_ref.Problem(c["spec"], c["probes"], c["links"], c["qadr"], c["skip"], 1.0, dtype)


@functools.lru_cache(maxsize=None)
def reference(name, row, dtname="float64", num_waypoints=0):
    """cart_ref.solve of one row of a case (computed once, shared; nobody writes into it)"""
    c = case(name)
    return cart_ref.solve(problem(name, np.dtype(dtname).type), c["spec"], c["link"], c["q"][row], c["tpos"][row],
                          None if c["tquat"] is None else c["tquat"][row], resolution=RESOLUTION, margin=MARGIN, num_waypoints=num_waypoints, **c["par"])


def link_pose(name, row, cfg):
    """the float64 pose of the case's link at the planned dofs cfg of a row"""
    c = case(name)
    pb = plan_ref.Problem(c["spec"], c["probes"][:1], c["links"][:1], c["qadr"], c["skip"], 1.0, np.float64)
    pb.set_row(c["q"][row])
    return cart_ref.Chain(pb, c["link"], c["spec"]).pose(np.asarray(cfg, np.float64))
