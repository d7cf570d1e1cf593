"""Reference for the self-collision test of the sphere model (include/mirigid.h "self-collision": mir_self_distance,
mir_plan_path_self, mir_path_clearance_self), in NumPy, parametrised by dtype.  A helper, no test.  It shares no code with the HIP kernels.

SelfProblem is a plan_ref.Problem whose clearance is two numbers: the scene value over the first N probes (the arithmetic of
plan_ref.Problem.clearance) and the self value over all N + E of them,

    s(i, j) = |c_i - c_j| - (r_i + r_j),   self_i = min over the j with bit link[j] of link_mask[link[i]] set (the lower j on a tie),
    self(q) = min(min_i self_i, self_max),

both -infinity for a configuration or a probe centre that is not finite.  plan_ref.plan / polyline_clearance / path_clearance take it
unchanged: they call clearance(q) and compare with a margin, so `mode` says what that one number is:

    "both"   the planner's question.  The scene value when the self test holds (self(q) >= self_margin), else -infinity: compared with
             `margin` it is exactly clear(q) of the header, in any dtype (no sum of the two values is formed).
    "scene"  the scene value alone;   "self"  the self value alone (compare it with self_margin).
"""
from __future__ import annotations

import numpy as np

import dist_ref
import plan_ref

START_IN_SELF_COLLISION, GOAL_IN_SELF_COLLISION = 7, 8


class SelfProblem(plan_ref.Problem):
    def __init__(self, spec, probes, links, dof_qadr, n_extra, link_mask, skip_geoms=0, max_distance=1.0, self_margin=0.0, self_max=1.0,
                 dtype=np.float64):
        super().__init__(spec, probes, links, dof_qadr, skip_geoms, max_distance, dtype)
        dt = self.dtype
        self.N = len(self.probes) - int(n_extra)
        self.mask = [int(w) for w in link_mask]
        lk = self.links
        self.enabled = np.array([[(self.mask[int(a)] >> int(b)) & 1 for b in lk] for a in lk], bool)
        self.self_margin, self.self_max = dt(self_margin), dt(self_max)
        self.mode = "both"

    def set_row(self, qrow):
        self.pairs = {}
        return super().set_row(qrow)

    def self_distances(self, pw):
        """per probe: (self_i (inf: no partner), its j (-1)) at the world centres pw"""
        dt = self.dtype
        d = (pw[:, None, :] - pw[None, :, :]).astype(dt)
        n2 = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype(dt) + d[..., 2] * d[..., 2]).astype(dt)
        r = self.probes[:, 3]
        s = (np.sqrt(n2).astype(dt) - (r[:, None] + r[None, :]).astype(dt)).astype(dt)
        s = np.where(self.enabled, s, dt(np.inf))
        j = s.argmin(1)   # (the first of equal minima: the lower j)
        best = s[np.arange(len(s)), j]
        return best, np.where(np.isfinite(best), j, -1)

    def both(self, qp):
        """(scene value, self value) of the configuration qp"""
        dt = self.dtype
        key = np.asarray(qp).astype(dt).tobytes()
        if key in self.pairs:
            return self.pairs[key]
        pw = self.centres(qp)
        if not (np.isfinite(pw).all() and np.isfinite(np.asarray(qp, np.float64)).all()):   # (not a configuration: blocked)
            out = (dt(-np.inf), dt(-np.inf))
        else:
            scene = self.max_distance
            for geom, c, Rg in self.frames:
                d = dist_ref.geom_distance(geom, ((pw[:self.N] - c) @ Rg).astype(dt), dt)[0]
                scene = min(scene, dt((d - self.probes[:self.N, 3]).min()))
            out = (dt(scene), dt(min(self.self_distances(pw)[0].min(), self.self_max)))
        self.pairs[key] = out
        return out

    def clearance(self, qp):
        self.checked += 1
        scene, own = self.both(qp)
        if self.mode == "scene":
            return scene
        if self.mode == "self":
            return own
        return scene if own >= self.self_margin else self.dtype(-np.inf)


def plan(pb: SelfProblem, qrow, goal, env, margin=0.0, **kw):
    """mir_plan_path_self of one row: plan_ref.plan with the clear(q) of both tests; a start (goal) that fails for the self test alone
    is status 7 (8) -- for one configuration the scene test decides first"""
    pb.mode = "both"
    out = plan_ref.plan(pb, qrow, goal, env, margin=margin, **kw)
    if out["status"] in (plan_ref.START_IN_COLLISION, plan_ref.GOAL_IN_COLLISION):
        start = pb.set_row(qrow)
        q = start if out["status"] == plan_ref.START_IN_COLLISION else np.asarray(goal).astype(pb.dtype)
        if pb.both(q)[0] >= pb.dtype(margin):
            out["status"] = START_IN_SELF_COLLISION if out["status"] == plan_ref.START_IN_COLLISION else GOAL_IN_SELF_COLLISION
    return out


def polyline_clearances(pb: SelfProblem, qrow, poly, resolution):
    """the swept check of both tests on the same samples -> seg_min (K-1,), seg_self_min (K-1,), the samples"""
    pb.mode = "scene"
    seg, samples = plan_ref.polyline_clearance(pb, qrow, poly, resolution)
    pb.mode = "self"
    seg_self, _ = plan_ref.polyline_clearance(pb, qrow, poly, resolution)
    pb.mode = "both"
    return seg, seg_self, samples


def path_clearance(pb: SelfProblem, qrow, path, resolution, margin):
    """mir_path_clearance_self of one row -> seg_min, seg_self_min, row_min, row_self_min, row_first_blocked"""
    seg, seg_self, _ = polyline_clearances(pb, qrow, path, resolution)
    blocked = np.flatnonzero((seg < pb.dtype(margin)) | (seg_self < pb.self_margin))
    return seg, seg_self, seg.min(), seg_self.min(), int(blocked[0]) if len(blocked) else -1


def self_distance(pb: SelfProblem, qrow, qp=None, max_distance=1.0):
    """mir_self_distance of one row at the planned dofs qp (None: those of the row) -> distance (N + E,), other (N + E,), row_min,
    row_pair, per probe the gap to the runner-up partner (inf: none), and the uncapped self_i"""
    dt = pb.dtype
    start = pb.set_row(qrow)
    pw = pb.centres(start if qp is None else qp)
    best, j = pb.self_distances(pw)
    hit = best <= dt(max_distance)
    distance, other = np.where(hit, best, dt(max_distance)).astype(dt), np.where(hit, j, -1)
    d = (pw[:, None, :] - pw[None, :, :]).astype(dt)
    s = np.sqrt((d * d).sum(2)) - (pb.probes[:, 3][:, None] + pb.probes[:, 3][None, :])
    s = np.where(pb.enabled, s, np.inf)
    s[np.arange(len(s)), np.maximum(j, 0)] = np.inf
    runner = s.min(1) - best
    if hit.any():
        i = int(np.flatnonzero(hit & (distance == distance[hit].min()))[0])
        return distance, other, distance[i], (i, int(other[i])), runner, best
    return distance, other, dt(max_distance), (-1, -1), runner, best
