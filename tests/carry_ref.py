"""Reference for the carried object (include/mirigid.h "carried object": mir_plan_path_carry, mir_path_clearance_carry), in NumPy,
parametrised by dtype.  A helper, no test.  It shares no code with the HIP kernel.

CarryProblem is a self_ref.SelfProblem (which is a plan_ref.Problem) with one more body rule: the carried free body C follows the
attach link Lk by the row's grasp transform G = (p_G, q_G),

    G from the start row:  p_G = qrot(conj(q_L), p_C - p_L),  q_G = qmul(conj(q_L), q_C)      (after the full forward kinematics)
    G given (7,):          p_G = xyz,  q_G = wxyz / sqrt(w^2 + x^2 + y^2 + z^2)
    clear(q):              after the forward kinematics of the moving bodies  p_C = p_L + qrot(q_L, p_G),  q_C = qmul(q_L, q_G)

so the probes whose link is C ride on the hand.  A G that is not finite, or a given quaternion whose squared norm is below 1e-30,
blocks the row: both values of every configuration are -infinity.  plan_ref.plan, self_ref.plan and the polyline checks take the
problem unchanged; `grasp` (None: from the start row) is an attribute because they call set_row(qrow) themselves.  Without a self
query the mask is all zero and n_extra = 0: the self value is then self_max everywhere and clear(q) is the scene test alone.
"""
from __future__ import annotations

import numpy as np

import self_ref
from plan_ref import _qmul, _qrot


def _conj(q):
    return (q * np.array([1, -1, -1, -1], q.dtype)).astype(q.dtype)


class CarryProblem(self_ref.SelfProblem):
    def __init__(self, spec, probes, links, dof_qadr, n_extra, link_mask, body, link, skip_geoms=0, max_distance=1.0, self_margin=0.0,
                 self_max=1.0, dtype=np.float64):
        super().__init__(spec, probes, links, dof_qadr, n_extra, [0] * 32 if link_mask is None else link_mask, skip_geoms, max_distance,
                         self_margin, self_max, dtype)
        assert self.model.jtype[body] == self_ref.plan_ref.kin_ref.FREE and body != link and body not in list(self.model.parent[1:])
        assert not any(self.scene.geoms[g]["body"] == body for g in self.tested), "a geom of the carried body is tested"
        self.body, self.link, self.grasp = int(body), int(link), None

    def set_row(self, qrow):
        dt = self.dtype
        start = super().set_row(qrow)   # (the full forward kinematics: the carried body where its qpos puts it)
        zero = False
        if self.grasp is None:
            lc = _conj(self.xq[self.link])
            pG, qG = _qrot(lc, (self.xp[self.body] - self.xp[self.link]).astype(dt)), _qmul(lc, self.xq[self.body])
        else:
            g = np.asarray(self.grasp).astype(dt)
            with np.errstate(all="ignore"):
                n2 = (g[3:] * g[3:]).sum(dtype=dt)
                zero = bool(n2 < 1e-30)
                pG, qG = g[:3].copy(), np.array([1, 0, 0, 0], dt) if zero else (g[3:] / np.sqrt(n2)).astype(dt)
        self.G = (pG, qG)
        self.blocked = zero or not (np.isfinite(pG).all() and np.isfinite(qG).all())
        return start

    def grasp_used(self):
        return np.concatenate(self.G)

    def _fk(self, q, only_moving):
        super()._fk(q, only_moving)
        if only_moving:
            pL, qL = self.xp[self.link], self.xq[self.link]
            self.xp[self.body] = (pL + _qrot(qL, self.G[0])).astype(self.dtype)
            self.xq[self.body] = _qmul(qL, self.G[1])

    def both(self, qp):
        if self.blocked:
            return self.dtype(-np.inf), self.dtype(-np.inf)
        with np.errstate(invalid="ignore"):
            return super().both(qp)
