"""Reference for mir_cartesian_path (include/mirigid.h, "Cartesian paths"): the rule of the header restated in NumPy, parametrised by
dtype.  A helper, no test.  `dtype=np.float64` is the reference; `dtype=np.float32` is the float32 port (every intermediate rounded to
float32) that the GPU tests take their yardstick from.  It shares no code with the HIP kernel.

It is composed from a plan_ref.Problem (or self_ref.SelfProblem / carry_ref.CarryProblem: clearance and the edge rule, the forward
kinematics of the spec) and an inverse-kinematics iteration of its own on that forward kinematics: the iteration of
mir_inverse_kinematics (accept / reject / stall, the lambda^2 schedule, max_step, the limit clamp, max_iters) on the moving joints.

    counts:   n_k = max(1, ceil(max(|p_k - p_{k-1}| / max_pos_step, angle(q_{k-1}, q_k) / max_rot_step))), S = sum n_k
    target:   lerp and q_{k-1} exp(t log(q_{k-1}^-1 q_k)) along the shorter arc; the end's own values at i == n_k
    sample:   IK from the last accepted configuration -> IK_FAILED; max_j |dq_j| > jump_threshold -> JOINT_JUMP; the edge rule from the
              last accepted configuration, the scene test before the self test -> BLOCKED / BLOCKED_SELF
"""
from __future__ import annotations

import numpy as np

import kin_ref
import plan_ref
from plan_ref import _qmul, _qrot

OK, START_IN_COLLISION, START_IN_SELF_COLLISION = 0, 2, 7
TOO_MANY_POINTS, NOT_FINITE, IK_FAILED, JOINT_JUMP, BLOCKED, BLOCKED_SELF = range(16, 22)
IK_DEFAULTS = dict(max_iters=20, respect_joint_limit=1, damping=0.05, pos_tol=5e-4, rot_tol=5e-3, max_step=0.5)
MAX_COUNT = 1 << 30


def _conj(q):
    return (q * np.array([1, -1, -1, -1], q.dtype)).astype(q.dtype)


def _norm(v, dt):
    acc = dt(0)
    for x in v:
        acc = dt(acc + dt(x * x))
    return dt(np.sqrt(acc))


def delta(qa, qb, dt):
    """d = conj(qa) qb along the shorter arc (d.w == 0 is not negated), sn = |d.xyz|, ang = 2 atan2(sn, d.w)"""
    d = _qmul(_conj(qa.astype(dt)), qb.astype(dt))
    if d[0] < 0:
        d = (-d).astype(dt)
    sn = _norm(d[1:], dt)
    return d, sn, dt(dt(2) * dt(np.arctan2(sn, d[0])))


def count(dp, ang, max_pos_step, max_rot_step, dt):
    """-> (n, the quotient under the ceil)"""
    with np.errstate(all="ignore"):
        cp, cr = dt(dt(dp) / dt(max_pos_step)), dt(dt(ang) / dt(max_rot_step))
    if not (np.isfinite(cp) and np.isfinite(cr)):
        return MAX_COUNT, dt(np.inf)
    c = max(cp, cr)
    if c <= 1:
        return 1, c
    return (int(np.ceil(c)) if c < MAX_COUNT else MAX_COUNT), c


def target(pa, qa, pb, qb, d, sn, ang, i, n, userot, dt):
    """the target of sample i = 1 .. n -> (p, q or None)"""
    if i == n:
        return pb.astype(dt), (qb.astype(dt) if userot else None)
    t = dt(dt(i) / dt(n))
    p = (pa + t * (pb - pa)).astype(dt)
    if not userot:
        return p, None
    if not sn > 1e-9:
        return p, qa.astype(dt)
    h = dt(dt(0.5) * dt(t * ang))
    s = dt(dt(np.sin(h)) / sn)
    return p, _qmul(qa.astype(dt), np.array([np.cos(h), s * d[1], s * d[2], s * d[3]], dt))


def waypoint_index(w, W, n_points, dt):
    u = dt(dt(dt(w) / dt(W - 1)) * dt(n_points - 1))
    i0 = min(int(u), n_points - 2)
    return i0, dt(u - dt(i0))


def resample(points, W, dt):
    """W waypoints at equal steps of the index of the dense points (n, D); the ends are the points' own values"""
    pts = np.asarray(points).astype(dt)
    n = len(pts)
    if n == 1:
        return np.repeat(pts, W, axis=0)
    out = []
    for w in range(W):
        if w == 0:
            out.append(pts[0])
        elif w == W - 1:
            out.append(pts[-1])
        else:
            i0, t = waypoint_index(w, W, n, dt)
            out.append((pts[i0] + t * (pts[i0 + 1] - pts[i0])).astype(dt))
    return np.stack(out)


def rot_error(tq, qe, dt):
    """rotvec(tq qe^-1), world axes"""
    d = _qmul(tq.astype(dt), _conj(qe))
    if d[0] < 0:
        d = (-d).astype(dt)
    sn = _norm(d[1:], dt)
    k = dt(dt(2) * dt(np.arctan2(sn, d[0])) / sn) if sn > 1e-9 else dt(2)
    return (k * d[1:]).astype(dt)


class Chain:
    """the chain world -> link of a plan_ref.Problem: its scalar joints, which of them move (the planned dofs), their limits"""

    def __init__(self, pb: plan_ref.Problem, link: int, spec):
        m = pb.model
        self.pb, self.link = pb, int(link)
        bodies, b = [], int(link)
        while b > 0:
            assert m.jtype[b] != kin_ref.FREE, "the link hangs off a free body"
            if m.jtype[b] in (kin_ref.REVOLUTE, kin_ref.PRISMATIC) and m.qadr[b] in pb.qadr:
                bodies.append(b)
            b = m.parent[b]
        self.bodies = bodies[::-1]
        assert self.bodies, "no moving joint"
        self.dof = [pb.qadr.index(m.qadr[b]) for b in self.bodies]   # the planned dof of each moving joint
        lim = m.limits(spec)
        self.limited = np.array([lim[m.dofadr[b]] is not None for b in self.bodies])
        rng = [lim[m.dofadr[b]] or (0.0, 0.0) for b in self.bodies]
        self.lo = np.array([np.float32(r[0]) for r in rng]).astype(pb.dtype)   # (the compiled model holds float32 limits)
        self.hi = np.array([np.float32(r[1]) for r in rng]).astype(pb.dtype)

    def pose(self, cfg):
        """the link's pose at the planned dofs cfg (and the bodies' poses in the problem)"""
        pb = self.pb
        pb.q[pb.qadr] = np.asarray(cfg).astype(pb.dtype)
        pb._fk(pb.q, True)
        return pb.xp[self.link].copy(), pb.xq[self.link].copy()

    def jacobian(self, userot):
        """6 x (moving joints) at the poses of the last pose(); the rotation rows are zero without an orientation target"""
        pb, dt = self.pb, self.pb.dtype
        J = np.zeros((6, len(self.bodies)), dt)
        pe = pb.xp[self.link]
        for c, b in enumerate(self.bodies):
            ax = _qrot(pb.xq[b], pb.axis[b])
            if pb.model.jtype[b] == kin_ref.REVOLUTE:
                J[:3, c] = np.cross(ax, (pe - pb.xp[b]).astype(dt))
                if userot:
                    J[3:, c] = ax
            else:
                J[:3, c] = ax
        return J


def ik(ch: Chain, cfg, tp, tq, opts, dt):
    """the iteration of mir_inverse_kinematics on the moving joints from the configuration cfg -> (cfg', |e_pos|, |e_rot|, iterations)"""
    op = {**IK_DEFAULTS, **opts}
    pos_tol, rot_tol, max_step = dt(op["pos_tol"]), dt(op["rot_tol"]), dt(op["max_step"])
    inv_pos, inv_rot = dt(1.0 / op["pos_tol"]), dt(1.0 / op["rot_tol"])
    d2 = dt(op["damping"] * op["damping"])
    lam_min, lam_max = dt(d2 * dt(1.0 / 256.0)), dt(d2 * dt(64.0))
    userot = tq is not None
    lim = ch.limited & bool(op["respect_joint_limit"])
    q = np.asarray(cfg).astype(dt).copy()
    q_acc, lam2, stall, iters = q.copy(), d2, 0, 0
    m_acc = epn = ern = e_acc = J = None
    for it in range(op["max_iters"] + 1):
        with np.errstate(all="ignore"):
            pe, qe = ch.pose(q)
            ep = (tp - pe).astype(dt)
            er = rot_error(tq, qe, dt) if userot else np.zeros(3, dt)
            epn_c, ern_c = _norm(ep, dt), _norm(er, dt)
            metric = dt(dt(epn_c * inv_pos) + dt(ern_c * inv_rot))
        if it == 0 or metric < m_acc:
            if it > 0:
                stall = stall + 1 if metric > dt(0.99) * m_acc else 0
                lam2 = max(dt(lam2 * dt(0.25)), lam_min)
            m_acc, epn, ern, e_acc, q_acc = metric, epn_c, ern_c, np.concatenate([ep, er]).astype(dt), q.copy()
            J = ch.jacobian(userot)
        else:
            stall += 1
            lam2 = min(dt(lam2 * dt(8.0)), lam_max)
        if (epn < pos_tol and ern < rot_tol) or stall >= 3 or it == op["max_iters"]:
            break
        iters = it + 1
        A = ((J @ J.T).astype(dt) + lam2 * np.eye(6, dtype=dt)).astype(dt)
        dq = (J.T @ np.linalg.solve(A, e_acc).astype(dt)).astype(dt)
        big = np.abs(dq).max()
        sc = dt(max_step / big) if big > max_step else dt(1)
        q = q_acc.copy()
        mv = (q_acc[ch.dof] + sc * dq).astype(dt)
        mv = np.where(lim, np.minimum(np.maximum(mv, ch.lo), ch.hi), mv).astype(dt)
        q[ch.dof] = mv
    return q_acc, epn, ern, iters


def counts(ch: Chain, qrow, tpos, tquat, max_pos_step, max_rot_step):
    """the segments of one row -> list of dict(pa, qa, pb, qb, d, sn, ang, n, quotient), not_finite"""
    pb = ch.pb
    dt = pb.dtype
    a0 = pb.set_row(qrow)
    pa, qa = ch.pose(a0)
    userot = tquat is not None
    segs, bad = [], False
    for k in range(len(tpos)):
        with np.errstate(all="ignore"):
            pk = np.asarray(tpos[k]).astype(dt)
            bad = bad or not np.isfinite(pk).all()
            qk = np.array([1, 0, 0, 0], dt)
            if userot:
                raw = np.asarray(tquat[k]).astype(dt)
                n2 = (raw * raw).sum(dtype=dt)
                bad = bad or not np.isfinite(raw).all() or not (n2 >= 1e-30) or not np.isfinite(n2)
                qk = (raw / np.sqrt(n2)).astype(dt)
            d, sn, ang = delta(qa, qk, dt) if userot else (np.array([1, 0, 0, 0], dt), dt(0), dt(0))
            n, c = count(_norm((pk - pa).astype(dt), dt), ang, max_pos_step, max_rot_step, dt)
        segs.append(dict(pa=pa, qa=qa, pb=pk, qb=qk, d=d, sn=sn, ang=ang, n=n, quotient=c))
        pa, qa = pk, qk
    return a0, segs, bad


def solve(pb: plan_ref.Problem, spec, link, qrow, tpos, tquat=None, max_pos_step=0.01, max_rot_step=0.05, jump_threshold=0.5, max_points=256,
          num_waypoints=0, resolution=0.05, margin=0.0, ignore_collision=False, max_samples=None, **ik_opts):
    """mir_cartesian_path of one row -> dict(status, points (n_points, D), n_points, fraction, S, iters (per accepted or failed sample),
    checked, failed_segment, path (W, D) or None, targets (per sample: p, q or None), last_clear / first_refused: the (scene, self)
    values of the last accepted and the first refused configuration of the edge checks).  max_samples: stop (status None) after that
    many samples -- the GPU tests use the prefix only."""
    dt = pb.dtype
    ch = Chain(pb, link, spec)
    a0, segs, bad = counts(ch, qrow, tpos, tquat, max_pos_step, max_rot_step)
    userot = tquat is not None
    S = sum(s["n"] for s in segs)
    two = hasattr(pb, "both")   # (a SelfProblem: the scene value and the self value)
    self_margin = getattr(pb, "self_margin", dt(0))
    margin = dt(margin)

    def values(q):
        if not two:
            return pb.clearance(q), dt(np.inf)   # (counts the configuration itself)
        pb.checked += 1
        return pb.both(q)

    out = dict(status=OK, points=[a0], S=S, iters=[], failed_segment=-1, targets=[], last_clear=None, first_refused=None, quotients=[s["quotient"] for s in segs])
    pb.checked = 0

    def done():
        pts = np.stack(out["points"])
        out.update(points=pts, n_points=len(pts), checked=pb.checked, fraction=dt(dt(len(pts) - 1) / dt(S)) if len(pts) > 1 else dt(0),
                   path=resample(pts, num_waypoints, dt) if num_waypoints else None)
        return out

    if bad:
        out["status"] = NOT_FINITE
        return done()
    if S + 1 > max_points:
        out["status"] = TOO_MANY_POINTS
        return done()
    if not ignore_collision:
        sc, sf = values(a0)
        if not sc >= margin:
            out["status"] = START_IN_COLLISION
            return done()
        if two and not sf >= self_margin:
            out["status"] = START_IN_SELF_COLLISION
            return done()
        out["last_clear"] = (sc, sf)
    prev, nsamp = a0, 0
    for k, s in enumerate(segs):
        for i in range(1, s["n"] + 1):
            if max_samples is not None and nsamp >= max_samples:
                out["status"] = None
                return done()
            nsamp += 1
            tp, tq = target(s["pa"], s["qa"], s["pb"], s["qb"], s["d"], s["sn"], s["ang"], i, s["n"], userot, dt)
            out["targets"].append((tp, tq))
            cand, epn, ern, iters = ik(ch, prev, tp, tq, ik_opts, dt)
            out["iters"].append(iters)
            op = {**IK_DEFAULTS, **ik_opts}
            status = OK
            if not (epn < dt(op["pos_tol"]) and ern < dt(op["rot_tol"])):
                status = IK_FAILED
            elif np.abs((cand - prev).astype(dt)).max() > dt(jump_threshold):
                status = JOINT_JUMP
            elif not ignore_collision:
                for q in plan_ref.edge_samples(prev, cand, resolution, dt):
                    sc, sf = values(q)
                    if not sc >= margin:
                        status = BLOCKED
                    elif two and not sf >= self_margin:
                        status = BLOCKED_SELF
                    if status != OK:
                        out["first_refused"] = (sc, sf)
                        break
                    out["last_clear"] = (sc, sf)
            if status != OK:
                out["status"], out["failed_segment"] = status, k
                return done()
            out["points"].append(cand)
            prev = cand
    return done()
