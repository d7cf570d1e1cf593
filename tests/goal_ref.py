"""Reference for mir_plan_path_goals (include/mirigid.h, "goal sets"): the rule of the header restated in NumPy, parametrised by dtype
like tests/plan_ref.py, whose Problem, u, edge_samples and resample it uses unchanged.  A helper, no test.  `dtype=np.float64` is the
reference, `dtype=np.float32` the float32 port the GPU tests take their yardstick from; both draw identical samples.

    goals:   the start's clear() first; then each goal g < n_goals: limits, clear(); the valid ones in ascending g.
    direct:  edge(start, goal_g) over the valid goals in ascending squared L2 distance (summed j ascending), the lower g on a tie.
    trees:   RRT-Connect of plan_ref.plan restated with Tb started as the forest of the valid goals; the parent walk of the extraction
             ends at whichever root it reaches, which is the row's goal.

    pose:    plan_pose() makes the goal set first, as mir_plan_path_pose does: for s = 0 .. max_samples - 1 the seed (the start, then every
             moving limited joint of the chain drawn by u(env, 0x40000000 | s, dof)), cart_ref.ik from it, and the candidate kept when it
             converged, lies inside the limits, is clear and is not within `dedup` of a kept one; then plan_goals() on the kept goals.

It shares no code with the HIP kernel.
"""
from __future__ import annotations

import numpy as np

import cart_ref
import plan_ref
from plan_ref import (GOAL_IN_COLLISION, GOAL_OUT_OF_LIMITS, ITERATION_LIMIT, MAX_POLY, NODE_LIMIT, OK, PATH_TOO_LONG, START_IN_COLLISION,
                      edge_samples, resample, u)

NO_VALID_GOAL = 9
MAX_GOALS = 8


def _dist2(a, b, dt):
    acc = dt(0)
    for x in (a - b).astype(dt):
        acc = dt(acc + x * x)
    return acc


def plan_goals(pb: plan_ref.Problem, qrow, goals, env, n_goals=None, W=16, max_nodes=128, max_iterations=512, smooth_passes=64, seed=0,
               resolution=0.05, step=0.3, margin=0.0, ignore_collision=False):
    """one row, goals (G, D) -> dict(status, poly (n_poly, D), path (W, D), iterations, nodes (na, nb), checked, goal_index,
    goal_status (G,))"""
    dt = pb.dtype
    start = pb.set_row(qrow)
    G = len(goals)
    assert 1 <= G <= MAX_GOALS < max_nodes
    ng = G if n_goals is None else min(max(int(n_goals), 0), G)
    pb.checked = 0
    margin, step = dt(margin), dt(step)
    clear = (lambda q: True) if ignore_collision else (lambda q: pb.clearance(q) >= margin)
    goal_status = np.full(G, -1, np.int32)

    def edge(a, b):
        return all(clear(q) for q in edge_samples(a, b, resolution, dt))

    def done(status, poly, gi=-1, it=0, na=1, nb=1):
        if status != OK:
            poly, gi = [start], -1
        poly = np.stack(poly)
        return dict(status=status, poly=poly, path=resample(poly, W, dt), iterations=it, nodes=(na, nb), checked=pb.checked, goal_index=gi,
                    goal_status=goal_status)

    if not clear(start):
        return done(START_IN_COLLISION, None)
    roots, root_goal = [], []
    for g in range(ng):
        with np.errstate(invalid="ignore"):
            q = np.asarray(goals[g]).astype(dt)
        if not np.isfinite(q).all() or ((q < pb.lo) | (q > pb.hi)).any():
            goal_status[g] = GOAL_OUT_OF_LIMITS
        elif not clear(q):
            goal_status[g] = GOAL_IN_COLLISION
        else:
            goal_status[g] = OK
            roots.append(q)
            root_goal.append(g)
    if not roots:
        return done(NO_VALID_GOAL, None)
    d2 = [_dist2(q, start, dt) for q in roots]
    for k in sorted(range(len(roots)), key=lambda k: (d2[k], k)):
        if edge(start, roots[k]):
            return done(OK, [start, roots[k]], root_goal[k])
    nodes, parent = [[start], list(roots)], [[-1], [-1] * len(roots)]

    def nearest(t, q):
        arr = np.stack(nodes[t])
        acc = np.zeros(len(arr), dt)
        for j in range(pb.D):
            e = (arr[:, j] - q[j]).astype(dt)
            acc = (acc + e * e).astype(dt)
        i = int(acc.argmin())
        return i, acc[i]

    poly, status, it_done, gi = None, ITERATION_LIMIT, 0, -1
    for it in range(max_iterations):
        it_done = it + 1
        t, o = it & 1, (it & 1) ^ 1
        qr = np.array([pb.lo[j] + dt(u(seed, env, it, j)) * (pb.hi[j] - pb.lo[j]) for j in range(pb.D)], dt)
        near, dn = nearest(t, qr)
        nv = nodes[t][near]
        with np.errstate(divide="ignore"):
            sc = min(dt(1), dt(step / np.sqrt(dn)))
        qn = (nv + sc * (qr - nv)).astype(dt)
        if not edge(nv, qn):
            continue
        if len(nodes[t]) >= max_nodes:
            status = NODE_LIMIT
            break
        nodes[t].append(qn)
        parent[t].append(near)
        inew = len(nodes[t]) - 1
        ci, _ = nearest(o, qn)
        cv, met, full = nodes[o][ci], False, False
        for _ in range(max_nodes):
            diff = (qn - cv).astype(dt)
            d = np.sqrt(_dist2(qn, cv, dt))
            last = d <= step
            tv = qn if last else (cv + dt(step / d) * diff).astype(dt)
            if not edge(cv, tv):
                break
            if len(nodes[o]) >= max_nodes:
                full = True
                break
            nodes[o].append(tv)
            parent[o].append(ci)
            ci, cv = len(nodes[o]) - 1, tv
            if last:
                met = True
                break
        if full:
            status = NODE_LIMIT
            break
        if not met:
            continue
        ia, ib = (ci, inew) if t else (inew, ci)
        head, n = [], ia
        while n >= 0:
            head.append(nodes[0][n])
            n = parent[0][n]
        tail, n, root = [], parent[1][ib], ib   # (the meeting node is in both trees: once)
        while n >= 0:
            tail.append(nodes[1][n])
            root, n = n, parent[1][n]
        poly, gi = head[::-1] + tail, root_goal[root]
        status = PATH_TOO_LONG if len(poly) > MAX_POLY else OK
        break
    na, nb = len(nodes[0]), len(nodes[1])
    if status != OK:
        return done(status, None, -1, it_done, na, nb)
    for s in range(smooth_passes):
        n = len(poly)
        if n < 3:
            break
        c = 0x80000000 | s
        i = min(int(np.float32(u(seed, env, c, 0) * np.float32(n - 2))), n - 3)
        j = i + 2 + min(int(np.float32(u(seed, env, c, 1) * np.float32(n - 2 - i))), n - 3 - i)
        if edge(poly[i], poly[j]):
            poly = poly[:i + 1] + poly[j:]
    return done(OK, poly, gi, it_done, na, nb)


NOT_FINITE = cart_ref.NOT_FINITE


def sample_goals(pb: plan_ref.Problem, ch: cart_ref.Chain, start, tp, tq, env, max_goals=4, max_samples=16, dedup=0.05, seed=0, margin=0.0,
                 ignore_collision=False, **ik_opts):
    """the goal set of one row at the start row last given to pb.set_row() -> (kept (n, D), stats [tried, converged, rejected, iterations])"""
    dt = pb.dtype
    op = {**cart_ref.IK_DEFAULTS, **ik_opts}
    pos_tol, rot_tol = dt(op["pos_tol"]), dt(op["rot_tol"])
    tp = np.asarray(tp).astype(dt)
    tq = None if tq is None else np.asarray(tq).astype(dt)
    if tq is not None:
        tq = (tq / np.sqrt((tq * tq).sum(dtype=dt))).astype(dt)
    kept, tried, conv, rej, iters = [], 0, 0, 0, 0
    for s in range(max_samples):
        if len(kept) >= max_goals:
            break
        tried += 1
        cfg = start.copy()
        if s > 0:
            for c, j in enumerate(ch.dof):
                if ch.limited[c]:
                    cfg[j] = dt(ch.lo[c] + dt(dt(u(seed, env, 0x40000000 | s, j)) * dt(ch.hi[c] - ch.lo[c])))
        q, epn, ern, it = cart_ref.ik(ch, cfg, tp, tq, ik_opts, dt)
        iters += it
        if not (epn < pos_tol and ern < rot_tol):
            continue
        conv += 1
        cand = start.copy()
        cand[ch.dof] = q[ch.dof]
        if not np.isfinite(cand).all() or ((cand < pb.lo) | (cand > pb.hi)).any():
            rej += 1
            continue
        if not ignore_collision and not pb.clearance(cand) >= dt(margin):
            rej += 1
            continue
        if any(np.abs(cand - k).max() < dt(dedup) for k in kept):
            continue
        kept.append(cand)
    return kept, [tried, conv, rej, iters]


def plan_pose(pb: plan_ref.Problem, spec, link, qrow, tp, tq, env, max_goals=4, max_samples=16, dedup=None, ik_opts=None, **plan_kw):
    """one row -> the dict of plan_goals plus goals (n_goals, D), n_goals, goal_stats"""
    dt = pb.dtype
    W = plan_kw.get("W", 16)
    start = pb.set_row(qrow)
    stay = dict(status=NOT_FINITE, poly=start[None], path=resample(start[None], W, dt), iterations=0, nodes=(1, 1), checked=0, goal_index=-1,
                goal_status=np.full(max_goals, -1, np.int32), goals=np.zeros((0, pb.D), dt), n_goals=0, goal_stats=[0, 0, 0, 0])
    bad = not np.isfinite(np.asarray(tp, np.float64)).all()
    if tq is not None:
        t = np.asarray(tq, np.float32)
        bad = bad or not np.isfinite(t).all() or not float((t.astype(np.float64) ** 2).sum()) >= 1e-30
    if bad:
        return stay
    margin, ignore = plan_kw.get("margin", 0.0), plan_kw.get("ignore_collision", False)
    if not ignore and not pb.clearance(start) >= dt(margin):
        return {**stay, "status": START_IN_COLLISION}
    ch = cart_ref.Chain(pb, link, spec)
    kept, stats = sample_goals(pb, ch, start, tp, tq, env, max_goals, max_samples, plan_kw.get("resolution", 0.05) if dedup is None else dedup,
                               plan_kw.get("seed", 0), margin, ignore, **(ik_opts or {}))
    if not kept:
        return {**stay, "status": NO_VALID_GOAL, "goal_stats": stats}
    out = plan_goals(pb, qrow, np.stack(kept), env, **plan_kw)
    gs = np.full(max_goals, -1, np.int32)
    gs[:len(kept)] = out["goal_status"]
    out.update(goal_status=gs, goals=np.stack(kept), n_goals=len(kept), goal_stats=stats)
    return out
