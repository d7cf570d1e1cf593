"""Reference for mir_certify_path_self / mir_certify_path_carry (include/mirigid.h, "certified clearance: self and carried object"): the
rule of the header restated in NumPy on self_ref.SelfProblem / carry_ref.CarryProblem, parametrised by the problem's dtype.  A helper, no
test.  A float64 problem gives the reference; a float32 problem gives the float32 port (every intermediate rounded to float32) that the
GPU tests take their yardstick from.  It is built on cert_ref (chains, midpoint, successor, tiles), self_ref and carry_ref.

    eff(pb)                  per body the link it counts as (the carried body: its attach link)
    lca(pb)                  (nbody, nbody): the chain depth of the lowest common ancestor-or-self, 255: none
    cn(pb)                   per sphere the bound on |centre| in its link's frame (|p_G| + |c_i| on the carried body)
    branch(pb, a, b)         per body the rows (dA, dSB, dP) after 0 .. depth + 1 bodies of the walk upward, and S, A, B, P
    speeds(pb, a, b)         v (N,) of the scene test and V (N + E, N + E) of the pair test
    evaluate(pb, q, hw, v, V)   one evaluation -> u, m, u_s, m_s, or None when a centre is not finite
    certify(pb, qrow, path)  one row -> the outputs of the entry point, the leaves, and every evaluated node
    replay(...)              the bisection of one segment on a GIVEN set of leaves
    dense_min(pb, qrow, path, n)   the brute force: both minima over n + 1 equally spaced configurations per segment, float64, batched

It shares no code with the HIP kernel and none with csrc/mir_certrel_front.h.
"""
from __future__ import annotations

import numpy as np

import cert_ref
import dist_ref
import kin_ref
from cert_ref import BLOCKED, BUDGET, CLEAR, DEPTH, NOT_FINITE, UNDECIDED, FACTOR  # noqa: F401

NONE = 255


def _carry(pb):
    return (int(pb.body), int(pb.link)) if hasattr(pb, "body") else (-1, -1)


def eff(pb):
    C, Lk = _carry(pb)
    return [Lk if b == C else b for b in range(pb.model.nbody)]


def _struct(pb):
    """per body: whether it starts a chain, its chain depth, its ancestors-or-self inside the chain (nearest first)"""
    if getattr(pb, "_certrel", None) is None:
        m = pb.model
        root = [True] + [m.parent[b] == 0 or m.jtype[b] == kin_ref.FREE for b in range(1, m.nbody)]
        up = [[] for _ in range(m.nbody)]
        for b in range(1, m.nbody):
            k = b
            while True:
                up[b].append(k)
                if root[k]:
                    break
                k = m.parent[k]
        depth = [len(u) - 1 for u in up]
        pb._certrel = dict(root=root, up=up, depth=depth)
    return pb._certrel


def lca(pb):
    st, e = _struct(pb), eff(pb)
    n = pb.model.nbody
    out = np.full((n, n), NONE, int)
    for a in range(n):
        for b in range(n):
            ua, ub = st["up"][e[a]], set(st["up"][e[b]])
            common = [k for k in ua if k in ub]
            if common:
                out[a, b] = st["depth"][common[0]]
    return out


def _norm(v, dt):
    return dt(np.sqrt(dt(dt(dt(v[0] * v[0]) + dt(v[1] * v[1])) + dt(v[2] * v[2]))))


def cn(pb):
    """(N + E,) in pb.dtype, at the row last given to pb.set_row() (the carried body's grasp is the row's)"""
    dt = pb.dtype
    C, _ = _carry(pb)
    out = np.array([_norm(c, dt) for c in pb.probes[:, :3]], dt)
    if C >= 0:
        g = _norm(pb.G[0].astype(dt), dt)
        on = pb.links == C
        out[on] = (g + out[on]).astype(dt)
    return out


def branch(pb, a, b):
    """-> rows: per body an array (depth + 2, 3) of (dA, dSB, dP) after t = 0, 1, ... bodies of the walk a, parent(a), ...; S, A, B, P with
    the carried body's entries those of its attach link"""
    m, dt, st, e = pb.model, pb.dtype, _struct(pb), eff(pb)
    cst = cert_ref._structure(pb)
    S, A, B, P, _ = cert_ref.chains(pb, a, b)
    S, A, B, P = (x.copy() for x in (S, A, B, P))
    for k in range(m.nbody):
        if e[k] != k:
            S[k], A[k], B[k], P[k] = S[e[k]], A[e[k]], B[e[k]], P[e[k]]
    adq = np.abs((np.asarray(b).astype(dt) - np.asarray(a).astype(dt)).astype(dt))
    rows = []
    for body in range(m.nbody):
        dA, dSB, dP = dt(0), dt(0), dt(0)
        out = [(dA, dSB, dP)]
        for k in (st["up"][e[body]] if e[body] > 0 else []):
            j = cst["jd"][k]
            if j >= 0 and m.jtype[k] == kin_ref.REVOLUTE:
                dA = dt(dA + adq[j])
                dSB = dt(dSB + dt(adq[j] * dt(S[e[body]] - S[k])))
            elif j >= 0:
                dP = dt(dP + dt(adq[j] * cst["axis_len"][k]))
            out.append((dA, dSB, dP))
        rows.append(np.array(out, dt))
    return rows, S, A, B, P


def steps(pb, la, lb):
    """how many bodies of the walk from link la enter rel(., lca(la, lb))"""
    st, e = _struct(pb), eff(pb)
    if e[la] == 0:
        return 0
    c = lca(pb)[la, lb] if getattr(pb, "_lca", None) is None else pb._lca[la, lb]
    return st["depth"][e[la]] + 1 if c == NONE else st["depth"][e[la]] - c


def speeds(pb, a, b):
    """v (N,): the scene test's speed bounds; V (N + E, N + E): v_ij of the pair test; in pb.dtype"""
    dt, e = pb.dtype, eff(pb)
    if getattr(pb, "_lca", None) is None:
        pb._lca = lca(pb)
    rows, S, A, B, P = branch(pb, a, b)
    c = cn(pb)
    n = pb.model.nbody
    T = np.zeros((n, n, 3), dt)
    for x in range(n):
        for y in range(n):
            T[x, y] = rows[x][steps(pb, x, y)]
    lk = pb.links
    Tij = T[lk[:, None], lk[None, :]]                                        # (NS, NS, 3): the branch of i against j's link
    rel = (((c[:, None] * Tij[..., 0]).astype(dt) + Tij[..., 1]).astype(dt) + Tij[..., 2]).astype(dt)
    V = np.maximum(((rel + rel.T).astype(dt) * dt(FACTOR)).astype(dt), dt(0)).astype(dt)
    el = np.array([e[k] for k in lk])
    N = getattr(pb, "N", len(lk))
    v = ((((S[el] + c).astype(dt) * A[el]).astype(dt) - B[el]).astype(dt) + P[el]).astype(dt)
    v = np.maximum((v * dt(FACTOR)).astype(dt), dt(0)).astype(dt)
    return v[:N], V


def pair_distances(pb, pw):
    """s_ij (N + E, N + E) in the arithmetic of self_ref.SelfProblem.self_distances, +inf where the pair is not enabled"""
    dt = pb.dtype
    d = (pw[:, None, :] - pw[None, :, :]).astype(dt)
    n2 = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype(dt) + d[..., 2] * d[..., 2]).astype(dt)
    r = pb.probes[:, 3]
    s = (np.sqrt(n2).astype(dt) - (r[:, None] + r[None, :]).astype(dt)).astype(dt)
    return np.where(pb.enabled, s, dt(np.inf))


def evaluate(pb, q, hw, v, V, self_on=True):
    """-> (u, m, u_s, m_s, L) at the planned dofs q, None when a centre (or q) is not finite; L: the largest |coordinate| of a centre"""
    dt = pb.dtype
    with np.errstate(invalid="ignore"):
        pw = pb.centres(q)
    if not (np.isfinite(pw).all() and np.isfinite(np.asarray(q, np.float64)).all()):
        return None
    N = getattr(pb, "N", len(pw))
    d = np.full(N, pb.max_distance, dt)
    for geom, c, Rg in pb.frames:
        g = dist_ref.geom_distance(geom, ((pw[:N] - c) @ Rg).astype(dt), dt)[0]
        d = np.minimum(d, (g - pb.probes[:N, 3]).astype(dt))
    u, m = dt(d.min()), dt((d - (hw * v).astype(dt)).astype(dt).min())
    us = ms = dt(np.inf)
    if self_on:
        s = pair_distances(pb, pw)
        us = dt(min(pb.self_max, s.min()))
        bound = (np.minimum(s, pb.self_max).astype(dt) - (hw * V).astype(dt)).astype(dt)
        ms = dt(min(pb.self_max, np.where(pb.enabled, bound, dt(np.inf)).min()))
    return u, m, us, ms, float(np.abs(pw).max())


def certify(pb, qrow, path, margin=0.0, tol=0.002, guard=1e-5, max_depth=12, max_evaluations=4096, bracket=False, ignore=False, self_on=True):
    """one row -> dict(seg_lower, seg_upper, seg_self_lower, seg_self_upper (K-1,), seg_status, row_*, row_first, leaves [(s, l, k)], stats
    (evaluations, leaves, deepest, finished), nodes [dict(s, l, k, q, u, lo, us, lo_s, leaf, upper, upper_s)], ends [dict(s, q, u, us)])"""
    dt = pb.dtype
    pb.set_row(qrow)
    bad = bool(getattr(pb, "blocked", False))
    path = np.asarray(path).astype(dt)
    margin, tol, guard = dt(np.float32(margin)), dt(np.float32(tol)), dt(np.float32(guard))
    smargin = pb.self_margin if self_on else dt(0)
    K = len(path)
    inf = dt(np.inf)
    lower, upper, lower_s, upper_s = (np.full(K - 1, inf, dt) for _ in range(4))
    status = np.zeros(K - 1, int)
    leaves, nodes, ends = [], [], []
    evals, deepest, finished, spent = 0, 0, 0, False

    def leaf_test(lo, up, mg):
        return (not bracket and lo >= mg) or lo >= dt(up - tol)

    for s in range(K - 1):
        a, b = path[s], path[s + 1]
        with np.errstate(invalid="ignore", over="ignore"):
            dq = (b - a).astype(dt)
        lo_S, up_S, lo_SS, up_SS = inf, inf, inf, inf
        nf, budget, depth_hit = bad, False, False
        if ignore:
            lower[s] = upper[s] = pb.max_distance
            lower_s[s] = upper_s[s] = pb.self_max if self_on else inf
            finished += 1
            continue
        if not nf and not (np.isfinite(a).all() and np.isfinite(b).all() and np.isfinite(dq).all()):
            nf = True
        if not nf and spent:
            budget = True
        if not nf and not budget:
            v, V = speeds(pb, a, b)
            ended = False
            for e in ((0, 1) if s == 0 else (1,)):
                if evals >= max_evaluations:
                    budget = ended = True
                    break
                evals += 1
                q = a if e == 0 else b
                w = evaluate(pb, q, dt(0), v, V, self_on)
                if w is None:
                    nf = ended = True
                    break
                u, m, us, ms, _ = w
                ends.append(dict(s=s, q=q.copy(), u=u, us=us))
                up_S, up_SS = min(up_S, u), min(up_SS, us)
                if not bracket and (u < margin or (self_on and us < smargin)):
                    lo_S, lo_SS = min(lo_S, dt(m - guard)), min(lo_SS, dt(ms - guard))
                    ended = True
                    break
            l, k = 0, 0
            while not ended:
                if evals >= max_evaluations:
                    budget = True
                    break
                evals += 1
                q, tm, hw = cert_ref.midpoint(a, dq, l, k, dt)
                w = evaluate(pb, q, hw, v, V, self_on)
                if w is None:
                    nf = True
                    break
                deepest = max(deepest, l)
                u, m, us, ms, _ = w
                lo, lo_s = dt(m - guard), dt(ms - guard)
                up_S, up_SS = min(up_S, u), min(up_SS, us)
                node = dict(s=s, l=l, k=k, q=q, u=u, lo=lo, us=us, lo_s=lo_s, leaf=False, upper=up_S, upper_s=up_SS, hw=hw)
                nodes.append(node)
                if not bracket and (u < margin or (self_on and us < smargin)):
                    lo_S, lo_SS = min(lo_S, lo), min(lo_SS, lo_s)
                    node["witness"] = True
                    break
                leaf = leaf_test(lo, up_S, margin) and (not self_on or leaf_test(lo_s, up_SS, smargin))
                if l >= max_depth and not leaf:
                    depth_hit = leaf = True
                    node["forced"] = True
                if leaf:
                    node["leaf"] = True
                    lo_S, lo_SS = min(lo_S, lo), min(lo_SS, lo_s)
                    leaves.append((s, l, k))
                    l, k, done = cert_ref.successor(l, k)
                    if done:
                        finished += 1
                        break
                else:
                    l, k = l + 1, 2 * k
        spent = spent or budget
        if nf or budget:
            lo_S = lo_SS = -inf
        lower[s], upper[s], lower_s[s], upper_s[s] = lo_S, up_S, lo_SS, up_SS
        blocked = up_S < margin or (self_on and up_SS < smargin)
        clear = lo_S >= margin and (not self_on or lo_SS >= smargin)
        status[s] = NOT_FINITE if nf else BUDGET if budget else BLOCKED if blocked else DEPTH if depth_hit else CLEAR if clear else UNDECIDED
    notclear = np.flatnonzero(status != CLEAR)
    return dict(seg_lower=lower, seg_upper=upper, seg_self_lower=lower_s, seg_self_upper=upper_s, seg_status=status, row_lower=lower.min(),
                row_upper=upper.min(), row_self_lower=lower_s.min(), row_self_upper=upper_s.min(), row_status=int(status.max()),
                row_first=int(notclear[0]) if len(notclear) else -1, leaves=leaves, stats=(evals, len(leaves), deepest, finished), nodes=nodes,
                ends=ends)


def replay(pb, qrow, path, s, leaves, guard, self_on=True):
    """the bisection of segment s replayed on a GIVEN set of leaves [(l, k)] in pb.dtype -> [dict(l, k, u, lo, us, lo_s, leaf, upper, upper_s,
    reach, L)] with the running minima that include the segment's endpoints (P_0 for segment 0 only); reach: the largest hw v_i or hw v_ij
    over the enabled pairs; L: the largest |coordinate| of a centre.  The leaves must tile [0, 1]."""
    dt = pb.dtype
    pb.set_row(qrow)
    path = np.asarray(path).astype(dt)
    a, b = path[s], path[s + 1]
    dq = (b - a).astype(dt)
    v, V = speeds(pb, a, b)
    vmax = max(float(v.max()), float(np.where(pb.enabled, V, 0).max()) if self_on else 0.0)
    guard = dt(np.float32(guard))
    upper, upper_s = dt(np.inf), dt(np.inf)
    for q in (([a] if s == 0 else []) + [b]):
        w = evaluate(pb, q, dt(0), v, V, self_on)
        upper, upper_s = min(upper, w[0]), min(upper_s, w[2])
    want, out = set(leaves), []
    l, k = 0, 0
    for _ in range(4 * len(want) + 4):
        q, _, hw = cert_ref.midpoint(a, dq, l, k, dt)
        u, m, us, ms, L = evaluate(pb, q, hw, v, V, self_on)
        upper, upper_s = min(upper, u), min(upper_s, us)
        leaf = (l, k) in want
        out.append(dict(l=l, k=k, u=u, lo=dt(m - guard), us=us, lo_s=dt(ms - guard), leaf=leaf, upper=upper, upper_s=upper_s,
                        reach=float(hw) * vmax, L=L))
        if leaf:
            l, k, done = cert_ref.successor(l, k)
            if done:
                return out
        else:
            l, k = l + 1, 2 * k
    raise AssertionError("the leaves do not tile [0, 1]")


# ---- the brute force, batched over configurations (float64)
def centres_batch(pb, Q):
    """sphere centres (T, N + E, 3) in the world at the planned dofs Q (T, D), float64, at the row last given to pb.set_row(); the carried
    body rides on its attach link by the row's grasp"""
    m = pb.model
    Q = np.asarray(Q, np.float64)
    T = len(Q)
    q = np.repeat(np.asarray(pb.q, np.float64)[None], T, 0)
    q[:, pb.qadr] = Q
    xp = np.repeat(np.asarray(pb.xp, np.float64)[None], T, 0)
    xq = np.repeat(np.asarray(pb.xq, np.float64)[None], T, 0)
    bpos, bquat, axis = (np.asarray(x, np.float64) for x in (pb.bpos, pb.bquat, pb.axis))
    for b in range(1, m.nbody):
        if not pb.moves[b]:
            continue
        jt, qa = m.jtype[b], m.qadr[b]
        P, Qx = np.repeat(bpos[b][None], T, 0), np.repeat(bquat[b][None], T, 0)
        if jt == kin_ref.REVOLUTE:
            h = 0.5 * q[:, qa]
            Qx = cert_ref._qmul(Qx, np.concatenate([np.cos(h)[:, None], axis[b][None] * np.sin(h)[:, None]], 1))
        elif jt == kin_ref.PRISMATIC:
            P = P + cert_ref._qrot(Qx, q[:, qa, None] * axis[b][None])
        par = m.parent[b]
        if par > 0:
            P, Qx = xp[:, par] + cert_ref._qrot(xq[:, par], P), cert_ref._qmul(xq[:, par], Qx)
        xp[:, b], xq[:, b] = P, Qx
    C, Lk = _carry(pb)
    if C >= 0:
        pG, qG = (np.asarray(x, np.float64) for x in pb.G)
        xp[:, C] = xp[:, Lk] + cert_ref._qrot(xq[:, Lk], np.repeat(pG[None], T, 0))
        xq[:, C] = cert_ref._qmul(xq[:, Lk], np.repeat(qG[None], T, 0))
    pr = np.asarray(pb.probes, np.float64)
    return xp[:, pb.links] + cert_ref._qrot(xq[:, pb.links], pr[None, :, :3])


def both_batch(pb, Q):
    """(scene clearance (T,), self clearance (T,) capped at self_max) of the configurations Q (T, D), float64"""
    pw = centres_batch(pb, Q)
    T = pw.shape[0]
    N = getattr(pb, "N", pw.shape[1])
    d = np.full((T, N), float(pb.max_distance))
    flat = pw[:, :N].reshape(-1, 3)
    rad = np.asarray(pb.probes[:, 3], np.float64)
    for geom, c, Rg in pb.frames:
        g = dist_ref.geom_distance(geom, (flat - np.asarray(c, np.float64)) @ np.asarray(Rg, np.float64), np.float64)[0]
        d = np.minimum(d, g.reshape(T, N) - rad[None, :N])
    own = np.full(T, float(pb.self_max))
    ii, jj = np.nonzero(np.triu(pb.enabled, 1))
    if len(ii):
        for t0 in range(0, T, 256):
            s = np.linalg.norm(pw[t0:t0 + 256, ii] - pw[t0:t0 + 256, jj], axis=2) - (rad[ii] + rad[jj])[None]
            own[t0:t0 + 256] = np.minimum(own[t0:t0 + 256], s.min(1))
    return d.min(1), own


def dense_min(pb, qrow, path, n=2048):
    """the minima of both clearances over t = i / n, i = 0 .. n, on every segment of the path (float64) -> (K-1,), (K-1,)"""
    pb.set_row(qrow)
    path = np.asarray(path, np.float64)
    t = np.arange(n + 1)[:, None] / n
    scene, own = [], []
    for s in range(len(path) - 1):
        a, b = path[s], path[s + 1]
        Q = a[None] if np.array_equal(a, b) else a[None] + t * (b - a)[None]
        x, y = both_batch(pb, Q)
        scene.append(float(x.min()))
        own.append(float(y.min()))
    return np.array(scene), np.array(own)
