"""Reference for mir_certify_path (include/mirigid.h, "certified clearance"): the rule of the header restated in NumPy on
plan_ref.Problem, parametrised by the problem's dtype.  A helper, no test.  A float64 problem gives the reference; a float32 problem gives
the float32 port (every intermediate rounded to float32) that the GPU tests take their yardstick from.

    chains(pb, a, b)        steps 1 and 2: S, A, B, P per body and v per probe, parent before child
    rho(pb, a, b)           rho_ij (N, D) in float64 straight from the spec: the chain between joint j's anchor and probe i
    per_probe(pb, qp)       d_i: the capped (distance - radius) of every probe at the planned dofs qp, None when a centre is not finite
    certify(pb, qrow, path) steps 3 - 8 of one row -> the outputs of the entry point, the leaves, and every evaluated node
    dense_min(pb, qrow, path, n)   the brute force: the minimum over n + 1 equally spaced configurations per segment, float64, batched

It shares no code with the HIP kernel and none with csrc/mir_cert_front.h.
"""
from __future__ import annotations

import numpy as np

import dist_ref
import kin_ref

CLEAR, UNDECIDED, DEPTH, BUDGET, BLOCKED, NOT_FINITE = range(6)
FACTOR = np.float32(1.0001)


def _structure(pb):
    """what does not depend on the segment: per body its parent, whether it starts a chain, |pos|, |axis|, its planned dof (-1: none)"""
    if getattr(pb, "_cert", None) is None:
        m, dt = pb.model, pb.dtype
        root = [True] + [m.parent[b] == 0 or m.jtype[b] == kin_ref.FREE for b in range(1, m.nbody)]
        norm = lambda v: dt(np.sqrt(dt(dt(dt(v[0] * v[0]) + dt(v[1] * v[1])) + dt(v[2] * v[2]))))  # noqa: E731
        pos_len = [dt(0) if m.jtype[b] == kin_ref.FREE or b == 0 else norm(pb.bpos[b]) for b in range(m.nbody)]
        axis_len = [norm(pb.axis[b]) if m.jtype[b] == kin_ref.PRISMATIC else dt(0) for b in range(m.nbody)]
        jd = [-1] * m.nbody
        for j, qa in enumerate(pb.qadr):
            b = next(b for b in range(1, m.nbody) if m.qadr[b] == qa and m.jtype[b] in (kin_ref.REVOLUTE, kin_ref.PRISMATIC))
            jd[b] = j
        cn = np.array([norm(c) for c in pb.probes[:, :3]], dt)
        pb._cert = dict(root=root, pos_len=pos_len, axis_len=axis_len, jd=jd, cn=cn)
    return pb._cert


def chains(pb, a, b):
    """S, A, B, P (nbody,) and v (N,) of the segment a -> b (planned dofs) at the row last given to pb.set_row(), in pb.dtype"""
    m, dt, st = pb.model, pb.dtype, _structure(pb)
    a, b = np.asarray(a).astype(dt), np.asarray(b).astype(dt)
    adq = np.abs((b - a).astype(dt))
    amax = np.maximum(np.abs(a), np.abs(b))
    S, A, Bs, P = (np.zeros(m.nbody, dt) for _ in range(4))
    for k in range(1, m.nbody):
        jt, j, par, rt = m.jtype[k], st["jd"][k], m.parent[k], st["root"][k]
        pris = dt(0)
        if jt == kin_ref.PRISMATIC:
            pris = dt((amax[j] if j >= 0 else abs(pb.q[m.qadr[k]])) * st["axis_len"][k])
        S[k] = dt(0) if rt else dt(dt(S[par] + st["pos_len"][k]) + pris)
        kind = 0 if j < 0 else (1 if jt == kin_ref.REVOLUTE else 2)
        d = adq[j] if j >= 0 else dt(0)
        base = (lambda x: dt(0)) if rt else (lambda x: x[par])
        A[k] = dt(base(A) + (d if kind == 1 else dt(0)))
        Bs[k] = dt(base(Bs) + (dt(d * S[k]) if kind == 1 else dt(0)))
        P[k] = dt(base(P) + (dt(d * st["axis_len"][k]) if kind == 2 else dt(0)))
    lk = pb.links
    v = dt(1) * ((((S[lk] + st["cn"]).astype(dt) * A[lk]).astype(dt) - Bs[lk]).astype(dt) + P[lk]).astype(dt)
    v = (v * dt(FACTOR)).astype(dt)
    return S, A, Bs, P, np.maximum(v, dt(0)).astype(dt)


def rho(pb, a, b):
    """rho_ij (N, D), float64, from the spec: for a revolute dof j on probe i's chain the sum of |pos| + slide over the bodies between
    joint j's body (excluded) and the probe's link (included) plus |c_i|; for a prismatic one |axis_j|; 0 off the chain"""
    m = pb.model
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    body_of = {}
    for j, qa in enumerate(pb.qadr):
        body_of[next(k for k in range(1, m.nbody) if m.qadr[k] == qa and m.jtype[k] in (kin_ref.REVOLUTE, kin_ref.PRISMATIC))] = j
    out = np.zeros((len(pb.probes), pb.D))
    for i, link in enumerate(pb.links):
        length, k = float(np.linalg.norm(np.asarray(pb.probes[i, :3], np.float64))), int(link)
        while k > 0:
            j = body_of.get(k, -1)
            if j >= 0:
                out[i, j] = length if m.jtype[k] == kin_ref.REVOLUTE else float(np.linalg.norm(np.asarray(pb.axis[k], np.float64)))
            if m.parent[k] == 0 or m.jtype[k] == kin_ref.FREE:
                break
            slide = 0.0
            if m.jtype[k] == kin_ref.PRISMATIC:
                slide = (max(abs(a[j]), abs(b[j])) if j >= 0 else abs(float(pb.q[m.qadr[k]]))) * float(np.linalg.norm(np.asarray(pb.axis[k], np.float64)))
            length += float(np.linalg.norm(np.asarray(pb.bpos[k], np.float64))) + slide
            k = m.parent[k]
    return out


def per_probe(pb, qp):
    """d_i (N,) at the planned dofs qp: min over the tested geoms of (distance - radius), capped at max_distance; None: not finite"""
    dt = pb.dtype
    pw = pb.centres(qp)
    if not (np.isfinite(pw).all() and np.isfinite(np.asarray(qp, np.float64)).all()):
        return None
    d = np.full(len(pb.probes), pb.max_distance, dt)
    for geom, c, Rg in pb.frames:
        g = dist_ref.geom_distance(geom, ((pw - c) @ Rg).astype(dt), dt)[0]
        d = np.minimum(d, (g - pb.probes[:, 3]).astype(dt))
    return d.astype(dt)


def midpoint(a, dq, l, k, dt):
    """the configuration of node (l, k): fmaf(tm, dq, a) per dof, and tm, hw"""
    tm, hw = dt((2 * k + 1) * 2.0 ** -(l + 1)), dt(2.0 ** -(l + 1))
    q = np.float64(tm) * dq.astype(np.float64) + a.astype(np.float64)   # (float32: the product is exact in float64, one rounding follows)
    return q.astype(dt), tm, hw


def successor(l, k):
    """the dyadic successor of an accepted leaf -> (l, k, done)"""
    while k & 1:
        k >>= 1
        l -= 1
    if l == 0:
        return l, k, True
    return l, k + 1, False


def certify(pb, qrow, path, margin=0.0, tol=0.002, guard=1e-5, max_depth=12, max_evaluations=4096, bracket=False, ignore=False, bad=False):
    """one row -> dict(seg_lower, seg_upper (K-1,), seg_status, row_lower, row_upper, row_status, row_first, leaves [(s, l, k)], stats
    (evaluations, leaves, deepest, finished), nodes [dict(s, l, k, q, u, lo, leaf, upper)], ends [dict(s, q, u)], v [per segment])"""
    dt = pb.dtype
    pb.set_row(qrow)
    path = np.asarray(path).astype(dt)
    margin, tol, guard = dt(np.float32(margin)), dt(np.float32(tol)), dt(np.float32(guard))
    K = len(path)
    inf = dt(np.inf)
    lower, upper, status = np.full(K - 1, inf, dt), np.full(K - 1, inf, dt), np.zeros(K - 1, int)
    leaves, nodes, ends, vs = [], [], [], []
    evals, deepest, finished, spent = 0, 0, 0, False
    for s in range(K - 1):
        a, b = path[s], path[s + 1]
        with np.errstate(invalid="ignore", over="ignore"):
            dq = (b - a).astype(dt)
        lo_s, up_s = inf, inf
        nf, budget, depth_hit = bool(bad), False, False
        vs.append(None)
        if ignore:
            lower[s] = upper[s] = pb.max_distance
            finished += 1
            continue
        if not nf and not (np.isfinite(a).all() and np.isfinite(b).all() and np.isfinite(dq).all()):
            nf = True
        if not nf and spent:
            budget = True
        if not nf and not budget:
            v = chains(pb, a, b)[4]
            vs[-1] = v
            ended = False
            for e in ((0, 1) if s == 0 else (1,)):
                if evals >= max_evaluations:
                    budget = ended = True
                    break
                evals += 1
                q = a if e == 0 else b
                d = per_probe(pb, q)
                if d is None:
                    nf = ended = True
                    break
                u = dt(d.min())
                ends.append(dict(s=s, q=q.copy(), u=u))
                up_s = min(up_s, u)
                if not bracket and u < margin:
                    lo_s = min(lo_s, dt(u - guard))
                    ended = True
                    break
            l, k = 0, 0
            while not ended:
                if evals >= max_evaluations:
                    budget = True
                    break
                evals += 1
                q, tm, hw = midpoint(a, dq, l, k, dt)
                d = per_probe(pb, q)
                if d is None:
                    nf = True
                    break
                deepest = max(deepest, l)
                u = dt(d.min())
                lo = dt(dt((d - (hw * v).astype(dt)).astype(dt).min()) - guard)
                up_s = min(up_s, u)
                node = dict(s=s, l=l, k=k, q=q, u=u, lo=lo, leaf=False, upper=up_s, hw=hw)
                nodes.append(node)
                if not bracket and u < margin:
                    lo_s = min(lo_s, lo)
                    node["witness"] = True
                    break
                leaf = (not bracket and lo >= margin) or lo >= dt(up_s - tol)
                if l >= max_depth and not leaf:
                    depth_hit = leaf = True
                    node["forced"] = True
                if leaf:
                    node["leaf"] = True
                    lo_s = min(lo_s, lo)
                    leaves.append((s, l, k))
                    l, k, done = successor(l, k)
                    if done:
                        finished += 1
                        break
                else:
                    l, k = l + 1, 2 * k
        spent = spent or budget
        if nf or budget:
            lo_s = -inf
        lower[s], upper[s] = lo_s, up_s
        status[s] = (NOT_FINITE if nf else BUDGET if budget else BLOCKED if up_s < margin else DEPTH if depth_hit else
                     CLEAR if lo_s >= margin else UNDECIDED)
    notclear = np.flatnonzero(status != CLEAR)
    return dict(seg_lower=lower, seg_upper=upper, seg_status=status, row_lower=lower.min(), row_upper=upper.min(), row_status=int(status.max()),
                row_first=int(notclear[0]) if len(notclear) else -1, leaves=leaves, stats=(evals, len(leaves), deepest, finished), nodes=nodes,
                ends=ends, v=vs)


def replay(pb, qrow, path, s, leaves, guard, v=None):
    """the bisection of segment s replayed on a GIVEN set of leaves [(l, k)] in pb.dtype: the nodes the rule evaluates for that tree,
    in its order -> [dict(l, k, u, lo, leaf, upper, reach, L)] with `upper` the running minimum that includes the segment's endpoints
    (P_0 for segment 0 only); reach = max_i hw v_i; L = the largest |coordinate| of a probe centre.  The leaves must tile [0, 1]."""
    dt = pb.dtype
    pb.set_row(qrow)
    path = np.asarray(path).astype(dt)
    a, b = path[s], path[s + 1]
    dq = (b - a).astype(dt)
    if v is None:
        v = chains(pb, a, b)[4]
    guard = dt(np.float32(guard))
    upper = min(dt(per_probe(pb, q).min()) for q in (([a] if s == 0 else []) + [b]))
    want, out = set(leaves), []
    l, k = 0, 0
    for _ in range(4 * len(want) + 4):
        q, _, hw = midpoint(a, dq, l, k, dt)
        d = per_probe(pb, q)
        u = dt(d.min())
        lo = dt(dt((d - (hw * v).astype(dt)).astype(dt).min()) - guard)
        upper = min(upper, u)
        leaf = (l, k) in want
        out.append(dict(l=l, k=k, u=u, lo=lo, leaf=leaf, upper=upper, reach=float((hw * v).max()), L=float(np.abs(pb.centres(q)).max())))
        if leaf:
            l, k, done = successor(l, k)
            if done:
                return out
        else:
            l, k = l + 1, 2 * k
    raise AssertionError("the leaves do not tile [0, 1]")


def tiles(leaves):
    """integer arithmetic on (l, k): the leaves, in order, tile [0, 1] exactly"""
    L = max((l for l, _ in leaves), default=0)
    at = 0
    for l, k in leaves:
        if k << (L - l) != at:
            return False
        at += 1 << (L - l)
    return at == 1 << L


# ---- the brute force, batched over configurations (float64)
def _qmul(a, b):
    return np.stack([a[..., 0] * b[..., 0] - a[..., 1] * b[..., 1] - a[..., 2] * b[..., 2] - a[..., 3] * b[..., 3],
                     a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0] + a[..., 2] * b[..., 3] - a[..., 3] * b[..., 2],
                     a[..., 0] * b[..., 2] - a[..., 1] * b[..., 3] + a[..., 2] * b[..., 0] + a[..., 3] * b[..., 1],
                     a[..., 0] * b[..., 3] + a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1] + a[..., 3] * b[..., 0]], -1)


def _qrot(q, v):
    t = 2.0 * np.cross(q[..., 1:], v)
    return v + q[..., :1] * t + np.cross(q[..., 1:], t)


def centres_batch(pb, Q):
    """probe centres (T, N, 3) in the world at the planned dofs Q (T, D), float64, at the row last given to pb.set_row()"""
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
            Qx = _qmul(Qx, np.concatenate([np.cos(h)[:, None], axis[b][None] * np.sin(h)[:, None]], 1))
        elif jt == kin_ref.PRISMATIC:
            P = P + _qrot(Qx, q[:, qa, None] * axis[b][None])
        par = m.parent[b]
        if par > 0:
            P, Qx = xp[:, par] + _qrot(xq[:, par], P), _qmul(xq[:, par], Qx)
        xp[:, b], xq[:, b] = P, Qx
    pr = np.asarray(pb.probes, np.float64)
    return xp[:, pb.links] + _qrot(xq[:, pb.links], pr[None, :, :3])


def clearance_batch(pb, Q):
    """the clearance (T,) of the configurations Q (T, D), float64"""
    pw = centres_batch(pb, Q)
    T, N = pw.shape[:2]
    d = np.full((T, N), float(pb.max_distance))
    flat = pw.reshape(-1, 3)
    for geom, c, Rg in pb.frames:
        g = dist_ref.geom_distance(geom, (flat - np.asarray(c, np.float64)) @ np.asarray(Rg, np.float64), np.float64)[0]
        d = np.minimum(d, g.reshape(T, N) - np.asarray(pb.probes[:, 3], np.float64)[None])
    return d.min(1)


def dense_min(pb, qrow, path, n=2048):
    """the minimum of the clearance over t = i / n, i = 0 .. n, on every segment of the path (float64) -> (K-1,)"""
    pb.set_row(qrow)
    path = np.asarray(path, np.float64)
    t = np.arange(n + 1)[:, None] / n
    out = []
    for s in range(len(path) - 1):
        a, b = path[s], path[s + 1]
        Q = a[None] if np.array_equal(a, b) else a[None] + t * (b - a)[None]
        out.append(float(clearance_batch(pb, Q).min()))
    return np.array(out)
