"""Reference for mir_plan_path / mir_path_clearance (include/mirigid.h): the planner of the header restated in NumPy, parametrised by
dtype.  A helper, no test.  `dtype=np.float64` is the reference; `dtype=np.float32` is the float32 port (every intermediate rounded to
float32) that the GPU tests take their yardstick from.  The random numbers are integers turned into float32 values that both dtypes hold
exactly, so both draw identical samples.

    clear(q):   forward kinematics from the spec (the local transform of a joint as the header of mir_signed_distance states it, parent
                before child), then dist_ref.geom_distance for every geom that is tested: min over probes of (d - radius), capped.
    edge(a, b): n_sub = max(1, ceil(max_j |b_j - a_j| / resolution)) <= 4096; a + (i / n_sub)(b - a), i = 1 .. n_sub, the last one b itself.
    plan():     RRT-Connect, extraction, shortcut smoothing, resampling -- step by step the text of the header.

It shares no code with the HIP kernel.  Geoms that are tested do not move with the planned dofs (the library refuses such a query), so
their world frames are computed once per start row.
"""
from __future__ import annotations

import numpy as np

import dist_ref
import kin_ref

OK, GOAL_OUT_OF_LIMITS, START_IN_COLLISION, GOAL_IN_COLLISION, NODE_LIMIT, ITERATION_LIMIT, PATH_TOO_LONG = range(7)
MAX_POLY, MAX_SUB = 128, 4096
M32 = 0xFFFFFFFF


def mix(x: int) -> int:
    """the 32-bit finaliser of MurmurHash3"""
    x &= M32
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    x ^= x >> 16
    return x


def u(seed: int, env: int, c: int, j: int) -> np.float32:
    """(x >> 8) 2^-24 with x = mix(mix(mix(seed ^ env) ^ c) ^ j): a float32 in [0, 1), exact"""
    x = mix(mix(mix((seed ^ env) & M32) ^ (c & M32)) ^ (j & M32))
    return np.float32((x >> 8) * 2.0 ** -24)


def _qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]], dtype=a.dtype)


def _qrot(q, v):
    t = (q.dtype.type(2) * np.cross(q[1:], v)).astype(q.dtype)
    return (v + q[0] * t + np.cross(q[1:], t)).astype(q.dtype)


class Problem:
    """one scene, one sphere model, one set of planned dofs: clear(q) at the start row last given to set_row()"""

    def __init__(self, spec, probes, links, dof_qadr, skip_geoms=0, max_distance=1.0, dtype=np.float64):
        self.dtype = dt = np.dtype(dtype).type
        self.model = m = kin_ref.Model(spec)
        self.nbody = spec.nbody
        self.bpos = np.array([list(spec.body[b].pos) for b in range(spec.nbody)]).astype(dt)
        self.bquat = np.array([list(spec.body[b].quat) for b in range(spec.nbody)]).astype(dt)
        self.axis = m.axis.astype(dt)
        self.qadr = [int(a) for a in dof_qadr]
        self.D = len(self.qadr)
        lim = m.limits(spec)
        self.lo, self.hi = np.zeros(self.D, dt), np.zeros(self.D, dt)
        planned = set()
        for j, qa in enumerate(self.qadr):
            b = next(b for b in range(1, m.nbody) if m.qadr[b] == qa and m.jtype[b] in (kin_ref.REVOLUTE, kin_ref.PRISMATIC))
            planned.add(b)
            self.lo[j], self.hi[j] = (dt(np.float32(v)) for v in lim[m.dofadr[b]])   # (the compiled model holds float32 limits)
        self.moves = [False] * m.nbody
        for b in range(1, m.nbody):
            chained = m.parent[b] > 0 and m.jtype[b] != kin_ref.FREE
            self.moves[b] = b in planned or (chained and self.moves[m.parent[b]])
        self.scene = dist_ref.Scene(spec)
        self.tested = [g for g in range(spec.ngeom) if not (int(skip_geoms) >> g) & 1]
        assert not any(self.moves[self.scene.geoms[g]["body"]] for g in self.tested), "a tested geom rides on a planned joint"
        self.probes = np.asarray(probes).astype(dt)
        self.links = np.zeros(len(self.probes), int) if links is None else np.asarray(links, int)
        self.groups = [(b, np.flatnonzero(self.links == b)) for b in sorted(set(self.links.tolist()))]
        self.max_distance = dt(max_distance)
        self.checked = 0

    def _local(self, b, q):
        dt, m = self.dtype, self.model
        jt, qa = m.jtype[b], m.qadr[b]
        if jt == kin_ref.FREE:
            Q = q[qa + 3:qa + 7]
            return q[qa:qa + 3].copy(), (Q / np.sqrt((Q * Q).sum(dtype=dt))).astype(dt)
        P, Q = self.bpos[b], self.bquat[b]
        if jt == kin_ref.REVOLUTE:
            h = dt(0.5) * q[qa]
            Q = _qmul(Q, np.concatenate([[np.cos(h)], self.axis[b] * np.sin(h)]).astype(dt))
        elif jt == kin_ref.PRISMATIC:
            P = (P + _qrot(Q, (q[qa] * self.axis[b]).astype(dt))).astype(dt)
        return P, Q

    def _fk(self, q, only_moving):
        m = self.model
        for b in range(1, m.nbody):
            if only_moving and not self.moves[b]:
                continue
            P, Q = self._local(b, q)
            par = m.parent[b]
            if par > 0 and m.jtype[b] != kin_ref.FREE:
                P, Q = (self.xp[par] + _qrot(self.xq[par], P)).astype(self.dtype), _qmul(self.xq[par], Q)
            self.xp[b], self.xq[b] = P, Q

    def set_row(self, qrow):
        """the full start configuration (nq,): every body's pose, the world frames of the tested geoms -> the planned dofs of the row"""
        dt = self.dtype
        self.q = np.asarray(qrow).astype(dt).copy()
        self.xp, self.xq = np.zeros((self.nbody, 3), dt), np.zeros((self.nbody, 4), dt)
        self.xq[:, 0] = 1
        self._fk(self.q, False)
        self.frames, self.seen = [], {}
        for g in self.tested:
            geom = self.scene.geoms[g]
            b = geom["body"]
            c = (self.xp[b] + _qrot(self.xq[b], geom["pos"].astype(dt))).astype(dt)
            Rg = dist_ref.qmat(_qmul(self.xq[b], geom["quat"].astype(dt)), dt)
            self.frames.append((geom, c, Rg))
        return self.q[self.qadr].copy()

    def centres(self, qp):
        """probe centres in the world at the planned dofs qp"""
        dt = self.dtype
        self.q[self.qadr] = np.asarray(qp).astype(dt)
        self._fk(self.q, True)
        pw = np.zeros((len(self.probes), 3), dt)
        for b, ix in self.groups:
            pw[ix] = self.probes[ix, :3] if b == 0 else (self.xp[b] + self.probes[ix, :3] @ dist_ref.qmat(self.xq[b], dt).T).astype(dt)
        return pw

    def clearance(self, qp):
        dt = self.dtype
        self.checked += 1
        key = np.asarray(qp).astype(dt).tobytes()   # (smoothing asks for the same configurations again and again: evaluated once)
        if key in self.seen:
            return self.seen[key]
        pw = self.centres(qp)
        if not (np.isfinite(pw).all() and np.isfinite(np.asarray(qp, np.float64)).all()):   # (not a configuration: blocked)
            return dt(-np.inf)
        best = self.max_distance
        for geom, c, Rg in self.frames:
            d = dist_ref.geom_distance(geom, ((pw - c) @ Rg).astype(dt), dt)[0]
            best = min(best, dt((d - self.probes[:, 3]).min()))
        self.seen[key] = dt(best)
        return dt(best)


def n_sub(a, b, resolution, dtype):
    dt = np.dtype(dtype).type
    m = np.abs((b - a).astype(dt)).max()
    with np.errstate(invalid="ignore"):
        r = np.ceil(dt(m / dt(resolution)))
    return int(min(max(r, 1), MAX_SUB)) if np.isfinite(r) else (MAX_SUB if r > 0 else 1)


def edge_samples(a, b, resolution, dtype):
    """the configurations edge(a, b) checks, in order; the last one is b itself"""
    dt = np.dtype(dtype).type
    n = n_sub(a, b, resolution, dtype)
    diff = (b - a).astype(dt)
    return [b if i == n else (a + dt(dt(i) / dt(n)) * diff).astype(dt) for i in range(1, n + 1)]


def resample(poly, W, dtype):
    """W configurations at equal steps of the cumulative L2 length of the polyline; the ends are the polyline's own bits; a polyline of
    one segment is interpolated at t = w / (W - 1) itself"""
    dt = np.dtype(dtype).type
    poly = np.asarray(poly).astype(dt)
    n = len(poly)
    if n == 1:
        return np.repeat(poly, W, axis=0)
    cum = [dt(0)]
    for k in range(n - 1):
        e = (poly[k + 1] - poly[k]).astype(dt)
        acc = dt(0)
        for x in e:
            acc = dt(acc + x * x)
        cum.append(dt(cum[-1] + np.sqrt(acc)))
    total, out, k = cum[-1], [], 0
    for w in range(W):
        if w == 0:
            out.append(poly[0])
        elif w == W - 1:
            out.append(poly[-1])
        else:
            f = dt(dt(w) / dt(W - 1))
            t = f
            if n > 2:
                s = dt(f * total)
                while k < n - 2 and cum[k + 1] <= s:
                    k += 1
                ln = dt(cum[k + 1] - cum[k])
                t = min(dt((s - cum[k]) / ln), dt(1)) if ln > 0 else dt(0)
            out.append((poly[k] + t * (poly[k + 1] - poly[k])).astype(dt))
    return np.stack(out)


def plan(pb: Problem, qrow, goal, env, W=16, max_nodes=128, max_iterations=512, smooth_passes=64, seed=0, resolution=0.05, step=0.3,
         margin=0.0, ignore_collision=False):
    """one row -> dict(status, poly (n_poly, D), path (W, D), iterations, nodes (na, nb), checked)"""
    dt = pb.dtype
    start = pb.set_row(qrow)
    goal = np.asarray(goal).astype(dt)
    pb.checked = 0
    margin, step = dt(margin), dt(step)
    clear = (lambda q: True) if ignore_collision else (lambda q: pb.clearance(q) >= margin)

    def edge(a, b):
        return all(clear(q) for q in edge_samples(a, b, resolution, dt))   # (all() stops at the first blocked sample)

    def done(status, poly, it=0, na=1, nb=1):
        if status != OK:
            poly = [start]
        poly = np.stack(poly)
        return dict(status=status, poly=poly, path=resample(poly, W, dt), iterations=it, nodes=(na, nb), checked=pb.checked)

    if ((goal < pb.lo) | (goal > pb.hi)).any() or not np.isfinite(goal).all():
        return done(GOAL_OUT_OF_LIMITS, None)
    if not clear(start):
        return done(START_IN_COLLISION, None)
    if not clear(goal):
        return done(GOAL_IN_COLLISION, None)
    if edge(start, goal):
        return done(OK, [start, goal])
    nodes, parent = [[start], [goal]], [[-1], [-1]]

    def nearest(t, q):
        arr = np.stack(nodes[t])
        acc = np.zeros(len(arr), dt)
        for j in range(pb.D):
            e = (arr[:, j] - q[j]).astype(dt)
            acc = (acc + e * e).astype(dt)
        i = int(acc.argmin())   # (the first of equal minima: the lower index)
        return i, acc[i]

    poly, status, it_done = None, ITERATION_LIMIT, 0
    for it in range(max_iterations):
        it_done = it + 1
        t, o = it & 1, (it & 1) ^ 1
        qr = np.array([pb.lo[j] + dt(u(seed, env, it, j)) * (pb.hi[j] - pb.lo[j]) for j in range(pb.D)], dt)
        near, d2 = nearest(t, qr)
        nv = nodes[t][near]
        with np.errstate(divide="ignore"):
            sc = min(dt(1), dt(step / np.sqrt(d2)))
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
            acc = dt(0)
            for x in diff:
                acc = dt(acc + x * x)
            d = np.sqrt(acc)
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
        tail, n = [], parent[1][ib]   # (the meeting node is in both trees: once)
        while n >= 0:
            tail.append(nodes[1][n])
            n = parent[1][n]
        poly = head[::-1] + tail
        status = PATH_TOO_LONG if len(poly) > MAX_POLY else OK
        break
    na, nb = len(nodes[0]), len(nodes[1])
    if status != OK:
        return done(status, None, it_done, na, nb)
    for s in range(smooth_passes):
        n = len(poly)
        if n < 3:
            break
        c = 0x80000000 | s
        i = min(int(np.float32(u(seed, env, c, 0) * np.float32(n - 2))), n - 3)
        j = i + 2 + min(int(np.float32(u(seed, env, c, 1) * np.float32(n - 2 - i))), n - 3 - i)
        if edge(poly[i], poly[j]):
            poly = poly[:i + 1] + poly[j:]
    return done(OK, poly, it_done, na, nb)


def polyline_clearance(pb: Problem, qrow, poly, resolution):
    """the swept check: seg_min (K-1,) over the samples of the edge rule on each segment (the first point counts for segment 0 only) and
    the samples themselves"""
    dt = pb.dtype
    pb.set_row(qrow)
    poly = np.asarray(poly).astype(dt)
    seg, samples = [], []
    for k in range(len(poly) - 1):
        qs = ([poly[0]] if k == 0 else []) + edge_samples(poly[k], poly[k + 1], resolution, dt)
        seg.append(min(pb.clearance(q) for q in qs))
        samples.extend(qs)
    return np.array(seg, dt), samples


def path_clearance(pb: Problem, qrow, path, resolution, margin):
    """mir_path_clearance of one row -> seg_min (K-1,), row_min, row_first_blocked"""
    seg, _ = polyline_clearance(pb, qrow, path, resolution)
    blocked = np.flatnonzero(seg < pb.dtype(margin))
    return seg, seg.min(), int(blocked[0]) if len(blocked) else -1


def polyline_length(poly):
    p = np.asarray(poly, np.float64)
    return float(np.sqrt(((p[1:] - p[:-1]) ** 2).sum(1)).sum())
