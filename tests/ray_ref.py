"""Reference for mir_raycast (include/mirigid.h): the range along rays of a sensor on a link, restated in NumPy from the definitions
of the header.  A helper, no test.  It shares no code with the HIP kernel; the hull faces come from its own brute force over vertex
triples.

    sensor origin o = o_link + R_link pos_offset, axes R_s = R_link R(quat_offset); ray i = o + t R_s d_i / |d_i|, t >= 0
    plane: two-sided, unbounded;  box, sphere, capsule: exact;  hull: the convex polytope of its vertices
    a solid that contains the origin is not seen;  the nearest entry wins, ties go to the lower geom index
    distance = clamp(t_hit, min_range, max_range) (max_range on a miss: nothing hit, or a hit beyond max_range)
    points = distance x unit direction (sensor frame), or origin + that in world axes;  normal: unit outward, 0 on a miss

Inputs are world link poses xpos (E, nbody, 3) / xquat (E, nbody, 4 wxyz) (the oracle's after `Oracle.fk`).  `dtype=np.float64` is the
reference; `dtype=np.float32` on the poses of `Oracle(f32=...)` is the float32 port the GPU tests use as their yardstick: the same
formulas with every intermediate rounded to float32.

`ambiguous` (E, N): the hit geom (or the hit-or-miss decision) changes when the direction is tilted by 1e-4 rad towards any of four
perpendicular directions, or the two nearest entries (of different geoms) lie within 1e-5 m.  A zero direction is never ambiguous.
"""
from __future__ import annotations

import itertools

import numpy as np

PLANE, BOX, SPHERE, CAPSULE, HULL = 0, 1, 2, 3, 4
TILT, NEAR = 1e-4, 1e-5


def qmat(q, dtype=np.float64):
    q = np.asarray(q).astype(dtype)
    q = q / np.sqrt((q * q).sum(dtype=dtype))
    w, x, y, z = q
    one, two = dtype(1), dtype(2)
    return np.array([[one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)],
                     [two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)],
                     [two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)]], dtype=dtype)


def qmul(a, b, dtype=np.float64):
    a, b = np.asarray(a).astype(dtype), np.asarray(b).astype(dtype)
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]], dtype=dtype)


def hull_planes(verts):
    """unit outward normals (P, 3) and offsets (P,) of the faces of the convex hull of `verts` (float64): every vertex triple whose plane
    has all vertices on one side; triples of one face give one plane.  Raises ValueError for a hull without volume."""
    v = np.asarray(verts, dtype=np.float64)
    scale = np.abs(v).max()
    tol = 1e-9 * scale
    ns, ds = [], []
    for i, j, k in itertools.combinations(range(len(v)), 3):
        n = np.cross(v[j] - v[i], v[k] - v[i])
        ln = np.linalg.norm(n)
        if ln <= 1e-12 * scale * scale:
            continue
        n = n / ln
        s = v @ n - n @ v[i]
        if s.max() > tol and s.min() < -tol:
            continue
        if s.max() <= tol and s.min() >= -tol:
            continue  # all vertices in this plane
        if s.max() > tol:
            n = -n
        d = float(n @ v[i])
        if any(n @ m > 1.0 - 1e-12 and abs(d - e) <= 10 * tol for m, e in zip(ns, ds)):
            continue
        ns.append(n)
        ds.append(d)
    if len(ns) < 4:
        raise ValueError("hull without volume")
    return np.array(ns), np.array(ds)


class Scene:
    """the geoms of a MirSceneSpec as the reference needs them (spec values in float64; hull planes computed once)"""

    def __init__(self, spec):
        self.ngeom, self.nbody = spec.ngeom, spec.nbody
        self.geoms = []
        for g in range(spec.ngeom):
            gs = spec.geom[g]
            size = np.array(list(gs.size), float)
            planes = None
            if gs.type == HULL:
                v0, nv = int(size[0]), int(size[1])
                planes = hull_planes([[spec.vert[i][k] for k in range(3)] for i in range(v0, v0 + nv)])
            self.geoms.append(dict(body=gs.body, type=gs.type, size=size, pos=np.array(list(gs.pos), float), quat=np.array(list(gs.quat), float), planes=planes))


def _sphere_t(oc, d, r2):
    """entry range (inf = miss) of unit rays d (N, 3) from oc (3,), outside the sphere of squared radius r2 about the origin"""
    b = d @ oc
    cr = np.cross(np.broadcast_to(oc, d.shape), d)
    disc = r2 - (cr * cr).sum(-1)
    t = -b - np.sqrt(np.maximum(disc, 0))
    return np.where((disc >= 0) & (b < 0), t, np.inf).astype(d.dtype)


def _entry(g, o, d, dtype):
    """(t (N,) entry range or inf, n (N, 3) unit outward normal in the geom frame) of unit rays d from o (geom frame), or None when the
    solid contains o"""
    N = d.shape[0]
    typ, s = g["type"], g["size"].astype(dtype)
    inf = dtype(np.inf)
    n = np.zeros((N, 3), dtype)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if typ == PLANE:
            t = -o[2] / d[:, 2]
            t = np.where((d[:, 2] != 0) & (t > 0), t, inf)
            n[:, 2] = 1 if o[2] >= 0 else -1
            return t.astype(dtype), n
        if typ == BOX:
            if (np.abs(o) <= s).all():
                return None
            tn, tf, kn = np.full(N, -inf, dtype), np.full(N, inf, dtype), np.zeros(N, int)
            for k in range(3):
                t1, t2 = (-s[k] - o[k]) / d[:, k], (s[k] - o[k]) / d[:, k]
                lo, hi = np.minimum(t1, t2), np.maximum(t1, t2)
                par, out = d[:, k] == 0, abs(o[k]) > s[k]
                lo = np.where(par, inf if out else -inf, lo)
                hi = np.where(par, -inf if out else inf, hi)
                upd = lo > tn
                tn, kn = np.where(upd, lo, tn), np.where(upd, k, kn)
                tf = np.minimum(tf, hi)
            n[np.arange(N), kn] = np.where(d[np.arange(N), kn] > 0, -1, 1)
            return np.where((tn <= tf) & (tn > 0), tn, inf).astype(dtype), n
        if typ == HULL:
            pn, pd = g["planes"][0].astype(dtype), g["planes"][1].astype(dtype)
            dist = pn @ o - pd
            if (dist <= 0).all():
                return None
            den = d @ pn.T
            tp = -dist[None, :] / den
            enter = np.where(den < 0, tp, -inf)
            enter = np.where((den == 0) & (dist[None, :] > 0), inf, enter)
            leave = np.where(den > 0, tp, inf)
            tn, arg, tf = enter.max(1), enter.argmax(1), leave.min(1)
            return np.where((tn <= tf) & (tn > 0), tn, inf).astype(dtype), pn[arg]
        r, hl = s[0], (s[1] if typ == CAPSULE else dtype(0))
        zc = np.clip(o[2], -hl, hl)
        if o[0] * o[0] + o[1] * o[1] + (o[2] - zc) * (o[2] - zc) <= r * r:
            return None
        ez = np.array([0, 0, 1], dtype)
        t = _sphere_t(o - hl * ez, d, r * r)
        if hl > 0:
            t = np.minimum(t, _sphere_t(o + hl * ez, d, r * r))
            c2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
            if o[0] * o[0] + o[1] * o[1] - r * r > 0:
                b = o[0] * d[:, 0] + o[1] * d[:, 1]
                cz = o[0] * d[:, 1] - o[1] * d[:, 0]
                disc = r * r * c2 - cz * cz
                tl = (-b - np.sqrt(np.maximum(disc, 0))) / c2
                ok = (disc >= 0) & (b < 0) & (c2 > 0) & (np.abs(o[2] + tl * d[:, 2]) <= hl)
                t = np.where(ok & (tl < t), tl, t)
        p = o[None, :] + np.where(np.isfinite(t), t, 0)[:, None] * d
        n = p.copy()
        n[:, 2] -= np.clip(p[:, 2], -hl, hl)
        return t.astype(dtype), (n / r).astype(dtype)


def _nearest(scene, frames, origin, dw, max_range, skip, dtype):
    """nearest entry per unit world ray dw (N, 3): t (inf = miss), geom, world normal, second-nearest entry of another geom"""
    N = dw.shape[0]
    t1, t2 = np.full(N, np.inf, dtype), np.full(N, np.inf, dtype)
    geom, nrm = np.full(N, -1, np.int64), np.zeros((N, 3), dtype)
    for g, (c, R) in enumerate(frames):
        if (skip >> g) & 1:
            continue
        o = R.T @ (origin - c)
        e = _entry(scene.geoms[g], o.astype(dtype), (dw @ R).astype(dtype), dtype)
        if e is None:
            continue
        t, n = e
        win = t < t1
        t2 = np.where(win, t1, np.minimum(t2, t))
        nrm = np.where(win[:, None], n @ R.T, nrm)
        geom = np.where(win, g, geom)
        t1 = np.where(win, t, t1)
    miss = ~(t1 <= max_range)
    return np.where(miss, np.inf, t1), np.where(miss, -1, geom), np.where(miss[:, None], 0, nrm).astype(dtype), t1, t2


def raycast_env(scene, xpos, xquat, link, pos_offset, quat_offset, dirs, min_range, max_range, skip_geoms=0, world_frame=False,
                dtype=np.float64, with_ambiguous=True):
    """one env: xpos (nbody, 3), xquat (nbody, 4) -> dict of t, distance, geom, points, normal, ambiguous"""
    xpos, xquat = np.asarray(xpos).astype(dtype), np.asarray(xquat).astype(dtype)
    dirs = np.asarray(dirs).astype(dtype)
    max_range, min_range = dtype(max_range), dtype(min_range)
    if link > 0:
        ol, ql = xpos[link], xquat[link]
    else:
        ol, ql = np.zeros(3, dtype), np.array([1, 0, 0, 0], dtype)
    origin = ol + qmat(ql, dtype) @ np.asarray(pos_offset).astype(dtype)
    Rs = qmat(qmul(ql / np.sqrt((ql * ql).sum(dtype=dtype)), np.asarray(quat_offset, float) / np.linalg.norm(np.asarray(quat_offset, float)), dtype), dtype)
    ln = np.sqrt((dirs * dirs).sum(-1))
    zero = ~(ln > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        ds = np.where(zero[:, None], 0, dirs / ln[:, None]).astype(dtype)
    dw = (ds @ Rs.T).astype(dtype)
    frames = []
    for g in scene.geoms:
        b = g["body"]
        c = xpos[b] + qmat(xquat[b], dtype) @ g["pos"].astype(dtype)
        frames.append((c, qmat(qmul(xquat[b] / np.sqrt((xquat[b] * xquat[b]).sum(dtype=dtype)), g["quat"], dtype), dtype)))
    t, geom, nw, t1, t2 = _nearest(scene, frames, origin, dw, max_range, int(skip_geoms), dtype)
    t, geom, nw = np.where(zero, np.inf, t), np.where(zero, -1, geom), np.where(zero[:, None], 0, nw)
    dist = np.clip(np.where(np.isfinite(t), t, max_range), min_range, max_range).astype(dtype)
    pts = dist[:, None] * ds
    out = {"t": t, "distance": dist, "geom": geom, "origin": origin, "Rs": Rs,
           "points": (origin + pts @ Rs.T if world_frame else pts).astype(dtype), "normal": (nw if world_frame else nw @ Rs).astype(dtype)}
    if with_ambiguous:
        with np.errstate(invalid="ignore"):
            amb = (t2 - t1) < NEAR
        p1 = np.cross(dw, np.where(np.abs(dw[:, :1]) < 0.9, np.array([[1.0, 0, 0]]), np.array([[0, 1.0, 0]])))
        p1 = p1 / np.maximum(np.linalg.norm(p1, axis=1, keepdims=True), 1e-300)
        p2 = np.cross(dw, p1)
        for p in (p1, -p1, p2, -p2):
            dt = dw + np.tan(TILT) * p
            dt = (dt / np.maximum(np.linalg.norm(dt, axis=1, keepdims=True), 1e-300)).astype(dtype)
            amb |= _nearest(scene, frames, origin, dt, max_range, int(skip_geoms), dtype)[1] != geom
        out["ambiguous"] = amb & ~zero
    return out


def raycast(scene, xpos, xquat, link, pos_offset, quat_offset, dirs, min_range, max_range, skip_geoms=0, world_frame=False,
            dtype=np.float64, with_ambiguous=True) -> dict:
    """the batched result in the shapes of MirScene.raycast: xpos (E, nbody, 3), xquat (E, nbody, 4) -> (E, N[, 3]) arrays"""
    rows = [raycast_env(scene, xpos[e], xquat[e], link, pos_offset, quat_offset, dirs, min_range, max_range, skip_geoms, world_frame, dtype,
                        with_ambiguous) for e in range(len(xpos))]
    return {k: np.stack([r[k] for r in rows]) for k in rows[0]}


def oracle_poses(o, envs=None):
    """xpos (E, nbody, 3), xquat (E, nbody, 4) of the oracle's current state (`Oracle.fk` per env)"""
    import orc

    envs = range(o.B) if envs is None else envs
    xp, xq = [], []
    for e in envs:
        o.fk(e)
        xp.append(o.read(orc.F_XPOS, e).reshape(-1, 3).copy())
        xq.append(o.read(orc.F_XQUAT, e).reshape(-1, 4).copy())
    return np.stack(xp), np.stack(xq)
