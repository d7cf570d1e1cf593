"""Reference for mir_signed_distance (include/mirigid.h): the signed distance from probe spheres to the nearest geom, restated in NumPy
from the definitions of the header.  A helper, no test.  It shares no code with the HIP kernel: the hull's outside distance is the
minimum over ALL vertex triples whose plane has every other vertex on one side (the brute force of ray_ref.hull_planes), each by
projection on the triangle's plane and, outside it, the nearest of its three edges -- not the kernel's fan table and region walk.

    per geom, probe centre p in the geom's frame:  d < 0 inside, `closest` the nearest surface point, `normal` the unit outward gradient
    plane: d = p.z (the solid is z <= 0);  sphere: |p| - r;  capsule: |p - c| - r;  box: |p - clamp(p)| outside, max_i(|p_i| - h_i) inside
    hull: max_f(n_f . p - d_f) inside, the nearest triangle outside
    s_g = d_g - radius; the lowest wins, ties go to the lower geom index; s > max_distance is a miss

Inputs are world link poses xpos (E, nbody, 3) / xquat (E, nbody, 4 wxyz) (the oracle's after `Oracle.fk`), so it serves the pose cache
and candidate configurations alike.  `dtype=np.float64` is the reference; `dtype=np.float32` on the poses of `Oracle(f32=...)` is the float32
port the GPU tests use as their yardstick: the same formulas with every intermediate rounded to float32.

`ambiguous` (E, N): the runner-up geom's s is within NEAR = 1e-4 m of the winner's; or the winner's s is within NEAR of max_distance; or
the winner's own answer is ill-conditioned -- the probe within NEAR of a sphere's centre or a capsule's axis; two interior face distances
of a box or hull within NEAR; |d| < SURF = 1e-5 of a box or hull, from either side; outside a hull, two triangles of different faces
within NEAR_TRI = 1e-5 m as nearest while their nearest points differ by more than SAME = 1e-6 m.
Two notes on the last rule.  Faces that meet in the nearest edge or vertex return the same point: there is nothing to choose, and without
SAME every probe in an edge or vertex region would be flagged.  And the rule is held at 1e-5, not at NEAR: the two distances differ by
delta^2 / 2d for a probe delta from the boundary between a face's region and its edge's, so the flagged band is sqrt(2 d x threshold)
wide -- at 1e-4, a tenth of all probes next to the 60-face ball and 3 % of the zoo case, more than the 2 % tests/test_dist_cpu.py allows.
A float32 minimum over triangles can take the wrong one of two only when they are within its rounding, 4e-7 d <= 2e-7 m here; 1e-5 is 50
times that.  The narrower rule excuses fewer probes, so the GPU test asks more than it would at 1e-4, not less.
"""
from __future__ import annotations

import itertools

import numpy as np

import ray_ref
from ray_ref import BOX, CAPSULE, HULL, PLANE, SPHERE, qmat, qmul  # noqa: F401

NEAR, SURF, SAME, NEAR_TRI = 1e-4, 1e-5, 1e-6, 1e-5


def hull_triangles(verts, planes):
    """every vertex triple that lies in a face plane: (T, 3, 3) vertices and (T,) the face of each"""
    v = np.asarray(verts, dtype=np.float64)
    pn, pd = planes
    tol = 1e-9 * np.abs(v).max()
    tris, face = [], []
    for f in range(len(pd)):
        on = [i for i in range(len(v)) if abs(pn[f] @ v[i] - pd[f]) <= 10 * tol]
        for i, j, k in itertools.combinations(on, 3):
            if np.linalg.norm(np.cross(v[j] - v[i], v[k] - v[i])) > 1e-12:
                tris.append(v[[i, j, k]])
                face.append(f)
    return np.array(tris), np.array(face)


class Scene:
    """the geoms of a MirSceneSpec as the reference needs them (spec values in float64; hull planes and triangles computed once)"""

    def __init__(self, spec):
        self.ngeom, self.nbody = spec.ngeom, spec.nbody
        self.geoms = []
        for g in range(spec.ngeom):
            gs = spec.geom[g]
            size = np.array(list(gs.size), float)
            d = dict(body=gs.body, type=gs.type, size=size, pos=np.array(list(gs.pos), float), quat=np.array(list(gs.quat), float))
            if gs.type == HULL:
                v0, nv = int(size[0]), int(size[1])
                d["verts"] = np.array([[spec.vert[i][k] for k in range(3)] for i in range(v0, v0 + nv)])
                d["planes"] = ray_ref.hull_planes(d["verts"])
                d["tris"], d["tri_face"] = hull_triangles(d["verts"], d["planes"])
            self.geoms.append(d)


def sphere_scene(probes):
    """a scene whose geoms are spheres in the world: probes (N, 4) centre and radius (the containment check of collision_spheres)"""
    sc = Scene.__new__(Scene)
    sc.ngeom, sc.nbody = len(probes), 1
    sc.geoms = [dict(body=0, type=SPHERE, size=np.array([p[3], 0.0, 0.0]), pos=np.array(p[:3], float), quat=np.array([1.0, 0, 0, 0])) for p in probes]
    return sc


def _unit(v, dtype):
    ln = np.sqrt((v * v).sum(-1))
    with np.errstate(divide="ignore", invalid="ignore"):
        return ln, np.where((ln > 0)[:, None], v / ln[:, None], np.array([0, 0, 1], dtype))


def _segment(p, a, b):
    ab = b - a
    t = np.clip(((p - a) @ ab) / (ab @ ab), 0, 1)
    return a + t[:, None] * ab


def _triangle(p, tri, dtype):
    """nearest point of the triangle to every p (N, 3): the foot on its plane when that lies inside, else the nearest point of an edge"""
    a, b, c = tri[0], tri[1], tri[2]
    n = np.cross(b - a, c - a)
    n = n / np.sqrt(n @ n)
    foot = p - ((p - a) @ n)[:, None] * n
    inside = np.ones(len(p), bool)
    for u, w in ((a, b), (b, c), (c, a)):
        inside &= np.cross(w - u, foot - u) @ n >= 0
    best, bd = foot, np.where(inside, ((p - foot) ** 2).sum(-1), np.inf)
    for u, w in ((a, b), (b, c), (c, a)):
        q = _segment(p, u, w)
        d2 = ((p - q) ** 2).sum(-1)
        take = ~inside & (d2 < bd)
        best, bd = np.where(take[:, None], q, best), np.where(take, d2, bd)
    return best.astype(dtype), bd.astype(dtype)


def geom_distance(g, p, dtype=np.float64):
    """-> d (N,), closest (N, 3), normal (N, 3), ill (N,) for probe centres p (N, 3) in the geom's frame"""
    p = np.asarray(p).astype(dtype)
    N = len(p)
    typ, s = g["type"], g["size"].astype(dtype)
    ez = np.array([0, 0, 1], dtype)
    if typ == PLANE:
        cp = p.copy()
        cp[:, 2] = 0
        return p[:, 2].copy(), cp, np.broadcast_to(ez, (N, 3)).copy(), np.zeros(N, bool)
    if typ in (SPHERE, CAPSULE):
        r, hl = s[0], (s[1] if typ == CAPSULE else dtype(0))
        c = np.zeros((N, 3), dtype)
        c[:, 2] = np.clip(p[:, 2], -hl, hl)
        ln, n = _unit(p - c, dtype)
        return (ln - r).astype(dtype), (c + r * n).astype(dtype), n.astype(dtype), ln < NEAR
    if typ == BOX:
        q = np.abs(p) - s
        cl = np.clip(p, -s, s)
        ln, n_out = _unit(p - cl, dtype)
        im = q.argmax(1)   # (the first of equal maxima: the lower axis)
        qm = q[np.arange(N), im]
        sg = np.where(p[np.arange(N), im] >= 0, dtype(1), dtype(-1))
        n_in = np.zeros((N, 3), dtype)
        n_in[np.arange(N), im] = sg
        cp_in = p.copy()
        cp_in[np.arange(N), im] = sg * s[im]
        out = (qm > 0) & (ln > 0)
        qs = np.sort(q, axis=1)
        ill = np.where(out, ln < SURF, (qs[:, 2] - qs[:, 1] < NEAR) | (np.abs(qm) < SURF))
        return np.where(out, ln, qm).astype(dtype), np.where(out[:, None], cl, cp_in).astype(dtype), np.where(out[:, None], n_out, n_in).astype(dtype), ill
    pn, pd = g["planes"][0].astype(dtype), g["planes"][1].astype(dtype)
    sf = p @ pn.T - pd
    fm = sf.argmax(1)
    sm = sf[np.arange(N), fm]
    d, n, cp = sm.copy(), pn[fm].copy(), (p - sm[:, None] * pn[fm]).astype(dtype)
    ss = np.sort(sf, axis=1)
    ill = (ss[:, -1] - ss[:, -2] < NEAR) | (np.abs(sm) < SURF)
    o = np.flatnonzero(sm > 0)
    if len(o):
        po = p[o]
        nf = len(pd)
        fd, fc = np.full((len(o), nf), np.inf), np.zeros((len(o), nf, 3))
        for tri, f in zip(g["tris"].astype(dtype), g["tri_face"]):
            q, d2 = _triangle(po, tri, dtype)
            take = d2 < fd[:, f]
            fd[:, f] = np.where(take, d2, fd[:, f])
            fc[:, f] = np.where(take[:, None], q, fc[:, f])
        k = fd.argmin(1)
        dk = np.sqrt(fd[np.arange(len(o)), k]).astype(dtype)
        ck = fc[np.arange(len(o)), k].astype(dtype)
        _, nk = _unit(po - ck, dtype)
        near = (np.sqrt(fd) - dk[:, None].astype(np.float64) < NEAR_TRI) & (np.sqrt(((fc - ck[:, None, :]) ** 2).sum(-1)) > SAME)
        d[o], cp[o], ill[o] = dk, ck, near.any(1) | (dk < SURF)
        n[o] = np.where((dk > 0)[:, None], nk, n[o])
    return d.astype(dtype), cp, n.astype(dtype), ill


def signed_distance_env(scene, xpos, xquat, probes, links, max_distance, skip_geoms=0, dtype=np.float64, with_ambiguous=True):
    """one env: xpos (nbody, 3), xquat (nbody, 4) -> dict of distance, geom, closest, normal, centre, s (the winner's, inf: nothing
    tested), ambiguous, inside (the winning geom contains the probe's centre)"""
    xpos, xquat = np.asarray(xpos).astype(dtype), np.asarray(xquat).astype(dtype)
    probes = np.asarray(probes).astype(dtype)
    N = len(probes)
    links = np.zeros(N, int) if links is None else np.asarray(links, int)
    max_distance = dtype(max_distance)
    R = {b: qmat(xquat[b], dtype) for b in set(links.tolist()) if b > 0}
    pw = np.stack([probes[i, :3] if links[i] == 0 else xpos[links[i]] + R[links[i]] @ probes[i, :3] for i in range(N)]).astype(dtype)
    s1, s2 = np.full(N, np.inf, dtype), np.full(N, np.inf, dtype)
    geom, cl, nr = np.full(N, -1, np.int64), pw.copy(), np.zeros((N, 3), dtype)
    ill, inside = np.zeros(N, bool), np.zeros(N, bool)
    for gi, g in enumerate(scene.geoms):
        if (int(skip_geoms) >> gi) & 1:
            continue
        b = g["body"]
        c = xpos[b] + qmat(xquat[b], dtype) @ g["pos"].astype(dtype)
        Rg = qmat(qmul(xquat[b] / np.sqrt((xquat[b] * xquat[b]).sum(dtype=dtype)), g["quat"], dtype), dtype)
        d, cp, n, il = geom_distance(g, ((pw - c) @ Rg).astype(dtype), dtype)
        s = (d - probes[:, 3]).astype(dtype)
        win = s < s1
        s2 = np.where(win, s1, np.minimum(s2, s))
        cl = np.where(win[:, None], (c + cp @ Rg.T).astype(dtype), cl)
        nr = np.where(win[:, None], (n @ Rg.T).astype(dtype), nr)
        geom, ill, inside = np.where(win, gi, geom), np.where(win, il, ill), np.where(win, d < 0, inside)
        s1 = np.where(win, s, s1)
    hit = s1 <= max_distance
    out = {"distance": np.where(hit, s1, max_distance).astype(dtype), "geom": np.where(hit, geom, -1), "closest": np.where(hit[:, None], cl, pw).astype(dtype),
           "normal": np.where(hit[:, None], nr, 0).astype(dtype), "centre": pw, "s": s1, "inside": inside & hit}
    if with_ambiguous:
        with np.errstate(invalid="ignore"):
            out["ambiguous"] = (s2 - s1 < NEAR) | (np.abs(s1 - max_distance) < NEAR) | (ill & hit)
    return out


def signed_distance(scene, xpos, xquat, probes, links, max_distance, skip_geoms=0, dtype=np.float64, with_ambiguous=True) -> dict:
    """the batched result in the shapes of MirScene.signed_distance: xpos (E, nbody, 3), xquat (E, nbody, 4) -> (E, N[, 3]) arrays, and
    row_min (E,) / row_argmin (E,)"""
    rows = [signed_distance_env(scene, xpos[e], xquat[e], probes, links, max_distance, skip_geoms, dtype, with_ambiguous) for e in range(len(xpos))]
    out = {k: np.stack([r[k] for r in rows]) for k in rows[0]}
    out["row_argmin"] = out["distance"].argmin(1)   # (the first of equal minima: the lower index)
    out["row_min"] = out["distance"].min(1)
    return out
