"""Float64 NumPy ray caster of the rasteriser's image definition with exact spheres and capsules (MIR_VIS_ROUND_GEOMS).

A plain helper module of the render tests (not a conftest).  It restates DESIGN.md 9 from the definition, in world coordinates
and double precision, sharing no code with the HIP kernels or the C oracle:
  * pinhole camera (vertical fov, pixel-centre sampling, row 0 = top); ray d = F + x R + y U, so t along d is the planar depth;
  * the nearest surface per pixel (strict <, geoms in scene order, envs in order; a plane only from env 0, only where t > 1e-6);
  * planes: checker of `checker_size` cells in the geom's x / y, normal facing the camera; boxes: slab test;
  * spheres and capsules: the exact surface with round=True, their bounding boxes with round=False (what the oracle draws);
    a camera inside a solid sees nothing of it; hulls: the bounding box of their vertices (float32, as the kernel's model holds them);
  * RGB = albedo x (ambient + diffuse x max(0, n.l)), clamped to [0, 1], floor(c x 255 + 0.5).

cast(...) returns a dict of (H, W) arrays: t (sky -1), geom (sky -1), env (sky -1), normal (H, W, 3) unit world normal (sky 0),
rgb (H, W, 3) uint8, cell (the checker parity of a plane pixel, the face of a box pixel (2 .. 7), else 0).
"""
import numpy as np

PLANE, BOX, SPHERE, CAPSULE, HULL = 0, 1, 2, 3, 4


def quat_mat(q):
    w, x, y, z = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def camera_basis(pos, lookat, up):
    pos, lookat, up = (np.array(list(v), float) for v in (pos, lookat, up))
    f = lookat - pos
    f /= np.linalg.norm(f)
    r = np.cross(f, up)
    for fb in ((0.0, 1.0, 0.0), (1.0, 0.0, 0.0)):  # view parallel to up: +y, then +x
        if r @ r >= 1e-24:
            break
        r = np.cross(f, fb)
    r /= np.linalg.norm(r)
    return f, r, np.cross(r, f)


def rays(cam, pos=None, lookat=None):
    """(H, W, 3) rays d = F + x R + y U of a camera (pos / lookat override the spec's)"""
    f, r, u = camera_basis(cam.pos if pos is None else pos, cam.lookat if lookat is None else lookat, cam.up)
    W, H = cam.width, cam.height
    ty = np.tan(0.5 * np.radians(cam.fov_deg))
    tx = ty * W / H
    xs = (2.0 * (np.arange(W) + 0.5) / W - 1.0) * tx
    ys = (1.0 - 2.0 * (np.arange(H) + 0.5) / H) * ty
    return f[None, None] + xs[None, :, None] * r[None, None] + ys[:, None, None] * u[None, None], (f, r, u, tx, ty)


def prims(spec, xpos, xquat, offsets=None, round=True):
    """[(env, geom, type, centre, R, size)] of every drawn geom; xpos (nenv, nbody, 3), xquat (nenv, nbody, 4 wxyz)"""
    out = []
    xpos, xquat = np.asarray(xpos, float), np.asarray(xquat, float)
    for e in range(xpos.shape[0]):
        for g in range(spec.ngeom):
            gs = spec.geom[g]
            if gs.type == PLANE and e > 0:
                continue
            bR = quat_mat(xquat[e, gs.body])
            c = xpos[e, gs.body] + bR @ np.array(list(gs.pos), float) + (np.asarray(offsets[e], float) if offsets is not None else 0.0)
            R = quat_mat(qmul(xquat[e, gs.body], np.array(list(gs.quat), float)))
            s = np.array(list(gs.size), float)
            typ = gs.type
            if typ == HULL:
                v = np.array([[float(np.float32(spec.vert[i][k])) for k in range(3)] for i in range(int(s[0]), int(s[0]) + int(s[1]))])
                typ, s = BOX, np.abs(v).max(0)
            elif typ in (SPHERE, CAPSULE) and not round:
                s = np.array([s[0], s[0], s[0] + (s[1] if typ == CAPSULE else 0.0)])
                typ = BOX
            out.append((e, g, typ, c, R, s))
    return out


def _rect(c, rad, cpos, basis, cam):
    """conservative pixel rectangle (j0, j1, i0, i1) of a sphere (c, rad), or None when it is wholly behind the camera"""
    f, r, u, tx, ty = basis
    v = c - cpos
    z, x, y = v @ f, v @ r, v @ u
    W, H = cam.width, cam.height
    if z + rad <= 0.0:
        return None
    if z - rad <= 1e-6:
        return 0, H, 0, W
    xr = [(x + sx) / (z + sz) for sx in (-rad, rad) for sz in (-rad, rad)]
    yr = [(y + sy) / (z + sz) for sy in (-rad, rad) for sz in (-rad, rad)]
    i0 = int(np.floor((min(xr) / tx + 1.0) * 0.5 * W)) - 1
    i1 = int(np.ceil((max(xr) / tx + 1.0) * 0.5 * W)) + 2
    j0 = int(np.floor((1.0 - max(yr) / ty) * 0.5 * H)) - 1
    j1 = int(np.ceil((1.0 - min(yr) / ty) * 0.5 * H)) + 2
    i0, i1, j0, j1 = max(i0, 0), min(i1, W), max(j0, 0), min(j1, H)
    if i0 >= i1 or j0 >= j1:
        return None
    return j0, j1, i0, i1


def _sphere(o, d, r):
    """entry t and hit mask of rays o + t d (o: (3,), d: (..., 3)) on the sphere |p| = r about the origin (o outside it)"""
    dd = np.einsum("...k,...k->...", d, d)
    beta = d @ o
    cr = np.cross(o[None], d.reshape(-1, 3)).reshape(d.shape)
    disc = r * r * dd - np.einsum("...k,...k->...", cr, cr)
    ok = (disc >= 0.0) & (beta < 0.0)
    t = (-beta - np.sqrt(np.maximum(disc, 0.0))) / dd
    return np.where(ok, t, np.inf)


def _capsule(o, d, r, hl):
    """entry t (inf = miss) and the unit normal in the frame, of rays o + t d on the capsule of radius r about |z| <= hl"""
    t = np.minimum(_sphere(o - [0, 0, hl], d, r), _sphere(o + [0, 0, hl], d, r))
    c2 = d[..., 0] ** 2 + d[..., 1] ** 2
    ac = o[0] ** 2 + o[1] ** 2 - r * r
    if ac > 0.0 and hl > 0.0:
        b = o[0] * d[..., 0] + o[1] * d[..., 1]
        cz = o[0] * d[..., 1] - o[1] * d[..., 0]
        disc = r * r * c2 - cz * cz
        with np.errstate(divide="ignore", invalid="ignore"):
            tl = (-b - np.sqrt(np.maximum(disc, 0.0))) / c2
        ok = (disc >= 0.0) & (b < 0.0) & (c2 > 0.0) & (np.abs(o[2] + tl * d[..., 2]) <= hl)
        t = np.where(ok & (tl < t), tl, t)
    p = o + np.where(np.isfinite(t), t, 0.0)[..., None] * d
    n = p - np.clip(p[..., 2], -hl, hl)[..., None] * np.array([0.0, 0.0, 1.0])
    return t, n / r


def _box(o, d, h):
    """entry t (inf = miss) and the unit normal in the frame, of rays o + t d on the box of half extents h (o outside it)"""
    tn = np.full(d.shape[:-1], -np.inf)
    tf = np.full(d.shape[:-1], np.inf)
    n = np.zeros(d.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(3):
            dk = d[..., k]
            t1, t2 = (-h[k] - o[k]) / dk, (h[k] - o[k]) / dk
            lo, hi = np.minimum(t1, t2), np.maximum(t1, t2)
            par = dk == 0.0
            lo = np.where(par, np.where(abs(o[k]) > h[k], np.inf, -np.inf), lo)
            hi = np.where(par, np.where(abs(o[k]) > h[k], -np.inf, np.inf), hi)
            upd = lo > tn
            tn = np.where(upd, lo, tn)
            nk = np.zeros(d.shape)
            nk[..., k] = np.where(dk > 0, -1.0, 1.0)
            n = np.where(upd[..., None], nk, n)
            tf = np.minimum(tf, hi)
    ok = (tn <= tf) & (tn > 1e-6)
    return np.where(ok, tn, np.inf), n


def cast(spec, cam, vis, xpos, xquat, offsets=None, round=True, pos=None, lookat=None):
    """One image of the geoms of nenv envs (offsets (nenv, 3) or None), see the module docstring."""
    W, H = cam.width, cam.height
    cpos = np.array(list(cam.pos if pos is None else pos), float)
    d, basis = rays(cam, pos, lookat)
    t = np.full((H, W), np.inf)
    geom = np.full((H, W), -1, np.int64)
    env = np.full((H, W), -1, np.int64)
    nrm = np.zeros((H, W, 3))
    cell = np.zeros((H, W), np.int64)
    alb = np.zeros((H, W, 3))
    for e, g, typ, c, R, s in prims(spec, xpos, xquat, offsets, round):
        oc = cpos - c
        if typ == PLANE:
            n = R[:, 2]
            dn, on = d @ n, oc @ n
            with np.errstate(divide="ignore", invalid="ignore"):
                tp = -on / dn
            ok = (dn != 0.0) & (tp > 1e-6) & (tp < t)
            hit = cpos + np.where(ok, tp, 0.0)[..., None] * d - c
            a = np.floor(hit @ R[:, 0] / vis.checker_size).astype(np.int64)
            b = np.floor(hit @ R[:, 1] / vis.checker_size).astype(np.int64)
            chk = np.array([list(vis.checker_rgb[0]), list(vis.checker_rgb[1])])[(a + b) & 1]
            t = np.where(ok, tp, t)
            geom[ok], env[ok] = g, e
            nrm[ok] = (1.0 if on >= 0.0 else -1.0) * n
            alb[ok] = chk[ok]
            cell[ok] = ((a + b) & 1)[ok]
            continue
        o = R.T @ oc
        if typ == BOX:
            rad = float(np.linalg.norm(s))
            inside = bool((np.abs(o) <= s).all())
        elif typ == SPHERE:
            rad = s[0]
            inside = o @ o <= s[0] * s[0]
        else:
            rad = s[0] + s[1]
            inside = o[0] ** 2 + o[1] ** 2 + (o[2] - np.clip(o[2], -s[1], s[1])) ** 2 <= s[0] * s[0]
        rc = None if inside else _rect(c, rad, cpos, basis, cam)
        if rc is None:
            continue
        j0, j1, i0, i1 = rc
        dl = d[j0:j1, i0:i1] @ R  # the rays in the geom frame
        if typ == BOX:
            tg, ng = _box(o, dl, s)
        else:
            tg, ng = _capsule(o, dl, s[0], s[1] if typ == CAPSULE else 0.0)
        sub = (slice(j0, j1), slice(i0, i1))
        ok = np.isfinite(tg) & (tg < t[sub])
        t[sub] = np.where(ok, tg, t[sub])
        geom[sub][ok], env[sub][ok] = g, e
        nrm[sub][ok] = (ng @ R.T)[ok]
        alb[sub][ok] = np.array(list(vis.geom_rgb[g]))
        cell[sub][ok] = (np.abs(ng) @ [1, 2, 3] * 2 + (ng.sum(-1) > 0))[ok] if typ == BOX else 0
    L = np.array(list(vis.light_dir), float)
    L /= np.linalg.norm(L)
    hit = np.isfinite(t)
    sh = vis.ambient + vis.diffuse * np.maximum(nrm @ L, 0.0)
    col = np.where(hit[..., None], alb * sh[..., None], np.array(list(vis.sky_rgb)))
    rgb = np.floor(np.clip(col, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
    return {"t": np.where(hit, t, -1.0), "geom": geom, "env": env, "normal": nrm, "rgb": rgb, "cell": cell}


def normal_u8(n):
    """a unit normal as the normal image stores it: round((n + 1) / 2 x 255), clamped"""
    return np.floor(np.clip((n + 1.0) * 0.5, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)


def silhouette(ids):
    """pixels whose 3 x 3 neighbourhood holds more than one id (edge pixels replicated)"""
    p = np.pad(ids, 1, mode="edge")
    H, W = ids.shape
    out = np.zeros(ids.shape, bool)
    for dj in (0, 1, 2):
        for di in (0, 1, 2):
            out |= p[dj:dj + H, di:di + W] != ids
    return out
