"""Signed distance without a GPU: the float64 reference of mir_signed_distance (tests/dist_ref.py) pinned from first principles, the
share of ambiguous probes of every case of tests/dist_cases.py, and the sphere model EntityView.collision_spheres() derives.
"""
import numpy as np
import pytest

import dist_cases
import dist_ref
import ray_ref
from gym_genesis.backend import spec as S


def _geom(t, size=(0, 0, 0), verts=None):
    g = dict(body=0, type=t, size=np.array(size, float), pos=np.zeros(3), quat=np.array([1.0, 0, 0, 0]))
    if verts is not None:
        g["verts"] = np.array(verts, float)
        g["planes"] = ray_ref.hull_planes(g["verts"])
        g["tris"], g["tri_face"] = dist_ref.hull_triangles(g["verts"], g["planes"])
    return g


H = (0.15, 0.1, 0.2)


def test_box_regions_and_inside():
    box = _geom(dist_ref.BOX, H)
    p = np.array([(0.15 + 0.3, 0.02, -0.1),              # face +x
                  (0.15 + 0.3, 0.1 + 0.4, 0.05),         # edge +x +y
                  (-0.15 - 0.1, -0.1 - 0.2, 0.2 + 0.2),  # vertex - - +
                  (0.1, 0.0, 0.0),                       # inside, nearest face +x (0.05 deep)
                  (0.0, -0.09, 0.15)])                   # inside, nearest face -y (0.01 deep)
    d, cp, n, ill = dist_ref.geom_distance(box, p)
    np.testing.assert_allclose(d, [0.3, 0.5, 0.3, -0.05, -0.01], atol=1e-15)
    np.testing.assert_allclose(cp, [(0.15, 0.02, -0.1), (0.15, 0.1, 0.05), (-0.15, -0.1, 0.2), (0.15, 0, 0), (0, -0.1, 0.15)], atol=1e-15)
    np.testing.assert_allclose(n, [(1, 0, 0), (0.6, 0.8, 0), (-1 / 3, -2 / 3, 2 / 3), (1, 0, 0), (0, -1, 0)], atol=1e-15)
    assert not ill.any()
    # an inside bisector: the lower axis, flagged
    d, cp, n, ill = dist_ref.geom_distance(box, np.array([(0.1, 0.05, 0.0)]))
    assert d[0] == pytest.approx(-0.05) and tuple(n[0]) == (1, 0, 0) and ill[0]


def test_box_as_hull_equals_box():
    rng = np.random.default_rng(5)
    p = rng.uniform(-0.3, 0.3, (600, 3))
    a = dist_ref.geom_distance(_geom(dist_ref.BOX, H), p)
    b = dist_ref.geom_distance(_geom(dist_ref.HULL, verts=S.box_hull_vertices(H)), p)
    ok = ~(a[3] | b[3])
    assert ok.mean() > 0.9 and (a[0] < 0).sum() > 10
    for x, y in zip(a[:3], b[:3]):
        np.testing.assert_allclose(x[ok], y[ok], atol=1e-12, rtol=0)


def test_icosphere_bounds():
    r = 0.15
    ball = _geom(dist_ref.HULL, verts=S.icosphere_vertices(r, 1))
    pn, pd = ball["planes"]
    assert len(pd) == 60
    rng = np.random.default_rng(6)
    p = rng.normal(size=(300, 3))
    p *= (rng.uniform(0.01, 0.5, 300) / np.linalg.norm(p, axis=1))[:, None]
    d, cp, n, _ = dist_ref.geom_distance(ball, p)
    ln = np.linalg.norm(p, axis=1)
    # the hull lies between its inscribed sphere (radius min d_f) and the sphere of its vertices: |p| - r <= d <= |p| - min d_f
    assert (d >= ln - r - 1e-12).all() and (d <= ln - pd.min() + 1e-12).all()
    # outside, a face plane bounds the distance from below; the closest point lies on the hull and the normal points at the probe
    out = d > 0
    assert out.sum() > 100 and (~out).sum() > 20
    assert (d[out] >= (p[out] @ pn.T - pd).max(1) - 1e-12).all()
    assert np.abs((cp @ pn.T - pd).max(1)).max() < 1e-12
    np.testing.assert_allclose((p - cp)[out], d[out, None] * n[out], atol=1e-12)
    np.testing.assert_allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-12)


def test_round_geoms_plane_and_radius():
    d, cp, n, ill = dist_ref.geom_distance(_geom(dist_ref.SPHERE, (0.15, 0, 0)), np.array([(0.0, 0.3, 0.4), (0.0, 0.0, 0.05), (0, 0, 0)]))
    np.testing.assert_allclose(d, [0.35, -0.1, -0.15], atol=1e-15)
    np.testing.assert_allclose(cp, [(0, 0.09, 0.12), (0, 0, 0.15), (0, 0, 0.15)], atol=1e-15)
    assert list(ill) == [False, False, True] and tuple(n[2]) == (0, 0, 1)
    d, cp, n, ill = dist_ref.geom_distance(_geom(dist_ref.CAPSULE, (0.08, 0.2, 0)), np.array([(0.3, 0.0, 0.1), (0.0, 0.0, 0.5), (0.0, 0.02, -0.1), (0, 0, 0.1)]))
    np.testing.assert_allclose(d, [0.22, 0.22, -0.06, -0.08], atol=1e-15)
    np.testing.assert_allclose(cp[:3], [(0.08, 0, 0.1), (0, 0, 0.28), (0, 0.08, -0.1)], atol=1e-15)
    assert list(ill) == [False, False, False, True] and tuple(n[3]) == (0, 0, 1)
    d, cp, n, _ = dist_ref.geom_distance(_geom(dist_ref.PLANE), np.array([(0.3, -0.2, 0.25), (0.3, -0.2, -0.25)]))
    assert list(d) == [0.25, -0.25] and (cp == [(0.3, -0.2, 0), (0.3, -0.2, 0)]).all() and (n == (0, 0, 1)).all()
    # a radius shifts s exactly; a winner beyond max_distance is a miss; the lower geom index keeps a tie
    sc = dist_ref.sphere_scene([(0, 0, 0, 0.1), (1.0, 0, 0, 0.1)])
    xp, xq = np.zeros((1, 3)), np.array([[1.0, 0, 0, 0]])
    probes = np.array([(0.5, 0, 0, 0.0), (0.5, 0, 0, 0.125), (0.25, 0, 0, 0.0), (0.0, 5.0, 0, 0.0)])
    r = dist_ref.signed_distance_env(sc, xp, xq, probes, None, 1.0)
    np.testing.assert_allclose(r["distance"], [0.4, 0.275, 0.15, 1.0], atol=1e-15)
    assert list(r["geom"]) == [0, 0, 0, -1] and list(r["ambiguous"]) == [True, True, False, False]
    assert (r["closest"][3] == (0, 5.0, 0)).all() and (r["normal"][3] == 0).all()


@pytest.mark.parametrize("name", ["zoo", "pick", "stack"])
def test_ambiguous_share(name):
    c, ref = dist_cases.case(name), dist_cases.reference(name)
    amb = ref["ambiguous"]
    print(f"\n[{name}] {len(c['probes'])} probes x {dist_cases.B} envs: {amb.mean():.4%} ambiguous, {int((ref['geom'] >= 0).sum())} within max_distance, "
          f"{int(ref['inside'].sum())} inside a solid")
    assert len(c["probes"]) <= S.DIST_MAX_PROBES
    assert amb.mean() < 0.02
    if name == "zoo":
        own = ref["geom"][:, c["degenerate"][:, 0]] == c["degenerate"][:, 1]   # (elsewhere another body lies over the probe)
        assert len(c["degenerate"]) >= 6 and own.mean() > 0.8 and amb[:, c["degenerate"][:, 0]][own].all(), "the hand-aimed degenerate probes are flagged"
        types = np.array([g["type"] for g in c["dscene"].geoms])
        ok = ~amb & (ref["geom"] >= 0)
        assert set(types[ref["geom"][ok]].tolist()) == {0, 1, 2, 3, 4}, "every geom type wins"
        for gi in range(len(types)):
            assert (ok & ref["inside"] & (ref["geom"] == gi)).sum() >= 3, f"geom {gi}: three unambiguous probes inside"
    cand = dist_cases.reference(name, "candidate")
    assert cand["ambiguous"].mean() < 0.02


@pytest.mark.parametrize("name", ["pick", "stack"])
def test_collision_spheres(name):
    c, robot = dist_cases.case(name), dist_cases.arm(name)
    sb = c["sb"]
    p, lk = robot.collision_spheres()
    p2, lk2 = robot.collision_spheres()
    assert p.dtype == np.float32 and lk.dtype == np.int32 and p.shape == (len(lk), 4) and 1 <= len(lk) <= 512
    assert np.array_equal(p, p2) and np.array_equal(lk, lk2), "deterministic"
    base = sb.body_index("link0")
    covered = set(robot._covered_links())
    assert base not in lk and base not in covered and covered == set(robot.link_idx) - {base}
    assert set(lk.tolist()) == {g["body"] for g in sb.geoms if g["body"] in covered}
    rng = np.random.default_rng(7)
    of_geom = robot._derive_spheres()[2]
    for gi, g in enumerate(sb.geoms):
        if g["body"] not in covered:
            continue
        mine = p[of_geom == gi].astype(np.float64)
        assert len(mine) >= 1 and (lk[of_geom == gi] == g["body"]).all()
        size, t = np.array(g["size"], float), g["type"]
        # a dense sample of the geom's surface (and its vertices), in the link's frame
        if t == S.GEOM_BOX:
            u = rng.uniform(-1, 1, (600, 3))
            u[np.arange(600), rng.integers(0, 3, 600)] = rng.choice([-1.0, 1.0], 600)
            local = np.concatenate([u, np.array(S.box_hull_vertices((1, 1, 1)), float)]) * size
            bound = np.linalg.norm(size)
        elif t == S.GEOM_CAPSULE:
            u = rng.normal(size=(600, 3))
            u /= np.linalg.norm(u, axis=1, keepdims=True)
            z = rng.uniform(-size[1], size[1], 600)
            side = np.stack([size[0] * u[:, 0] / np.hypot(u[:, 0], u[:, 1]), size[0] * u[:, 1] / np.hypot(u[:, 0], u[:, 1]), z], 1)
            caps = size[0] * u + np.where(u[:, 2:3] >= 0, 1, -1) * np.array([0, 0, size[1]])
            local = np.concatenate([side, caps, [(0, 0, size[1] + size[0]), (0, 0, -size[1] - size[0])]])
            bound = size[0] + size[1]
        else:
            raise AssertionError(f"the arm has a geom of type {t}: extend the sample")
        pts = np.array(g["pos"], float) + local @ ray_ref.qmat(g["quat"]).T
        d = dist_ref.signed_distance_env(dist_ref.sphere_scene(mine), np.zeros((1, 3)), np.array([[1.0, 0, 0, 0]]), np.c_[pts, np.zeros(len(pts))], None, 10.0,
                                         with_ambiguous=False)["distance"]
        assert d.max() <= 1e-9, (g, d.max())
        # (the model is float32 and its radii are padded for that rounding by 2^-22 relative: 1e-6 leaves room for it and no more)
        assert mine[:, 3].max() <= bound * (1 + 1e-6), (g, mine[:, 3].max(), bound)
    # a finer model has more spheres; a replacement is what comes back
    assert len(robot.collision_spheres(spacing=0.02)[1]) > len(lk)
    robot.set_collision_spheres(p[:3], lk[:3])
    assert np.array_equal(robot.collision_spheres()[0], p[:3])
    with pytest.raises(ValueError):
        robot.set_collision_spheres(p[:1], [base - 1 if base > 1 else 0])


def test_sphere_model_of_a_hull_and_a_sphere():
    from gym_genesis.tasks.views import EntityView

    sb = dist_cases.case("zoo")["sb"]
    for name in ("ball", "hullbox", "sphere"):
        ent = EntityView(None, sb, name, ())
        p, lk = ent.collision_spheres()
        g = next(g for g in sb.geoms if g["body"] == sb.body_index(name))
        assert (lk == sb.body_index(name)).all()
        if name == "sphere":
            assert p.shape == (1, 4) and g["size"][0] <= p[0, 3] <= g["size"][0] * (1 + 1e-6), "a sphere becomes itself (padded for float32)"
            continue
        v = np.array(sb.verts[int(g["size"][0]):int(g["size"][0]) + int(g["size"][1])])
        w = np.random.default_rng(8).dirichlet(np.ones(len(v)), 500) @ v   # (points of the hull)
        d = dist_ref.signed_distance_env(dist_ref.sphere_scene(p.astype(np.float64)), np.zeros((1, 3)), np.array([[1.0, 0, 0, 0]]),
                                         np.c_[np.concatenate([v, w]), np.zeros(len(v) + 500)], None, 10.0, with_ambiguous=False)["distance"]
        centre = 0.5 * (v.min(0) + v.max(0))   # (a hull's bounding radius: about the centre of its bounding box)
        assert d.max() <= 1e-9 and p[:, 3].max() <= np.linalg.norm(v - centre, axis=1).max() * (1 + 1e-6)


def test_hull_fans_of_the_library():
    """the planes and triangle fans mir_signed_distance builds per hull (mir_hullfan.h through `make dist-host`) on the two zoo hulls:
    the planes are dist_ref's, the fans tile every face (their areas add up to the brute-force face's), the minimum over the fans is
    dist_ref's outside distance, and the flat hull is refused"""
    import ctypes as C
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-s", "-C", os.path.join(root, "gym-genesis_amd", "csrc"), "dist-host"], stdout=subprocess.DEVNULL)
    L = C.CDLL(os.path.join(root, "tests", "_build", "libmirdist.so"))

    def fan(verts):
        v = np.ascontiguousarray(verts, np.float64)
        planes, tris = np.zeros((64, 4), np.float32), np.zeros((192, 3, 4), np.float32)
        npl, ntr = C.c_int(), C.c_int()
        rc = L.dist_host_fan(v.ctypes.data_as(C.c_void_p), len(v), planes.ctypes.data_as(C.c_void_p), 64, C.byref(npl), tris.ctypes.data_as(C.c_void_p), 192, C.byref(ntr))
        return rc, planes[:npl.value], tris[:ntr.value]

    rng = np.random.default_rng(9)
    for verts in (S.box_hull_vertices(dist_cases.ray_cases.ZOO_HULL_BOX), S.icosphere_vertices(dist_cases.ray_cases.ZOO_BALL_R, 1)):
        g = _geom(dist_ref.HULL, verts=verts)
        pn, pd = g["planes"]
        rc, planes, tris = fan(verts)
        assert rc == 0 and len(planes) == len(pd) and len(tris) <= 2 * len(verts) - 4
        # every plane of the library is one of the reference's, once
        match = [int(np.argmin(np.abs(pn @ pl[:3] - 1) + np.abs(pd - pl[3]))) for pl in planes.astype(np.float64)]
        assert sorted(match) == list(range(len(pd)))
        assert max(np.abs(pn[m] - pl[:3]).max() + abs(pd[m] - pl[3]) for m, pl in zip(match, planes.astype(np.float64))) < 1e-6
        # the fans: vertices of the hull, in their face's plane, counter-clockwise seen from outside, areas adding up to the face's
        area = np.zeros(len(planes))
        for t in tris.astype(np.float64):
            f = int(t[0, 3])
            a, b, c = t[:, :3]
            assert all(np.abs(np.asarray(verts) - x).max(1).min() < 1e-7 for x in (a, b, c))
            n = np.cross(b - a, c - a)
            assert n @ planes[f, :3] > 0 and np.abs(t[:, :3] @ planes[f, :3].astype(np.float64) - planes[f, 3]).max() < 1e-6
            area[f] += 0.5 * np.linalg.norm(n)
        assert (np.diff(tris[:, 0, 3]) >= 0).all(), "triangles in face order: the lower face keeps a tie"
        for f, m in enumerate(match):
            on = np.asarray(verts)[np.abs(np.asarray(verts) @ pn[m] - pd[m]) < 1e-9]
            # (the face is convex: the area of its hull = half the sum over its brute-force triples / (k - 2 choose ...) -- by a fan of our own)
            ctr = on.mean(0)
            u = np.cross(pn[m], [1.0, 0, 0] if abs(pn[m][0]) < 0.9 else [0, 1.0, 0])
            u /= np.linalg.norm(u)
            ang = np.arctan2((on - ctr) @ np.cross(pn[m], u), (on - ctr) @ u)
            ring = on[np.argsort(ang)]
            want = 0.5 * sum(np.linalg.norm(np.cross(ring[i] - ctr, ring[(i + 1) % len(ring)] - ctr)) for i in range(len(ring)))
            assert abs(area[f] - want) < 1e-7, (f, area[f], want)
        # the minimum over the fans is the reference's outside distance
        p = rng.normal(size=(200, 3))
        p *= (rng.uniform(0.3, 0.6, 200) / np.linalg.norm(p, axis=1))[:, None]
        d_ref = dist_ref.geom_distance(g, p)[0]
        d_fan = np.sqrt(np.min([dist_ref._triangle(p, t[:, :3], np.float64)[1] for t in tris.astype(np.float64)], axis=0))
        assert (d_ref > 0).all() and np.abs(d_fan - d_ref).max() < 1e-6
    assert fan([(0.1, 0.1, 0.0), (-0.1, 0.1, 0.0), (-0.1, -0.1, 0.0), (0.1, -0.1, 0.0)])[0] == -1
