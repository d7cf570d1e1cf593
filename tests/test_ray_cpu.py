"""Range sensing without a GPU: the float64 reference of mir_raycast (tests/ray_ref.py) pinned from first principles, the ray patterns
and the sensor plumbing of gym_genesis/tasks/sensors.py, and the condition under which the GPU tests compare -- at most 2 % of the rays
of every case of tests/ray_cases.py are ambiguous.
"""
import numpy as np
import pytest
import torch

import orc
import ray_cases
import ray_ref
import round_caster
from gym_genesis.backend import models
from gym_genesis.backend import spec as S
from gym_genesis.backend.spec import make_camera, make_ray_query
from gym_genesis.tasks import sensors

I4 = (1.0, 0.0, 0.0, 0.0)


def _one(gtype, size=(0, 0, 0), quat=I4, pos=(0.0, 0.0, 1.0), vertices=None, plane=False):
    """a scene with one geom on the world body (and optionally the floor) -> (ray_ref.Scene, xpos, xquat) of one env"""
    sb = S.SceneBuilder()
    if plane:
        sb.add_geom(0, S.GEOM_PLANE)
    if vertices is None:
        sb.add_geom(0, gtype, size=size, pos=pos, quat=quat)
    else:
        sb.add_geom(0, gtype, pos=pos, quat=quat, vertices=vertices)
    return ray_ref.Scene(sb.build()), np.zeros((1, 3)), np.array([I4])


def _cast(sc, origin, dirs, max_range=100.0, min_range=0.0, **kw):
    scene, xp, xq = sc
    return ray_ref.raycast_env(scene, xp, xq, 0, origin, I4, np.atleast_2d(np.array(dirs, float)), min_range, max_range, **kw)


def test_known_answers():
    h = 1.7
    r = _cast(_one(S.GEOM_BOX, (0.1, 0.1, 0.1), pos=(5, 5, 5), plane=True), (0.2, -0.3, h), [(0, 0, -1), (0, 0, -3), (0, 0, 1), (0, 0, 0)])
    assert np.allclose(r["t"][:2], h, atol=1e-15) and np.all(r["geom"] == [0, 0, -1, -1]) and np.allclose(r["normal"][0], (0, 0, 1))
    assert np.allclose(r["points"][1], (0, 0, -h)) and np.all(r["distance"][2:] == 100.0) and not r["ambiguous"][3]
    assert np.allclose(_cast(_one(S.GEOM_BOX, (0.1, 0.1, 0.1), pos=(5, 5, 5), plane=True), (0, 0, -h), [(0, 0, 1)])["normal"][0], (0, 0, -1)), "two-sided"
    # sphere of radius 0.25 at (0, 0, 1): centre hit from the side, a tangent miss, an origin inside
    sph = _one(S.GEOM_SPHERE, (0.25, 0, 0))
    r = _cast(sph, (2.0, 0, 1.0), [(-1, 0, 0), (-2.0, 2.0 * np.tan(np.arcsin(0.125)) + 1e-6, 0), (-2.0, 0.2, 0)])
    assert abs(r["t"][0] - 1.75) < 1e-15 and np.allclose(r["normal"][0], (1, 0, 0)) and r["geom"][1] == -1 and r["geom"][2] == 0
    p = np.array((2.0, 0, 1.0)) + r["points"][2]
    assert abs(np.linalg.norm(p - (0, 0, 1.0)) - 0.25) < 1e-14, "the hit point lies on the sphere"
    assert _cast(sph, (0.1, 0.0, 1.1), [(1, 0, 0), (0, 0, -1)])["geom"].tolist() == [-1, -1], "a solid that contains the origin is not seen"
    # capsule r 0.1, hl 0.3 about z: its side, its cap, beside the cap
    cap = _one(S.GEOM_CAPSULE, (0.1, 0.3, 0))
    r = _cast(cap, (1.0, 0, 1.2), [(-1, 0, 0)])
    assert abs(r["t"][0] - 0.9) < 1e-15 and np.allclose(r["normal"][0], (1, 0, 0))
    r = _cast(cap, (0.0, 0, 3.0), [(0, 0, -1)])
    assert abs(r["t"][0] - 1.6) < 1e-15 and np.allclose(r["normal"][0], (0, 0, 1))
    r = _cast(cap, (1.0, 0, 1.35), [(-1, 0, 0)])
    assert abs(r["t"][0] - (1.0 - np.sqrt(0.1 ** 2 - 0.05 ** 2))) < 1e-15, "the rounded cap"
    # box rotated by 90 deg about z: its x half extent lies along world y
    c = np.sqrt(0.5)
    box = _one(S.GEOM_BOX, (0.3, 0.1, 0.2), quat=(c, 0, 0, c))
    r = _cast(box, (0.0, 2.0, 1.0), [(0, -1, 0)])
    assert abs(r["t"][0] - 1.7) < 1e-15 and np.allclose(r["normal"][0], (0, 1, 0), atol=1e-15)
    r = _cast(box, (2.0, 0.0, 1.0), [(-1, 0, 0), (-2.0, 0.3 + 1e-9, 0), (-1, 0, 0)], max_range=1.5)
    assert r["geom"].tolist() == [-1, -1, -1] and np.all(r["distance"] == 1.5), "max_range shorter than the hit: a miss"
    r = _cast(box, (2.0, 0.0, 1.0), [(-1, 0, 0)], min_range=2.5)
    assert r["geom"][0] == 0 and abs(r["t"][0] - 1.9) < 1e-15 and r["distance"][0] == 2.5, "min_range longer than the hit: clamped, geom kept"
    # world frame: points = origin + distance x direction
    r = _cast(box, (2.0, 0.0, 1.0), [(-1, 0, 0)], world_frame=True)
    assert np.allclose(r["points"][0], (0.1, 0.0, 1.0), atol=1e-15)


def test_a_hull_of_box_vertices_is_the_box():
    rng = np.random.default_rng(5)
    h = (0.2, 0.1, 0.3)
    q = rng.normal(size=4)
    q = tuple(q / np.linalg.norm(q))
    o = (1.0, -0.7, 1.9)
    d = (np.array((0.0, 0.0, 1.0)) - o) / np.linalg.norm(np.array((0.0, 0.0, 1.0)) - o) + 0.2 * rng.normal(size=(2000, 3))
    a = _cast(_one(S.GEOM_BOX, h, quat=q), o, d, with_ambiguous=False)
    b = _cast(_one(S.GEOM_HULL, quat=q, vertices=S.box_hull_vertices(h)), o, d, with_ambiguous=False)
    assert 200 < (a["geom"] >= 0).sum() < 1800 and np.array_equal(a["geom"], b["geom"])
    assert np.abs(a["distance"] - b["distance"]).max() <= 1e-12 and np.abs(a["normal"] - b["normal"]).max() <= 1e-12
    with pytest.raises(ValueError):
        ray_ref.hull_planes([(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0)])


def test_the_icosphere_hull_lies_between_its_inscribed_and_circumscribed_spheres():
    R = 0.2
    verts = S.icosphere_vertices(R, 1)
    assert len(verts) == 32
    n, dd = ray_ref.hull_planes(verts)
    r_in = dd.min()
    assert 0.8 * R < r_in < R and len(dd) == 60
    o = (0.0, 0.0, 3.0)
    d = np.array((0.0, 0.0, -1.0)) + 0.08 * np.random.default_rng(6).normal(size=(500, 3))
    hull = _cast(_one(S.GEOM_HULL, vertices=verts), o, d, with_ambiguous=False)
    inner = _cast(_one(S.GEOM_SPHERE, (r_in, 0, 0)), o, d, with_ambiguous=False)
    outer = _cast(_one(S.GEOM_SPHERE, (R, 0, 0)), o, d, with_ambiguous=False)
    assert 50 < (inner["geom"] >= 0).sum() < 450
    assert np.all(hull["t"] <= inner["t"] + 1e-12) and np.all(hull["t"] >= outer["t"] - 1e-12)


def test_against_the_round_caster_on_the_pick_scene():
    c = ray_cases.case("pick")
    spec = c["spec"]
    pat = sensors.DepthCameraPattern((16, 12), 50.0)
    pos, look = (1.2, 0.0, 0.9), (0.3, 0.0, 0.2)
    cam = make_camera(16, 12, pos, look, 50.0)
    vis = c["sb"].visual(round_geoms=True)
    # (the oracle's link quaternions are unit to 1e-7; round_caster takes a quaternion as it is, the reference normalises it, as
    #  mir_link_kinematics defines a link's rotation: both get the normalised ones)
    xqn = c["xq"] / np.linalg.norm(c["xq"], axis=-1, keepdims=True)
    for e in range(2):
        rc = round_caster.cast(spec, cam, vis, c["xp"][e:e + 1], xqn[e:e + 1], round=True)
        d, _ = round_caster.rays(cam)
        r = ray_ref.raycast_env(c["scene"], c["xp"][e], xqn[e], 0, pos, sensors.lookat_quat(pos, look), pat.directions().astype(np.float64), 0.0, 50.0,
                                with_ambiguous=False)
        both = (rc["geom"].reshape(-1) == r["geom"]) & (r["geom"] >= 0)
        assert both.sum() > 150
        want = (rc["t"] * np.linalg.norm(d, axis=-1)).reshape(-1)
        # (the pattern's directions are float32: the two rays differ by 6e-8 rad, a few 1e-8 m of range at these distances)
        dd = sensors._unit(pat.rays().reshape(-1, 3))
        r64 = ray_ref.raycast_env(c["scene"], c["xp"][e], xqn[e], 0, pos, sensors.lookat_quat(pos, look), dd, 0.0, 50.0, with_ambiguous=False)
        assert np.abs(r64["t"] - want)[both].max() <= 1e-9
        assert np.abs(np.abs((r64["normal"] @ r64["Rs"].T) - rc["normal"].reshape(-1, 3))[both]).max() <= 1e-9


def test_patterns():
    sp = sensors.SphericalPattern((360.0, 30.0), (64, 16))
    d = sp.directions()
    assert sp.shape == (64, 16) and d.shape == (1024, 3) and d.dtype == np.float32
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1).max() < 1e-6
    g = d.reshape(64, 16, 3)
    el = np.radians(15.0)
    assert np.allclose(g[0, 0], (-np.cos(el), 0, -np.sin(el)), atol=1e-6) and np.allclose(g[32, 15], (np.cos(el), 0, np.sin(el)), atol=1e-6)
    assert np.allclose(g[63, 0, :2] / np.cos(el), (np.cos(np.pi - 2 * np.pi / 64), np.sin(np.pi - 2 * np.pi / 64)), atol=1e-6), "a full turn leaves out its end"
    half = sensors.SphericalPattern((90.0, 0.0), (3, 1)).directions()
    assert np.allclose(half, [(np.sqrt(0.5), -np.sqrt(0.5), 0), (1, 0, 0), (np.sqrt(0.5), np.sqrt(0.5), 0)], atol=1e-6)
    gp = sensors.GridPattern(0.5, (1.0, 2.0))
    d = gp.directions().reshape(3, 5, 3)
    assert gp.shape == (3, 5) and np.allclose(d[1, 2], (0, 0, -1)) and np.abs(np.linalg.norm(d, axis=-1) - 1).max() < 1e-6
    corner = d[0, 0] / -d[0, 0, 2]
    assert np.allclose(sorted(np.abs(corner[:2])), (0.5, 1.0), atol=1e-6) and np.allclose(d[0, 0, :2], -d[2, 4, :2], atol=1e-6)
    dc = sensors.DepthCameraPattern((4, 2), 90.0)
    d = dc.directions().reshape(2, 4, 3)
    assert dc.shape == (2, 4) and np.abs(np.linalg.norm(d, axis=-1) - 1).max() < 1e-6
    # pixel centres, row 0 at the top, d = F + x R + y U with F = +x, R = -y, U = +z: tan(45) = 1 vertically, 2 horizontally
    assert np.allclose(d[0, 0] / d[0, 0, 0], (1, 1.5, 0.5), atol=1e-6) and np.allclose(d[1, 3] / d[1, 3, 0], (1, -1.5, -0.5), atol=1e-6)
    # ... which is the camera of mirigid.h looking along `lookat - pos`
    cam = make_camera(4, 2, (1.0, 2.0, 3.0), (0.0, 0.5, 1.0), 90.0)
    want, _ = round_caster.rays(cam)
    Rs = ray_ref.qmat(sensors.lookat_quat((1.0, 2.0, 3.0), (0.0, 0.5, 1.0)))
    assert np.abs(dc.rays() @ Rs.T - want).max() < 1e-12
    assert np.allclose(ray_ref.qmat(sensors.euler_to_quat((0, 0, 90))) @ (1, 0, 0), (0, 1, 0)) and np.allclose(ray_ref.qmat(sensors.euler_to_quat((90, 0, 90))) @ (0, 1, 0), (0, 0, 1))


class _Recorder:
    """stands in for a MirScene: records what the sensor passes to raycast"""

    def __init__(self, spec, n):
        self.spec, self.num_envs, self.device, self.calls = spec, n, torch.device("cpu"), []

    def raycast(self, dirs, **kw):
        self.calls.append(dict(dirs=dirs, **kw))
        R = self.num_envs if kw["env_idx"] is None else int(kw["env_idx"].numel())
        N = dirs.shape[0]
        out = {}
        if kw["distance"]:
            out["distance"] = torch.full((R, N), 2.0)
        if kw["points"]:
            out["points"] = torch.zeros((R, N, 3))
        if kw["geom"]:
            out["geom"] = torch.zeros((R, N), dtype=torch.int32)
        if kw["normal"]:
            out["normal"] = torch.zeros((R, N, 3))
        return out


def test_the_sensor_passes_on_mask_offsets_frame_rows_and_shapes():
    from gym_genesis.tasks.views import EntityView, SceneView

    sb = models.franka_cube_pick_scene()
    spec = sb.build()
    mir = _Recorder(spec, 6)
    scene = SceneView(mir)
    robot = EntityView(mir, sb, "link0" if "link0" in [b["name"] for b in sb.bodies] else sb.bodies[1]["name"], [])
    hand = robot.get_link("hand")
    pat = sensors.SphericalPattern((360.0, 30.0), (8, 4))
    s = scene.add_sensor(sensors.Lidar(pattern=pat, link=hand, pos_offset=(0.0, 0.1, 0.2), euler_offset=(0.0, 0.0, 90.0), min_range=0.05, max_range=7.0,
                                       return_world_frame=True))
    own = {g for g in range(spec.ngeom) if spec.geom[g].body in robot.link_idx}
    assert own and s.skip_geoms == sum(1 << g for g in own), "skip_own_entity: every geom of the hand's kinematic tree"
    r = s.read()
    assert r._fields == ("points", "distances") and r.points.shape == (6, 8, 4, 3) and r.distances.shape == (6, 8, 4)
    k = mir.calls[-1]
    assert k["link"] == hand.idx and k["pos_offset"] == (0.0, 0.1, 0.2) and np.allclose(k["quat_offset"], (np.sqrt(0.5), 0, 0, np.sqrt(0.5)))
    assert k["min_range"] == 0.05 and k["max_range"] == 7.0 and k["world_frame"] is True and k["env_idx"] is None and k["skip_geoms"] == s.skip_geoms
    assert k["distance"] and k["points"] and not k["geom"] and not k["normal"]
    assert k["dirs"] is mir.calls[0]["dirs"] and np.array_equal(k["dirs"].numpy(), pat.directions()), "uploaded once"
    r = s.read(envs_idx=[4, 0, 0], geoms=True, normals=True)
    assert r._fields == ("points", "distances", "geoms", "normals") and r.geoms.shape == (3, 8, 4) and r.normals.shape == (3, 8, 4, 3)
    assert mir.calls[-1]["env_idx"].tolist() == [4, 0, 0] and mir.calls[-1]["geom"] and mir.calls[-1]["normal"]
    assert s.read(envs_idx=np.arange(6)).points.shape[0] == 6 and mir.calls[-1]["env_idx"] is None, "arange(B) is all envs"
    with pytest.raises(IndexError):
        s.read(envs_idx=[6])
    # by entity and link name, own entity kept; fixed in the world; a depth camera's image
    s2 = scene.add_sensor(sensors.Raycaster(pattern=pat, entity=robot, link="hand", skip_own_entity=False))
    assert s2.link_body == hand.idx and s2.skip_geoms == 0
    s3 = scene.add_sensor(sensors.DepthCamera(pattern=sensors.DepthCameraPattern((4, 2), 90.0), pos_offset=(1, 2, 3)))
    assert s3.link_body == 0 and s3.skip_geoms == 0 and s3.quat_offset == (1.0, 0.0, 0.0, 0.0)
    img = s3.read_image(envs_idx=[1])
    cosines = sensors.DepthCameraPattern((4, 2), 90.0).directions()[:, 0].reshape(2, 4)
    assert img.shape == (1, 2, 4) and np.allclose(img[0].numpy(), 2.0 * cosines) and not mir.calls[-1]["points"]
    with pytest.raises(TypeError):
        s.read_image()
    q = make_ray_query(5, 3, (1, 2, 3), (0, 1, 0, 0), 0.5, 9.0, [0, 3], True)
    assert (q.n_rays, q.link_body, q.skip_geoms, q.flags, q.min_range, q.max_range) == (5, 3, 9, 1, 0.5, 9.0) and q.struct_size == 64


@pytest.mark.parametrize("name", ["zoo", "pick", "stack"])
def test_at_most_two_percent_of_the_gpu_tier_rays_are_ambiguous(name):
    c = ray_cases.case(name)
    for si, s in enumerate(c["sensors"]):
        r = ray_cases.reference(name, si)
        share = float(r["ambiguous"].mean())
        hits = float((r["geom"] >= 0).mean())
        print(f"[{name}, {s['label']}] {r['geom'].size} rays, {100 * hits:.1f} % hit, {100 * share:.2f} % ambiguous")
        assert share <= 0.02, (name, s["label"], share)
        assert hits > 0.2 or s["max_range"] < 2.0, "the case casts at something"
    if name == "zoo":
        # every geom type is hit by the world sensor; the hull distances are not those of the bounding box on at least one ray
        r = ray_cases.reference("zoo", 0)
        assert set(range(6)) <= set(np.unique(r["geom"]).tolist())
