"""The float64 reference of the round-geom images (tests/round_caster.py) on the CPU: known answers for a sphere and a capsule, and
agreement with the C oracle (oracle/orc_render.c) wherever both draw boxes and planes."""
import numpy as np

import orc
import round_caster as rc
from gym_genesis.backend import models
from gym_genesis.backend.spec import GEOM_BOX, GEOM_CAPSULE, GEOM_PLANE, GEOM_SPHERE, SceneBuilder, make_camera


def _one(gtype, size, quat=(1, 0, 0, 0)):
    b = SceneBuilder()
    b.add_geom(0, GEOM_PLANE)
    b.add_geom(0, gtype, size=size, pos=(0.0, 0.0, 1.0), quat=quat, rgb=(0.9, 0.3, 0.2))
    return b


def _cast(b, cam, **kw):
    spec = b.build()
    return rc.cast(spec, cam, b.visual(), np.zeros((1, spec.nbody, 3)), np.tile([1.0, 0, 0, 0], (1, spec.nbody, 1)), **kw)


def _run_width(mask_row):
    idx = np.flatnonzero(mask_row)
    return idx[-1] - idx[0] + 1 if len(idx) else 0


def test_sphere_depth_and_silhouette():
    r, dist, N, fov = 0.05, 3.0, 201, 10.0
    b = _one(GEOM_SPHERE, (r, 0, 0))
    cam = make_camera(N, N, (dist, 0.0, 1.0), (0.0, 0.0, 1.0), fov)
    out = _cast(b, cam)
    c = N // 2
    assert out["geom"][c, c] == 1
    assert abs(out["t"][c, c] - (dist - r)) < 1e-9
    assert np.allclose(out["normal"][c, c], [1.0, 0.0, 0.0], atol=1e-9)
    px = np.tan(np.arcsin(r / dist)) / (2 * np.tan(np.radians(fov) / 2) / N)  # silhouette radius in pixels
    w = _run_width(out["geom"][c] == 1)
    assert abs(w - 2 * px) <= 1.0, (w, 2 * px)
    assert abs(_run_width(out["geom"][:, c] == 1) - 2 * px) <= 1.0
    # the bounding box (what round=False and the oracle draw) is wider
    boxed = _cast(b, cam, round=False)
    assert (boxed["geom"] == 1).sum() > (out["geom"] == 1).sum() * 1.2


def test_capsule_side_on_and_end_on():
    r, hl, dist, N, fov = 0.04, 0.1, 2.5, 241, 12.0
    pix = 2 * np.tan(np.radians(fov) / 2) / N
    # side on: axis z, camera on +x
    b = _one(GEOM_CAPSULE, (r, hl, 0))
    cam = make_camera(N, N, (dist, 0.0, 1.0), (0.0, 0.0, 1.0), fov)
    out = _cast(b, cam)
    c = N // 2
    assert out["geom"][c, c] == 1 and abs(out["t"][c, c] - (dist - r)) < 1e-9
    assert abs(_run_width(out["geom"][c] == 1) - 2 * np.tan(np.arcsin(r / dist)) / pix) <= 1.0
    # vertical extent: the end spheres' silhouettes
    top = np.arctan(hl / dist) + np.arcsin(r / np.hypot(dist, hl))
    assert abs(_run_width(out["geom"][:, c] == 1) - 2 * np.tan(top) / pix) <= 1.5
    # end on: axis along the view (the geom rotated 90 degrees about y), the near end sphere bounds the silhouette
    s = np.sqrt(0.5)
    b = _one(GEOM_CAPSULE, (r, hl, 0), quat=(s, 0.0, s, 0.0))
    out = _cast(b, cam)
    assert abs(out["t"][c, c] - (dist - hl - r)) < 1e-9
    assert abs(_run_width(out["geom"][c] == 1) - 2 * np.tan(np.arcsin(r / (dist - hl))) / pix) <= 1.0
    assert np.allclose(out["normal"][c, c], [1.0, 0.0, 0.0], atol=1e-9)
    # a camera inside the capsule sees nothing of it
    inside = make_camera(64, 48, (0.0, 0.0, 1.02), (1.0, 0.0, 1.0), 60)
    assert (_cast(_one(GEOM_CAPSULE, (r, hl, 0)), inside)["geom"] != 1).all()


def _random_links(spec, nenv, seed):
    rng = np.random.RandomState(seed)
    xpos = np.stack([rng.uniform(-0.3, 0.7, (nenv, spec.nbody)), rng.uniform(-0.4, 0.4, (nenv, spec.nbody)),
                     rng.uniform(0.05, 1.0, (nenv, spec.nbody))], -1)
    q = rng.normal(size=(nenv, spec.nbody, 4))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    xpos[:, 0], q[:, 0] = 0.0, [1.0, 0.0, 0.0, 0.0]
    return xpos, q


def test_boxes_and_planes_match_the_oracle():
    """Box-only scenes, and round geoms drawn as bounding boxes: the caster's depth and RGB are the oracle's (<= 1 LSB except at
    silhouettes), per env and in a global view of several envs."""
    for shape, round_ in (("box", True), ("capsule", False)):
        b = models.franka_cube_pick_scene(link_shape=shape)
        spec, vis = b.build(), b.visual()
        if round_:
            assert all(spec.geom[g].type in (GEOM_PLANE, GEOM_BOX) for g in range(spec.ngeom))
        xpos, xquat = _random_links(spec, 3, seed=1)
        offs = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
        views = [(make_camera(160, 120, (3.5, 0.0, 2.5), (0, 0, 0.5), 30), xpos[:1], xquat[:1], None),
                 (make_camera(96, 80, (1.0, 0.8, 0.9), (0.2, 0.0, 0.3), 70), xpos[1:2], xquat[1:2], None),
                 (make_camera(128, 96, (4.0, -3.0, 3.0), (0.5, 0.5, 0.3), 45), xpos, xquat, offs)]
        for cam, xp, xq, off in views:
            ref, t_ref = orc.render_image(spec, cam, vis, xp, xq, offsets=off, want_depth=True)
            got = rc.cast(spec, cam, vis, xp, xq, offsets=off, round=round_)
            edge = rc.silhouette(got["geom"] * 64 + got["env"])
            assert ((got["t"] > 0) == (t_ref > 0))[~edge].all()
            both = (got["t"] > 0) & (t_ref > 0) & ~edge
            assert np.allclose(got["t"][both], t_ref[both], rtol=1e-9)
            diff = np.abs(got["rgb"].astype(int) - ref.astype(int)).max(-1)
            assert (diff[~edge] <= 1).all()
            assert (diff > 1).mean() <= 0.01
