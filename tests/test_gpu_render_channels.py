"""Depth, segmentation and normal images of the rasteriser (mir_render_outputs, MirScene.render_outputs, CameraView.render /
render_batch) against the float64 ray caster of the oracle (oracle/orc_render.c) and against the RGB path.

Definitions (include/mirigid.h): depth = planar camera-z metres (sky 0.0); segmentation = the visible geom's body
("link") or geom index (sky -1); normal = the visible face's outward world normal as round((n + 1) / 2 * 255) (sky 0 0 0).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import orc
from gym_genesis.backend import models
from gym_genesis.backend.spec import make_camera

pytestmark = pytest.mark.gpu

HOME = np.array(models.FRANKA_HOME, dtype=np.float32)
GEOM_PLANE, GEOM_SPHERE, GEOM_CAPSULE = 0, 2, 3


def _stepped_scene(builder, B, steps=30, seed=0):
    from gym_genesis.backend.lib import MirScene

    sc = MirScene(builder.build(), B)
    rng = np.random.RandomState(seed)
    pos = np.stack([rng.uniform(0.45, 0.80, B), rng.uniform(-0.25, 0.25, B), np.full(B, 0.02)], 1).astype(np.float32)
    sc.reset(pos, np.tile(np.array([0, 0, 0, 1], np.float32), (B, 1)), np.tile(HOME, (B, 1)))
    acts = torch.as_tensor(rng.uniform(-1, 1, (steps, B, 9)).astype(np.float32), device=sc.device)
    for t in range(steps):
        sc.set_pd_targets(acts[t])
        sc.step(1)
    return sc


def _stack_scene(B, seed=3):
    from gym_genesis.backend.lib import MirScene

    b = models.franka_cube_stack_scene()
    st = MirScene(b.build(), B)
    rng = np.random.RandomState(seed)
    pos = np.zeros((B, 5, 3), np.float32)
    pos[:, :, 0] = np.array([-0.3, -0.15, 0.0, 0.15, 0.3]) + rng.uniform(-0.03, 0.03, (B, 5))
    pos[:, :, 1] = rng.uniform(-0.2, 0.2, (B, 5))
    pos[:, :, 2] = models.STACK_CUBE_Z
    st.reset(pos, np.tile(np.array([0, 0, 0, 1], np.float32), (B, 5, 1)), np.tile(HOME, (B, 1)))
    st.step(3)
    return b, st


def _quat_mat(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _geoms(spec):
    """(body, type, half extents as the renderer draws them, geom pos, geom rotation) per geom"""
    out = []
    for g in range(spec.ngeom):
        gs = spec.geom[g]
        s = list(gs.size)
        h = {GEOM_SPHERE: (s[0], s[0], s[0]), GEOM_CAPSULE: (s[0], s[0], s[0] + s[1])}.get(gs.type, (s[0], s[1], s[2]))
        out.append((gs.body, gs.type, np.array(h), np.array(list(gs.pos)), _quat_mat(list(gs.quat))))
    return out


def _basis(pos, lookat, up):
    pos, lookat, up = (np.array(list(v), float) for v in (pos, lookat, up))
    f = lookat - pos
    f /= np.linalg.norm(f)
    r = np.cross(f, up)
    for fb in ((0.0, 1.0, 0.0), (1.0, 0.0, 0.0)):
        if r @ r >= 1e-12:
            break
        r = np.cross(f, fb)
    r /= np.linalg.norm(r)
    return f, r, np.cross(r, f)


def _rays(cam, pos, lookat, up):
    """(H, W, 3) un-normalised pixel rays d = F + x R + y U (t along d is the planar depth)"""
    f, r, u = _basis(pos, lookat, up)
    ty = np.tan(0.5 * np.radians(cam.fov_deg))
    tx = ty * cam.width / cam.height
    xs = -tx + tx / cam.width + np.arange(cam.width) * 2 * tx / cam.width
    ys = ty - ty / cam.height - np.arange(cam.height) * 2 * ty / cam.height
    return f[None, None] + xs[None, :, None] * r[None, None] + ys[:, None, None] * u[None, None]


def _check_surfaces(geoms, xpos, xquat, cam_pos, rays, t_ref, seg_geom, seg_link, normal, max_frac):
    """Every pixel with geom id g >= 0: the oracle's hit point lies on g's surface, the decoded normal is the outward normal of the
    face it lies on (a plane's: facing the camera) within 1 LSB, and the link image is g_body of the geom image."""
    body = np.array([g[0] for g in geoms])
    assert np.array_equal(seg_link, np.where(seg_geom >= 0, body[np.maximum(seg_geom, 0)], -1))
    hit = (seg_geom >= 0) & (t_ref > 0)
    bad = np.zeros(seg_geom.shape, bool)
    bad |= (seg_geom >= 0) != (t_ref > 0)
    for g, (b, typ, h, gp, gR) in enumerate(geoms):
        m = hit & (seg_geom == g)
        if not m.any():
            continue
        bR = _quat_mat(xquat[b])
        c, R = xpos[b] + bR @ gp, bR @ gR
        P = np.array(list(cam_pos), float) + t_ref[m][:, None] * rays[m]
        p = (P - c) @ R                       # the hit point in the geom's frame
        if typ == GEOM_PLANE:
            on = np.abs(p[:, 2]) <= 1e-4
            side = 1.0 if (np.array(list(cam_pos), float) - c) @ R[:, 2] > 0 else -1.0
            n = np.tile(side * R[:, 2], (len(p), 1))
        else:
            q = np.abs(p) / h
            on = np.abs(q.max(1) - 1.0) <= 1e-3
            k = q.argmax(1)
            n = np.sign(p[np.arange(len(p)), k])[:, None] * R[:, k].T
        want = np.clip(np.round((n + 1.0) * 0.5 * 255.0), 0, 255)
        ok_n = (np.abs(normal[m].astype(int) - want.astype(int)) <= 1).all(1)
        sub = np.zeros(m.sum(), bool)
        sub |= ~on | ~ok_n
        bad[m] |= sub
    assert bad.mean() <= max_frac, f"{bad.sum()} pixels off their surface or normal ({bad.mean():.2e} of the image)"


def _check_depth(depth, t_ref, max_frac):
    both = (depth > 0) & (t_ref > 0)
    sky = (depth == 0) & (t_ref < 0)
    assert (depth >= 0.0).all()
    ok = sky | (both & (np.abs(depth - t_ref) <= 1e-4 * t_ref))
    assert (~ok).mean() <= max_frac, f"{(~ok).sum()} depth pixels off ({(~ok).mean():.2e} of the image)"


def _all(sc, cam, vis, **kw):
    """(rgb, depth, seg geom, seg link, normal) as NumPy"""
    r, d, sg, n = sc.render_outputs(cam, vis, rgb=True, depth=True, segmentation=True, normal=True, seg_level="geom", **kw)
    sl = sc.render_outputs(cam, vis, rgb=False, segmentation=True, **kw)[2]
    return tuple(t.cpu().numpy() for t in (r, d, sg, sl, n))


@pytest.mark.parametrize("res", [(640, 480), (128, 96)])
def test_per_env_channels_match_oracle(res):
    B = 6
    builder = models.franka_cube_pick_scene()
    sc = _stepped_scene(builder, B)
    spec = builder.build()
    cam = make_camera(res[0], res[1], (3.5, 0.0, 2.5), (0, 0, 0.5), 30)
    vis = builder.visual()
    rgb, depth, sg, sl, nrm = _all(sc, cam, vis)
    assert depth.shape == (B, res[1], res[0]) and depth.dtype == np.float32 and sg.dtype == np.int32 and nrm.shape == rgb.shape
    xpos, xquat = (t.cpu().numpy().astype(np.float64) for t in sc.get_links())
    rays = _rays(cam, cam.pos, cam.lookat, cam.up)
    geoms = _geoms(spec)
    for e in range(B):
        _, t_ref = orc.render_image(spec, cam, vis, xpos[e:e + 1], xquat[e:e + 1], want_depth=True)
        _check_depth(depth[e], t_ref, 5e-4)
        _check_surfaces(geoms, xpos[e], xquat[e], cam.pos, rays, t_ref, sg[e], sl[e], nrm[e], 5e-4)
        assert len(np.unique(sg[e])) >= 4


def test_per_env_camera_channels_match_oracle():
    B = 4
    b, sc = _stack_scene(B, seed=0)
    spec = b.build()
    vis = b.visual()
    cam = make_camera(160, 120, (0, 0, 0), (1, 0, 0), 70)
    cp = np.array([[0.6, 0.3 * e - 0.4, 1.3] for e in range(B)], np.float32)
    cl = np.array([[-0.1, 0.0, 0.75]] * B, np.float32)
    cl[0] = cp[0] - [0, 0, 1.0]  # straight down: parallel to up = +z
    rgb, depth, sg, sl, nrm = _all(sc, cam, vis, cam_pos=cp, cam_lookat=cl)
    assert np.array_equal(rgb, sc.render_cams(cam, vis, cp, cl).cpu().numpy())
    xpos, xquat = (t.cpu().numpy().astype(np.float64) for t in sc.get_links())
    geoms = _geoms(spec)
    for e in range(B):
        ce = make_camera(160, 120, cp[e], cl[e], 70)
        _, t_ref = orc.render_image(spec, ce, vis, xpos[e:e + 1], xquat[e:e + 1], want_depth=True)
        _check_depth(depth[e], t_ref, 2e-3)
        _check_surfaces(geoms, xpos[e], xquat[e], cp[e], _rays(ce, cp[e], cl[e], ce.up), t_ref, sg[e], sl[e], nrm[e], 2e-3)


def _grid(B):
    side = int(np.ceil(np.sqrt(B)))
    idx = np.arange(B)
    return np.stack([(idx % side - (side - 1) / 2) * 1.0, (idx // side - (side - 1) / 2) * 1.0, np.zeros(B)], 1).astype(np.float32)


def test_global_channels_match_oracle_and_the_splat_path():
    B = 400
    builder = models.franka_cube_pick_scene()
    sc = _stepped_scene(builder, B, steps=3)
    spec = builder.build()
    vis = builder.visual()
    off = _grid(B)
    offt = torch.as_tensor(off, device=sc.device)
    cam = make_camera(320, 240, (14.0, -3.0, 9.0), (0, 0, 0.5), 40)
    # the splat path (B x ngeom > 512) against the oracle
    _, depth, sg, sl, nrm = _all(sc, cam, vis, mode=1, env_offset=offt)
    assert depth.shape == (240, 320) and nrm.shape == (240, 320, 3)
    xpos, xquat = (t.cpu().numpy() for t in sc.get_links())
    _, t_ref = orc.render_image(spec, cam, vis, xpos, xquat, offsets=off, want_depth=True)
    _check_depth(depth, t_ref, 3e-3)
    body = np.array([g[0] for g in _geoms(spec)])
    assert np.array_equal(sl, np.where(sg >= 0, body[np.maximum(sg, 0)], -1))
    # splat / resolve against the generic tiled kernel, several views (also inside the grid and close up)
    cams = (cam, make_camera(640, 480, (0.0, -18.0, 12.0), (0, 0, 0.0), 50), make_camera(202, 99, (3.0, 2.0, 1.5), (0, 0, 0.3), 70),
            make_camera(640, 480, (0.45, 0.35, 0.5), (0.0, 0.0, 0.35), 60))
    for c in cams:
        sc.debug_render_path(generic=True)
        ref = _all(sc, c, vis, mode=1, env_offset=offt)
        sc.debug_render_path()
        got = _all(sc, c, vis, mode=1, env_offset=offt)
        assert np.array_equal(got[0], sc.render(c, vis, mode=1, env_offset=offt).cpu().numpy())
        for a, r in zip(got[1:], ref[1:]):
            diff = a != r
            diff = diff.any(-1) if diff.ndim == 3 else diff
            assert diff.mean() <= 1e-4, f"{diff.sum()} pixels differ between the two global paths ({c.width}x{c.height})"


def test_binned_aux_equals_generic_aux_bit_for_bit():
    B = 5
    pick = models.franka_cube_pick_scene()
    sc = _stepped_scene(pick, B, steps=12)
    cams = [make_camera(640, 480, (3.5, 0.0, 2.5), (0, 0, 0.5), 30), make_camera(128, 96, (3.5, 0.0, 2.5), (0, 0, 0.5), 30),
            make_camera(200, 77, (0.9, 0.3, 0.6), (0.3, 0.0, 0.4), 70), make_camera(96, 40, (0.0, 0.0, 3.0), (0.4, 0.0, 0.0), 45, up=(1.0, 0.0, 0.0)),
            make_camera(64, 64, (0.3, 0.0, 0.05), (0.65, 0.0, 0.0), 100), make_camera(320, 200, (1.5, 1.0, 1.0), (0.4, 0.0, 0.2), 50, up=(0.3, 0.0, 1.0))]
    b, st = _stack_scene(B)
    stack_cam = make_camera(256, 160, (1.2, 0.0, 1.6), (-0.2, 0.0, 0.75), 50)
    for scene, vis in ((sc, pick.visual()), (st, b.visual())):
        for cam in cams + [stack_cam]:
            scene.debug_render_path(generic=True)
            ref = _all(scene, cam, vis)
            for rows in (0, 32, 160, 480):
                scene.debug_render_path(generic=False, strip_rows=rows)
                got = _all(scene, cam, vis)
                for k in range(5):
                    assert np.array_equal(got[k], ref[k]), f"channel {k}: binned differs from generic ({cam.width}x{cam.height}, rows {rows})"
            scene.debug_render_path()


def test_rgb_is_untouched_by_the_aux_channels():
    B = 8
    builder = models.franka_cube_pick_scene()
    sc = _stepped_scene(builder, B, steps=4)
    vis = builder.visual()
    cam = make_camera(160, 120, (3.5, 0.0, 2.5), (0, 0, 0.5), 30)
    q0, v0 = (t.clone() for t in sc.get_state()[:2])
    before = sc.render(cam, vis).clone()
    r, d, s, n = sc.render_outputs(cam, vis, rgb=True, depth=True)
    assert s is None and n is None and d is not None
    assert torch.equal(r, before)
    sc.render_outputs(cam, vis, rgb=False, depth=True, segmentation=True, normal=True, seg_level="geom")
    assert torch.equal(sc.render(cam, vis), before)
    q1, v1 = sc.get_state()[:2]
    assert torch.equal(q0, q1) and torch.equal(v0, v1)
    d2 = sc.render_outputs(cam, vis, rgb=False, depth=True)[1]
    assert torch.equal(d, d2)


def test_camera_render_returns_all_four_images():
    from gym_genesis.env import GenesisEnv

    B, H, W = 16, 96, 128
    env = GenesisEnv(task="cube_pick", robot="franka", num_envs=B, enable_pixels=True, observation_height=H, observation_width=W,
                     camera_capture_mode="global")
    obs, _ = env.reset(seed=0)
    cam = env.get_cams()
    rgb, depth, seg, nrm = cam.render(depth=True, segmentation=True, normal=True)
    assert rgb.shape == (H, W, 3) and rgb.dtype == np.uint8 and np.array_equal(rgb, obs["pixels"].cpu().numpy())
    assert depth.shape == (H, W) and depth.dtype == np.float32 and (depth > 0).any()
    assert seg.shape == (H, W) and seg.dtype == np.int32 and seg.max() > 0
    assert nrm.shape == (H, W, 3) and nrm.dtype == np.uint8
    assert cam.render(rgb=False, depth=True)[0] is None
    assert np.array_equal(cam.render()[0], rgb)
    g = cam.render(segmentation=True, segmentation_level="geom")[2]
    assert g.shape == (H, W) and ((g >= 0) == (seg >= 0)).all()
    bt = cam.render_batch(depth=True, segmentation=True, normal=True)
    assert tuple(bt[0].shape) == (B, H, W, 3) and tuple(bt[1].shape) == (B, H, W) and bt[2].dtype == torch.int32 and bt[3].is_cuda
    assert torch.equal(bt[0], cam.render_envs())
    env = GenesisEnv(task="cube_stack", robot="franka", num_envs=3, enable_pixels=True, observation_height=60, observation_width=80,
                     camera_capture_mode="per_env")
    obs, _ = env.reset(seed=0)
    top, side, wrist = env.get_cams()
    pos, look, up, _ = env._env._wrist_camera()
    outs = [top.render_batch(depth=True, segmentation=True, normal=True, pos=env._env.PER_ENV_TOP[0], lookat=env._env.PER_ENV_TOP[1]),
            side.render_batch(depth=True, segmentation=True, normal=True, pos=env._env.PER_ENV_SIDE[0], lookat=env._env.PER_ENV_SIDE[1]),
            wrist.render_batch(depth=True, segmentation=True, normal=True, cam_pos=pos, cam_lookat=look, cam_up=up)]
    for o, (h, w) in zip(outs, ((60, 80), (60, 80), (480, 640))):
        assert tuple(o[1].shape) == (3, h, w) and (o[1] > 0).any() and (o[2] >= 0).any()
    assert torch.equal(outs[0][0], obs["pixels"]["top"])


def test_abi_errors():
    B = 2
    builder = models.franka_cube_pick_scene()
    sc = _stepped_scene(builder, B, steps=1)
    from gym_genesis.backend.lib import MirRenderOutputs

    vis = builder.visual()
    cam = make_camera(64, 48, (3.5, 0.0, 2.5), (0, 0, 0.5), 30)
    d = torch.empty((B, 48, 64), dtype=torch.float32, device=sc.device)

    def call(o, c=cam):
        return sc.lib.mir_render_outputs(sc.h, C.byref(c), C.byref(vis), 0, None, None, None, None, C.byref(o), sc._stream())

    o = MirRenderOutputs(C.sizeof(MirRenderOutputs) - 8, 0, None, C.c_void_p(d.data_ptr()), None, None)
    assert call(o) == -1 and b"size" in sc.lib.mir_last_error()
    assert call(MirRenderOutputs(C.sizeof(MirRenderOutputs), 0, None, None, None, None)) == -1
    assert call(MirRenderOutputs(C.sizeof(MirRenderOutputs), 2, None, C.c_void_p(d.data_ptr()), None, None)) == -1
    big = make_camera(32768, 32768, (3.5, 0.0, 2.5), (0, 0, 0.5), 30)   # 3.2e9 bytes of RGB, 4.3e9 of depth
    assert call(MirRenderOutputs(C.sizeof(MirRenderOutputs), 0, None, C.c_void_p(d.data_ptr()), None, None), big) == -2
    assert b"2^32" in sc.lib.mir_last_error()
    assert call(MirRenderOutputs(C.sizeof(MirRenderOutputs), 0, None, C.c_void_p(d.data_ptr()), None, None)) == 0
    torch.cuda.synchronize()
    assert torch.equal(d, sc.render_outputs(cam, vis, rgb=False, depth=True)[1])
