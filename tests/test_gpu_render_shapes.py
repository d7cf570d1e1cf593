"""Spheres and capsules drawn as themselves (MIR_VIS_ROUND_GEOMS, SceneBuilder.visual(round_geoms=True)): every render entry point,
mode and pixel path against the float64 ray caster of tests/round_caster.py, and the paths against each other."""
import ctypes as C

import numpy as np
import pytest
import torch

import round_caster as rc
from gym_genesis.backend import models
from gym_genesis.backend.spec import GEOM_CAPSULE, GEOM_SPHERE, make_camera

pytestmark = pytest.mark.gpu

HOME = np.array(models.FRANKA_HOME, dtype=np.float32)
# static round geoms added to the Franka pick scene (world body, no contacts): (type, size, pos, quat)
EXTRA = [(GEOM_SPHERE, (0.06, 0, 0), (0.35, 0.45, 0.25), (1, 0, 0, 0)),
         (GEOM_CAPSULE, (0.04, 0.15, 0), (0.30, 0.50, 0.40), (0.7071068, 0.0, 0.7071068, 0.0)),
         (GEOM_CAPSULE, (0.05, 0.10, 0), (0.60, -0.45, 0.30), (0.9, 0.3, -0.2, 0.25)),
         (GEOM_SPHERE, (0.03, 0, 0), (0.20, -0.35, 0.60), (1, 0, 0, 0)),
         (GEOM_CAPSULE, (0.025, 0.2, 0), (-0.3, 0.0, 0.15), (0.8, 0.0, 0.0, 0.6))]


def _builder(extra=True, link_shape="capsule"):
    b = models.franka_cube_pick_scene(link_shape=link_shape)
    if extra:
        for k, (t, s, p, q) in enumerate(EXTRA):
            b.add_geom(0, t, size=s, pos=p, quat=q, contype=0, conaffinity=0, rgb=(0.2 + 0.15 * k, 0.7, 0.9 - 0.15 * k))
    return b


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


def _all(sc, cam, vis, **kw):
    """(rgb, depth, seg geom, seg link, normal) as NumPy"""
    r, d, sg, n = sc.render_outputs(cam, vis, rgb=True, depth=True, segmentation=True, normal=True, seg_level="geom", **kw)
    sl = sc.render_outputs(cam, vis, rgb=False, segmentation=True, **kw)[2]
    return tuple(t.cpu().numpy() for t in (r, d, sg, sl, n))


def _links(sc):
    return tuple(t.cpu().numpy().astype(np.float64) for t in sc.get_links())


def _check(got, ref, spec, global_view=False, id_frac=2e-3):
    """got = _all(...) of one image, ref = rc.cast(...): ids off silhouettes, depth 2e-4 t, normals and RGB 1 LSB"""
    rgb, depth, sg, sl, nrm = got
    key = (ref["geom"] * 256 + ref["env"]) * 8 + ref["cell"] if global_view else ref["geom"] * 8 + ref["cell"]
    # a silhouette pixel: two surfaces in its 3 x 3 neighbourhood in the reference; a tie: another geom drawn at the reference's depth
    # (coincident surfaces, e.g. the end spheres of two link capsules that meet at a joint)
    edge = rc.silhouette(key)
    bad_id = sg != ref["geom"]
    tie = bad_id & (sg >= 0) & (ref["geom"] >= 0) & (np.abs(depth - ref["t"]) <= 2e-4 * np.abs(ref["t"]))
    far = bad_id & ~edge & ~tie
    assert far.sum() == 0, (f"{far.sum()} pixels with another surface away from any silhouette: got / want geoms "
                            f"{sorted(set(zip(sg[far].tolist(), ref['geom'][far].tolist())))}, depth / t {depth[far] / ref['t'][far]}")
    assert bad_id.mean() <= id_frac, f"{bad_id.sum()} pixels with another surface ({bad_id.mean():.2e})"
    body = np.array([spec.geom[g].body for g in range(spec.ngeom)])
    assert np.array_equal(sl, np.where(sg >= 0, body[np.maximum(sg, 0)], -1))
    ok = ~bad_id & ~edge
    hit = ok & (ref["t"] > 0)
    assert (depth[ok & (ref["t"] < 0)] == 0.0).all()
    assert (np.abs(depth[hit] - ref["t"][hit]) <= 2e-4 * ref["t"][hit]).all(), np.abs(depth[hit] / ref["t"][hit] - 1).max()
    dn = np.abs(nrm.astype(int) - rc.normal_u8(ref["normal"]).astype(int)).max(-1)
    assert (dn[hit] <= 1).all(), f"{(dn[hit] > 1).sum()} normals off by more than 1 LSB"
    dc = np.abs(rgb.astype(int) - ref["rgb"].astype(int)).max(-1)
    assert (dc[ok] <= 1).all(), f"{(dc[ok] > 1).sum()} colours off by more than 1 LSB"


@pytest.mark.parametrize("res", [(640, 480), (128, 96)])
def test_per_env_round_channels_match_caster(res):
    B = 4
    builder = _builder()
    sc = _stepped_scene(builder, B)
    spec, vis = builder.build(), builder.visual(round_geoms=True)
    cams = [make_camera(res[0], res[1], (3.5, 0.0, 2.5), (0, 0, 0.5), 30), make_camera(res[0], res[1], (1.4, 1.1, 0.9), (0.3, 0.0, 0.35), 55)]
    xpos, xquat = _links(sc)
    for cam in cams:
        got = _all(sc, cam, vis)
        for e in range(B):
            ref = rc.cast(spec, cam, vis, xpos[e:e + 1], xquat[e:e + 1])
            _check(tuple(g[e] for g in got), ref, spec)
        assert (np.isin(got[2], [g for g in range(spec.ngeom) if spec.geom[g].type == GEOM_CAPSULE])).any()
        # RGB is what mir_render draws
        assert np.array_equal(got[0], sc.render(cam, vis).cpu().numpy())


def test_per_env_cameras_round_channels_match_caster():
    B = 3
    builder = _builder()
    sc = _stepped_scene(builder, B, steps=10)
    spec, vis = builder.build(), builder.visual(round_geoms=True)
    cam = make_camera(160, 120, (0, 0, 0), (1, 0, 0), 90)
    cp = np.array([[0.5, 0.0, 1.6], [0.30, 0.38, 0.42], [1.2, 0.6, 0.7]], np.float32)
    cl = np.array([[0.5, 0.0, 0.0], [1.30, 0.20, 0.42], [0.3, 0.0, 0.3]], np.float32)  # 0: straight down; 1: the capsule half behind
    rgb, depth, sg, sl, nrm = _all(sc, cam, vis, cam_pos=cp, cam_lookat=cl)
    assert np.array_equal(rgb, sc.render_cams(cam, vis, cp, cl).cpu().numpy())
    xpos, xquat = _links(sc)
    for e in range(B):
        ref = rc.cast(spec, cam, vis, xpos[e:e + 1], xquat[e:e + 1], pos=cp[e], lookat=cl[e])
        _check((rgb[e], depth[e], sg[e], sl[e], nrm[e]), ref, spec)
    assert (sg[1] == spec.ngeom - len(EXTRA) + 1).any()  # the capsule that straddles camera 1's plane is on screen


def _grid(B):
    side = int(np.ceil(np.sqrt(B)))
    idx = np.arange(B)
    return np.stack([(idx % side - (side - 1) / 2) * 1.5, (idx // side - (side - 1) / 2) * 1.5, np.zeros(B)], 1).astype(np.float32)


@pytest.mark.parametrize("B", [3, 48])
def test_global_round_channels_match_caster_on_both_paths(B):
    builder = _builder()
    sc = _stepped_scene(builder, B, steps=5)
    spec, vis = builder.build(), builder.visual(round_geoms=True)
    assert (B * spec.ngeom > 512) == (B == 48)  # 48 envs: the splat path; 3: the generic tiled kernel
    off = _grid(B)
    offt = torch.as_tensor(off, device=sc.device)
    cams = [make_camera(320, 240, (9.0, -3.0, 6.0), (0, 0, 0.5), 45), make_camera(256, 200, (1.8, 1.2, 1.0), (0.0, 0.0, 0.4), 60)]
    xpos, xquat = _links(sc)
    for cam in cams:
        got = _all(sc, cam, vis, mode=1, env_offset=offt)
        ref = rc.cast(spec, cam, vis, xpos, xquat, offsets=off)
        _check(got, ref, spec, global_view=True)
        sc.debug_render_path(generic=True)
        gen = _all(sc, cam, vis, mode=1, env_offset=offt)
        sc.debug_render_path()
        # splat / resolve against the generic kernel: the same w per pixel; ids differ only on exact ties of w
        both = (got[1] > 0) & (gen[1] > 0)
        assert ((got[1] > 0) != (gen[1] > 0)).mean() <= 1e-4
        assert (np.abs(got[1][both] - gen[1][both]) <= 1e-6 * gen[1][both]).all()
        diff = got[2] != gen[2]
        assert (got[1][diff] == gen[1][diff]).all()


def test_round_binned_equals_generic_bit_for_bit():
    B = 3
    builder = _builder()
    sc = _stepped_scene(builder, B, steps=12)
    vis = builder.visual(round_geoms=True)
    cams = [make_camera(640, 480, (3.5, 0.0, 2.5), (0, 0, 0.5), 30), make_camera(200, 77, (0.9, 0.3, 0.6), (0.3, 0.0, 0.4), 70),
            make_camera(96, 40, (0.0, 0.0, 3.0), (0.4, 0.0, 0.0), 45, up=(1.0, 0.0, 0.0)), make_camera(64, 64, (0.3, 0.0, 0.05), (0.65, 0.0, 0.0), 100)]
    for cam in cams:
        sc.debug_render_path(generic=True)
        ref = _all(sc, cam, vis)
        for rows in (0, 32, 160):
            sc.debug_render_path(generic=False, strip_rows=rows)
            got = _all(sc, cam, vis)
            for k in range(5):
                assert np.array_equal(got[k], ref[k]), f"channel {k}: binned differs from generic ({cam.width}x{cam.height}, rows {rows})"
        sc.debug_render_path()


def test_flag_on_a_box_scene_changes_nothing():
    builder = models.franka_cube_pick_scene(link_shape="box")
    sc = _stepped_scene(builder, 40, steps=6)
    assert 40 * builder.build().ngeom > 512
    off, on = builder.visual(), builder.visual(round_geoms=True)
    offt = torch.as_tensor(_grid(40), device=sc.device)
    cam = make_camera(200, 152, (3.5, 0.0, 2.5), (0, 0, 0.5), 30)
    gcam = make_camera(240, 180, (9.0, -3.0, 6.0), (0, 0, 0.5), 45)
    for generic in (False, True):
        sc.debug_render_path(generic=generic)
        for kw, c in (({}, cam), ({"mode": 1, "env_offset": offt}, gcam)):
            a, b = _all(sc, c, off, **kw), _all(sc, c, on, **kw)
            for k in range(5):
                assert np.array_equal(a[k], b[k]), (generic, kw.get("mode", 0), k)
    sc.debug_render_path()


def test_camera_inside_a_round_geom_draws_nothing_of_it():
    builder = _builder()
    sc = _stepped_scene(builder, 2, steps=1)
    spec, vis = builder.build(), builder.visual(round_geoms=True)
    g0 = spec.ngeom - len(EXTRA)
    cam = make_camera(96, 64, (0, 0, 0), (1, 0, 0), 80)
    cp = np.array([[0.35, 0.45, 0.26], [0.36, 0.50, 0.41]], np.float32)  # inside the sphere g0, inside the capsule g0 + 1
    cl = cp + np.array([[0.0, -1.0, 0.0], [0.0, -1.0, 0.1]], np.float32)
    _, depth, sg, _, _ = _all(sc, cam, vis, cam_pos=cp, cam_lookat=cl)
    assert not (sg[0] == g0).any() and not (sg[1] == g0 + 1).any()
    assert (depth > 0).any()


def test_visual_flags_abi():
    from gym_genesis.backend.lib import MirRenderOutputs

    builder = _builder(extra=False)
    sc = _stepped_scene(builder, 2, steps=1)
    cam = make_camera(64, 48, (3.5, 0.0, 2.5), (0, 0, 0.5), 30)
    px = torch.empty((2, 48, 64, 3), dtype=torch.uint8, device=sc.device)
    d = torch.empty((2, 48, 64), dtype=torch.float32, device=sc.device)
    pos = torch.tensor([[3.5, 0.0, 2.5]] * 2, device=sc.device)
    look = torch.tensor([[0.0, 0.0, 0.5]] * 2, device=sc.device)
    o = MirRenderOutputs(C.sizeof(MirRenderOutputs), 0, None, C.c_void_p(d.data_ptr()), None, None)
    for flags, want in ((2, -1), (3, -1), (-1, -1), (1, 0), (0, 0)):
        vis = builder.visual()
        vis.flags = flags
        st = sc._stream()
        assert sc.lib.mir_render(sc.h, C.byref(cam), C.byref(vis), 0, None, C.c_void_p(px.data_ptr()), st) == want
        assert sc.lib.mir_render_cams(sc.h, C.byref(cam), C.byref(vis), C.c_void_p(pos.data_ptr()), C.c_void_p(look.data_ptr()), None,
                                      C.c_void_p(px.data_ptr()), st) == want
        assert sc.lib.mir_render_outputs(sc.h, C.byref(cam), C.byref(vis), 0, None, None, None, None, C.byref(o), st) == want
        if want:
            assert b"flags" in sc.lib.mir_last_error()
    torch.cuda.synchronize()
    # a scene without round geoms accepts the flag and draws what it draws without it
    boxes = models.franka_cube_pick_scene(link_shape="box")
    sb = _stepped_scene(boxes, 2, steps=1)
    assert torch.equal(sb.render(cam, boxes.visual(round_geoms=True)), sb.render(cam, boxes.visual()))


def test_genesis_env_round_geoms():
    from gym_genesis.env import GenesisEnv

    B, H, W = 4, 96, 128
    envs = [GenesisEnv(task="cube_pick", robot="franka", num_envs=B, enable_pixels=True, observation_height=H, observation_width=W,
                       camera_capture_mode="per_env", round_geoms=r) for r in (False, True)]
    obs = [e.reset(seed=0)[0] for e in envs]
    act = np.random.RandomState(0).uniform(-1, 1, (3, B, 9)).astype(np.float32)
    for t in range(3):
        obs = [e.step(torch.as_tensor(act[t], device=obs[0]["pixels"].device))[0] for e in envs]
    frames = [e.render() for e in envs]
    assert frames[0] is not None and frames[1] is not None
    a, b = (o["pixels"].cpu().numpy() for o in obs)
    spec = envs[0]._env._builder.build()
    links = [g for g in range(spec.ngeom) if spec.geom[g].type == GEOM_CAPSULE]
    segs = [e.get_cams().render_batch(rgb=False, segmentation=True, segmentation_level="geom")[2].cpu().numpy() for e in envs]
    on_link = np.isin(segs[0], links) | np.isin(segs[1], links)
    diff = (a != b).any(-1)
    assert diff.any() and not (diff & ~on_link).any()
