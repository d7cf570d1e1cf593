"""Batched ray-cast range sensing on the GPU (include/mirigid.h: mir_raycast; tasks/sensors.py: Lidar / Raycaster / DepthCamera).

States are SET (set_state), not stepped to, except in the read-changes-nothing test: the GPU, the float64 oracle and its float32 build
hold the same float32 bits.  B = 5 envs.  The cases -- scenes, seeds, sensors, rays -- are those of tests/ray_cases.py, whose share of
ambiguous rays tests/test_ray_cpu.py holds under 2 %.

Yardstick: tests/ray_ref.py evaluated in float32 on the link poses of the oracle's float32 build (the float32 port).  Per output the GPU
is allowed 4 x max(port error, 2^-23 x max_range) on distance and points and 4 x max(port error, 2^-23) on unit normals; the metric is
the max absolute error against the float64 reference over the unambiguous rays.  Every figure is printed before it is asserted.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import ray_cases
import ray_ref
import round_caster
from gym_genesis.backend.spec import MirRayQuery, make_camera, make_ray_query
from gym_genesis.tasks import sensors

pytestmark = pytest.mark.gpu

B = ray_cases.B
OUTS = ("distance", "points", "geom", "normal")
_scenes = {}


def _scene(name):
    if name not in _scenes:
        from gym_genesis.backend.lib import MirScene

        c = ray_cases.case(name)
        sc = MirScene(c["spec"], B)
        sc.set_state(qpos=c["q"], qvel=np.zeros((B, sc.nv), np.float32))
        _scenes[name] = sc
    return _scenes[name]


def _read(sc, s, world_frame=False, **kw):
    return sc.raycast(s["dirs"], link=s["link"], pos_offset=s["pos_offset"], quat_offset=s["quat_offset"], min_range=s["min_range"],
                      max_range=s["max_range"], skip_geoms=s["skip"], world_frame=world_frame, geom=True, normal=True, **kw)


def _check(name, si, world_frame):
    """geom ids equal on the unambiguous rays; distance, points, normal within the yardstick rule -> the figures"""
    c, sc = ray_cases.case(name), _scene(name)
    s = c["sensors"][si]
    ref, port = ray_cases.reference(name, si, world_frame), ray_cases.reference(name, si, world_frame, np.float32)
    got = {k: v.cpu().numpy() for k, v in _read(sc, s, world_frame).items()}
    ok = ~ref["ambiguous"]
    assert got["distance"].shape == ref["distance"].shape and got["points"].shape == ref["points"].shape
    bad = (got["geom"] != ref["geom"]) & ok
    print(f"\n[raycast, {name}, {s['label']}, {'world' if world_frame else 'sensor'} frame] {ok.sum()} of {ok.size} rays unambiguous, "
          f"{int((ref['geom'] >= 0).sum())} hits, {int(bad.sum())} geom ids differ")
    assert not bad.any(), (np.argwhere(bad)[:5], got["geom"][bad][:5], ref["geom"][bad][:5])
    same = ok & (port["geom"] == ref["geom"])
    fig = {}
    for k in ("distance", "points", "normal"):
        floor = 2.0 ** -23 * (1.0 if k == "normal" else s["max_range"])
        m = same if got[k].ndim == 2 else same[..., None]
        yard = float(np.abs(port[k].astype(np.float64) - ref[k])[np.broadcast_to(m, got[k].shape)].max())
        err = float(np.abs(got[k].astype(np.float64) - ref[k])[np.broadcast_to(ok if got[k].ndim == 2 else ok[..., None], got[k].shape)].max())
        fig[k] = (err, yard, 4.0 * max(yard, floor))
    print("    " + "   ".join(f"{k}: GPU {e:.3e} port {y:.3e} allowed {a:.3e}" for k, (e, y, a) in fig.items()))
    for k, (e, y, a) in fig.items():
        assert e <= a, (name, s["label"], k, e, y, a)
    return got, ref, ok


@pytest.mark.parametrize("world_frame", [False, True])
def test_every_geom_type(world_frame):
    c = ray_cases.case("zoo")
    for si in range(len(c["sensors"])):
        got, ref, ok = _check("zoo", si, world_frame)
        if si == 0:
            assert set(range(6)) <= set(np.unique(got["geom"][ok]).tolist()), "the world sensor sees every geom type"
            zero = np.all(c["sensors"][0]["dirs"] == 0, axis=1)
            assert zero.sum() == 1 and (got["geom"][:, zero] == -1).all() and (got["normal"][:, zero] == 0).all() and (got["distance"][:, zero] == 6.0).all()
        if si == 2:
            assert (got["distance"] <= 1.0).all() and (got["geom"][got["distance"] == 1.0] == -1).all(), "max_range shorter than a hit"
        if si == 3:
            near = ok & (ref["t"] < 3.0)
            assert near.sum() > 50 and (got["distance"][near] == 3.0).all() and (got["geom"][near] >= 0).all(), "min_range longer than a hit"
    # hulls are their polytopes, not their bounding boxes: where the float64 reference of the boxed scene differs, the GPU is not the box
    s = c["sensors"][0]
    boxed = ray_ref.Scene(c["spec"])
    for g in boxed.geoms:
        if g["type"] == ray_ref.HULL:
            v0, nv = int(g["size"][0]), int(g["size"][1])
            g["type"], g["size"], g["planes"] = ray_ref.BOX, np.abs(np.array([[c["spec"].vert[i][k] for k in range(3)] for i in range(v0, v0 + nv)])).max(0), None
    box = ray_ref.raycast(boxed, c["xp"], c["xq"], s["link"], s["pos_offset"], s["quat_offset"], s["dirs"], 0.0, 6.0, with_ambiguous=False)
    got, ref, ok = _check("zoo", 0, world_frame)
    differs = ok & (ref["geom"] == 5) & (np.abs(box["distance"] - ref["distance"]) > 1e-3)
    print(f"    {int(differs.sum())} rays on the icosphere hull where the bounding box is more than 1 mm off")
    assert differs.sum() >= 1 and (np.abs(got["distance"] - box["distance"])[differs] > 5e-4).all()


@pytest.mark.parametrize("name", ["pick", "stack"])
def test_both_device_models(name):
    sc = _scene(name)
    assert sc.kernel == (16 if name == "pick" else 64)
    for si in range(2):
        for wf in (False, True):
            got, ref, ok = _check(name, si, wf)
        assert (got["geom"] >= 0).mean() > 0.2
    own = ray_cases.case(name)["sensors"][0]["skip"]
    lidar = _read(sc, ray_cases.case(name)["sensors"][0])["geom"].cpu().numpy()
    assert not any((own >> int(g)) & 1 for g in np.unique(lidar) if g >= 0), "skip_own_entity: no geom of the arm is reported"


def _raw(sc, q, dirs, idx, R, outs):
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    rc = sc.lib.mir_raycast(sc.h, None if q is None else C.byref(q), p(dirs), p(idx), R, p(outs.get("distance")), p(outs.get("points")), p(outs.get("geom")),
                            p(outs.get("normal")), sc._stream())
    torch.cuda.synchronize()
    return rc, sc.lib.mir_last_error()


def _dirs260():
    d = np.random.default_rng(41).normal(size=(260, 3)).astype(np.float32)
    d[:, 2] -= 0.5
    return d


def test_addressing_and_tails():
    sc = _scene("zoo")
    s = dict(ray_cases.case("zoo")["sensors"][1], dirs=_dirs260())
    plain = _read(sc, s)
    assert (plain["geom"] >= 0).float().mean() > 0.2
    for idx in ([4, 3, 2, 1, 0], [2, 2, 0, 4, 2, 2, 1], [3]):
        rows = _read(sc, s, env_idx=torch.tensor(idx, device=sc.device))
        for k in OUTS:
            assert rows[k].shape[0] == len(idx) and torch.equal(rows[k], plain[k][idx]), (idx, k)
    for n in (1, 7, 257, 260):
        part = _read(sc, dict(s, dirs=s["dirs"][:n]))
        for k in OUTS:
            assert part[k].shape[1] == n and torch.equal(part[k], plain[k][:, :n]), (n, k)
    # outputs that start one float past a 16-byte boundary (and N = 7: every row starts at another phase)
    for n in (260, 7):
        d = torch.as_tensor(s["dirs"][:n], device=sc.device)
        q = make_ray_query(n, s["link"], s["pos_offset"], s["quat_offset"], s["min_range"], s["max_range"], s["skip"])
        flat = {k: torch.full((B * n * (3 if k in ("points", "normal") else 1) + 1,), -7.0, device=sc.device) for k in ("distance", "points", "normal")}
        assert all(t.data_ptr() % 16 == 0 for t in flat.values())
        rc, _ = _raw(sc, q, d, None, 0, {k: t[1:] for k, t in flat.items()})
        assert rc == 0
        for k, t in flat.items():
            assert float(t[0]) == -7.0 and torch.equal(t[1:].reshape(plain[k][:, :n].shape), plain[k][:, :n]), (n, k)


def test_nullable_outputs():
    sc = _scene("pick")
    s = ray_cases.case("pick")["sensors"][0]
    full = _read(sc, s)
    kw = dict(link=s["link"], pos_offset=s["pos_offset"], quat_offset=s["quat_offset"], max_range=s["max_range"], skip_geoms=s["skip"])
    for k in OUTS:
        one = sc.raycast(s["dirs"], **kw, **{o: o == k for o in OUTS})
        assert list(one) == [k] and torch.equal(one[k], full[k]), k
    before = sc.state_version
    rc, _ = _raw(sc, make_ray_query(len(s["dirs"]), s["link"]), torch.as_tensor(s["dirs"], device=sc.device), None, 0, {})
    assert rc == 0 and sc.state_version == before, "all four NULL: MIR_OK"
    # (an EMPTY tensor's data_ptr() is NULL, which would mean "all envs": the row list is a real address, its length 0; the output is
    #  large enough for a full call all the same)
    idx = torch.zeros(1, dtype=torch.long, device=sc.device)
    nan = torch.full((B, len(s["dirs"])), float("nan"), device=sc.device)
    rc, _ = _raw(sc, make_ray_query(len(s["dirs"]), s["link"]), torch.as_tensor(s["dirs"], device=sc.device), idx, 0, {"distance": nan})
    assert rc == 0 and torch.isnan(nan).all(), "R == 0: MIR_OK, nothing written"


def test_against_the_rasteriser():
    """cam.render(depth=True) with round_geoms and DepthCamera.read_image() of the same camera pose, both against the float64 reference's
    planar depth, on pixels whose 3 x 3 neighbourhood has one segmentation id"""
    from gym_genesis.tasks.views import SceneView

    c, sc = ray_cases.case("pick"), _scene("pick")
    s = c["sensors"][1]
    pat = sensors.DepthCameraPattern((16, 12), 50.0)
    pos, look = s["pos_offset"], (0.3, 0.0, 0.2)
    assert np.allclose(s["quat_offset"], sensors.lookat_quat(pos, look))
    sensor = SceneView(sc).add_sensor(sensors.DepthCamera(pattern=pat, pos_offset=pos, quat_offset=s["quat_offset"], max_range=s["max_range"]))
    img = sensor.read_image().cpu().numpy()
    _, depth, seg, _ = sc.render_outputs(make_camera(16, 12, pos, look, 50.0), c["sb"].visual(round_geoms=True), mode=0, rgb=False, depth=True,
                                         segmentation=True, seg_level="geom")
    depth, seg = depth.cpu().numpy(), seg.cpu().numpy()
    ref, port = ray_cases.reference("pick", 1), ray_cases.reference("pick", 1, False, np.float32)
    cosine = s["dirs"].astype(np.float64)[:, 0]
    truth = (ref["distance"] * cosine[None]).reshape(B, 12, 16)
    yard = np.abs((port["distance"] * s["dirs"][:, 0][None]).astype(np.float64).reshape(B, 12, 16) - truth)
    ok = (~ref["ambiguous"] & (ref["geom"] >= 0) & (port["geom"] == ref["geom"])).reshape(B, 12, 16)
    for e in range(B):
        ok[e] &= ~round_caster.silhouette(seg[e]) & (seg[e] == ref["geom"][e].reshape(12, 16))
    allowed = 4.0 * max(float(yard[ok].max()), 2.0 ** -23 * s["max_range"])
    e_r, e_s = float(np.abs(depth - truth)[ok].max()), float(np.abs(img - truth)[ok].max())
    print(f"\n[raycast vs rasteriser, pick, {ok.sum()} of {ok.size} pixels] planar depth: rasteriser {e_r:.3e} sensor {e_s:.3e} port {float(yard[ok].max()):.3e} allowed {allowed:.3e}")
    assert ok.sum() > 0.6 * ok.size
    assert e_s <= allowed and e_r <= allowed


def test_a_read_changes_nothing():
    import test_gpu_contact_forces as cf
    from gym_genesis.env import GenesisEnv

    n = 8
    _, acts = cf._grasp(n)
    envs = [GenesisEnv(task="cube_pick", robot="franka", num_envs=n, enable_pixels=False) for _ in range(2)]
    for e in envs:
        e.reset(seed=3)
    tasks = [e._env for e in envs]
    mirs = [t._mir for t in tasks]
    for m in mirs:
        m.set_diag(True)
    lidar = tasks[0].scene.add_sensor(sensors.Lidar(pattern=sensors.SphericalPattern((360.0, 60.0), (32, 8)), link=tasks[0].franka.get_link("hand"), max_range=5.0))
    assert lidar.skip_geoms
    A = torch.as_tensor(acts, device=mirs[0].device)
    v0 = [m.state_version for m in mirs]
    for t in range(50):
        res = [e.step(A[8 * t % acts.shape[0]]) for e in envs]
        r = lidar.read(geoms=(t % 2 == 0), normals=(t % 3 == 0))
        for k in ("agent_pos", "environment_state"):
            assert torch.equal(res[0][0][k], res[1][0][k]), (t, k)
        assert torch.equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])
        for x, y in zip(mirs[0].get_state(), mirs[1].get_state()):   # qpos, qvel, targets, warm start
            assert torch.equal(x, y), t
        for x, y in zip(mirs[0].get_diag(points=True), mirs[1].get_diag(points=True)):
            assert torch.equal(x, y), t
        assert mirs[0].state_version - v0[0] == mirs[1].state_version - v0[1]
    assert torch.isfinite(r.distances).all() and float(r.distances.min()) < 5.0
    assert mirs[0].raycast_launches == 50
    # ... and between two device-resident rollouts that keep every contact point
    K = 4
    stride = mirs[0].agent_dim + mirs[0].env_dim + 2
    rows = [torch.zeros((K, n, stride), device=m.device) for m in mirs]
    for call in range(2):
        a = A[100 + K * call:100 + K * (call + 1)].contiguous()
        for m, r_ in zip(mirs, rows):
            m.rollout_exact(a, r_)
        lidar.read()
        assert torch.equal(rows[0], rows[1]), call
        for x, y in zip(mirs[0].get_state(), mirs[1].get_state()):
            assert torch.equal(x, y), call
        for x, y in zip(mirs[0].get_diag(points=True), mirs[1].get_diag(points=True)):
            assert torch.equal(x, y), call
        assert mirs[0].state_version - v0[0] == mirs[1].state_version - v0[1]


def test_refusals_launch_nothing():
    from gym_genesis.backend import spec as S
    from gym_genesis.backend.lib import MirError, MirScene

    sc = _scene("pick")
    nbody, ngeom = sc.nbody, sc.ngeom
    d = torch.as_tensor(_dirs260()[:8], device=sc.device)
    dist = torch.full((B, 8), float("nan"), device=sc.device)
    before, launches = sc.state_version, sc.__dict__.get("raycast_launches", 0)
    good = lambda **kw: make_ray_query(8, **kw)  # noqa: E731
    assert _raw(sc, good(), d, None, 0, {"distance": dist})[0] == 0 and torch.isfinite(dist).all()
    dist.fill_(float("nan"))
    bad = [_raw(sc, None, d, None, 0, {"distance": dist}), _raw(sc, good(), None, None, 0, {"distance": dist})]
    h, sc.h = sc.h, C.c_void_p(0)
    try:
        bad.append(_raw(sc, good(), d, None, 0, {"distance": dist}))
    finally:
        sc.h = h
    q = good(); q.struct_size -= 8; bad.append(_raw(sc, q, d, None, 0, {"distance": dist}))
    q = good(); q.n_rays = 0; bad.append(_raw(sc, q, d, None, 0, {"distance": dist}))
    for link in (-1, nbody):
        bad.append(_raw(sc, good(link=link), d, None, 0, {"distance": dist}))
    for lo, hi in ((-0.1, 1.0), (1.0, 1.0), (2.0, 1.0), (0.0, float("inf")), (float("nan"), 1.0), (0.0, float("nan"))):
        bad.append(_raw(sc, good(min_range=lo, max_range=hi), d, None, 0, {"distance": dist}))
    q = good(); q.flags = 2; bad.append(_raw(sc, q, d, None, 0, {"distance": dist}))
    bad.append(_raw(sc, good(skip_geoms=1 << ngeom), d, None, 0, {"distance": dist}))
    bad.append(_raw(sc, good(skip_geoms=1 << 63), d, None, 0, {"distance": dist}))
    for rc, msg in bad:
        assert rc == -1 and b"mir_raycast" in msg, (rc, msg)
    assert sc.state_version == before
    # capacity: R x N beyond 2^31 - 1 (nothing is read: nothing is launched)
    q = good(); q.n_rays = 1 << 16
    idx = torch.zeros(1, dtype=torch.long, device=sc.device)
    rc, msg = _raw(sc, q, d, idx, 1 << 15, {"distance": dist})
    assert rc == -2 and b"mir_raycast" in msg
    # between mir_step_begin and mir_step_end
    bufs = (sc.empty(sc.agent_dim), sc.empty(sc.env_dim), sc.empty(), sc.empty(dtype=torch.uint8))
    state = [x.clone() for x in sc.get_state()]
    sc.step_begin(None, *bufs)
    rc, msg = _raw(sc, good(), d, None, 0, {"distance": dist})
    sc.step_end()
    assert rc == -1 and b"mir_raycast" in msg and b"pending" in msg
    sc.set_state(*state)   # (the shared scene goes back to the state the other tests compare)
    assert torch.isnan(dist).all(), "a refused call launches nothing"
    assert sc.__dict__.get("raycast_launches", 0) == launches
    assert C.sizeof(MirRayQuery) == sc.lib.mir_ray_query_sizeof()
    # a hull without volume: four vertices in one plane
    sb = S.SceneBuilder()
    sb.add_geom(0, S.GEOM_PLANE)
    sb.add_body("flat", 0, pos=(0.0, 0.0, 0.5), jtype=S.JNT_FREE, mass=0.3, inertia=S.sphere_inertia(0.3, 0.1))
    sb.add_geom("flat", S.GEOM_HULL, vertices=[(0.1, 0.1, 0.0), (-0.1, 0.1, 0.0), (-0.1, -0.1, 0.0), (0.1, -0.1, 0.0)])
    sb.task = dict(eef_body=1, obj_body=1, grip_dof=(), reward_z=0.1)
    try:
        flat = MirScene(sb.build(), 2)
    except MirError as e:   # (a scene compiler that refuses the flat hull itself leaves mir_raycast nothing to refuse)
        assert "hull" in str(e)
    else:
        out = torch.full((2, 8), float("nan"), device=flat.device)
        for _ in range(2):   # (the verdict is kept: the second call fails the same way)
            rc, msg = _raw(flat, good(), d, None, 0, {"distance": out})
            assert rc == -1 and b"mir_raycast" in msg and b"volume" in msg, (rc, msg)
        assert torch.isnan(out).all()
