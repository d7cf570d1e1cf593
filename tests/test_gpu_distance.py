"""Batched signed-distance queries on the GPU (include/mirigid.h: mir_signed_distance; tasks/views.py: get_clearance / in_collision;
tasks/sensors.py: Proximity).

States are SET (set_state), not stepped to, except in the call-changes-nothing test: the GPU, the float64 oracle and its float32 build
hold the same float32 bits.  B = 5 envs.  The cases -- scenes, seeds, probes -- are those of tests/dist_cases.py, whose share of
ambiguous probes tests/test_dist_cpu.py holds under 2 %.

Yardstick: tests/dist_ref.py evaluated in float32 on the link poses of the oracle's float32 build (the float32 port).  Per output the GPU
is allowed 4 x max(port error, 2^-23 x L): L = 1 for unit normals, and for distance and closest the largest absolute world coordinate
or distance in the float64 reference of the case; the metric is the max absolute error against the float64 reference over the
unambiguous probes.  Factor and floor are those of tests/test_gpu_raycast.py.  Every figure is printed before it is asserted.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import dist_cases
import dist_ref
from gym_genesis.backend.spec import MirDistQuery, make_dist_query
from gym_genesis.tasks import sensors

pytestmark = pytest.mark.gpu

B = dist_cases.B
OUTS = ("distance", "geom", "closest", "normal", "row_min", "row_argmin")
_scenes = {}


def _scene(name):
    if name not in _scenes:
        from gym_genesis.backend.lib import MirScene

        c = dist_cases.case(name)
        sc = MirScene(c["spec"], B)
        sc.set_state(qpos=c["q"], qvel=np.zeros((B, sc.nv), np.float32))
        _scenes[name] = sc
    return _scenes[name]


def _read(sc, c, **kw):
    args = dict(links=c["links"], max_distance=c["max_distance"], skip_geoms=c["skip"], geom=True, closest=True, normal=True, row_min=True)
    args.update(kw)
    return sc.signed_distance(c["probes"], **args)


def _scale(ref):
    """L of the yardstick's floor: the largest absolute world coordinate or distance in the float64 reference"""
    return float(max(np.abs(ref["closest"]).max(), np.abs(ref["centre"]).max(), np.abs(ref["distance"]).max()))


def _compare(label, got, ref, port):
    """geom ids equal on the unambiguous probes; distance, closest, normal within the yardstick rule -> ok mask"""
    got = {k: v.cpu().numpy() for k, v in got.items()}
    ok = ~ref["ambiguous"]
    assert got["distance"].shape == ref["distance"].shape and got["closest"].shape == ref["closest"].shape
    bad = (got["geom"] != ref["geom"]) & ok
    print(f"\n[signed distance, {label}] {ok.sum()} of {ok.size} probes unambiguous, {int((ref['geom'] >= 0).sum())} within max_distance, "
          f"{int(ref['inside'].sum())} inside a solid, {int(bad.sum())} geom ids differ")
    assert not bad.any(), (np.argwhere(bad)[:5], got["geom"][bad][:5], ref["geom"][bad][:5])
    same = ok & (port["geom"] == ref["geom"])
    L, fig = _scale(ref), {}
    for k in ("distance", "closest", "normal"):
        floor = 2.0 ** -23 * (1.0 if k == "normal" else L)
        sel = lambda m: np.broadcast_to(m if got[k].ndim == 2 else m[..., None], got[k].shape)  # noqa: E731
        yard = float(np.abs(port[k].astype(np.float64) - ref[k])[sel(same)].max())
        err = float(np.abs(got[k].astype(np.float64) - ref[k])[sel(ok)].max())
        fig[k] = (err, yard, 4.0 * max(yard, floor))
    print(f"    L = {L:.3f}   " + "   ".join(f"{k}: GPU {e:.3e} port {y:.3e} allowed {a:.3e}" for k, (e, y, a) in fig.items()))
    for k, (e, y, a) in fig.items():
        assert e <= a, (label, k, e, y, a)
    return got, ok


def _check(name, at="state", **kw):
    c, sc = dist_cases.case(name), _scene(name)
    if at == "candidate":
        kw["qpos"] = dist_cases.candidate(name)["q"]
    return _compare(f"{name}, {at}", _read(sc, c, **kw), dist_cases.reference(name, at), dist_cases.reference(name, at, np.float32)) + (dist_cases.reference(name, at),)


def test_every_geom_type():
    c = dist_cases.case("zoo")
    got, ok, ref = _check("zoo")
    types = np.array([g["type"] for g in c["dscene"].geoms])
    hit = ok & (got["geom"] >= 0)
    won = sorted(set(types[got["geom"][hit]].tolist()))
    inside = {int(t): int((hit & (got["distance"] < 0) & (types[np.maximum(got["geom"], 0)] == t) & ref["inside"]).sum()) for t in range(5)}
    print(f"    types that win: {won}; unambiguous interior probes with negative distance per type: {inside}")
    assert won == [0, 1, 2, 3, 4], "every geom type wins at least once"
    assert all(n >= 3 for n in inside.values()), inside
    miss = got["geom"] == -1
    assert miss.any() and (got["distance"][miss] == c["max_distance"]).all() and (got["normal"][miss] == 0).all()
    assert np.array_equal(got["closest"][miss], ref["centre"].astype(np.float32)[miss]) or np.abs(got["closest"][miss] - ref["centre"][miss]).max() < 4 * 2.0 ** -23 * _scale(ref)


@pytest.mark.parametrize("name", ["pick", "stack"])
def test_both_device_models(name):
    sc, c = _scene(name), dist_cases.case(name)
    assert sc.kernel == (16 if name == "pick" else 64)
    got, ok, ref = _check(name)
    assert (got["geom"] >= 0).mean() > 0.2
    assert not any((c["skip"] >> int(g)) & 1 for g in np.unique(got["geom"]) if g >= 0), "no geom of the arm is reported"


@pytest.mark.parametrize("name", ["pick", "stack", "zoo"])
def test_candidate_qpos(name):
    c, sc = dist_cases.case(name), _scene(name)
    # qpos = the current state: the in-kernel forward kinematics against the pose cache, within the yardstick's allowance
    cache = _read(sc, c)
    ref, port = dist_cases.reference(name), dist_cases.reference(name, "state", np.float32)
    state = [x.clone() for x in sc.get_state()]
    got, ok = _compare(f"{name}, qpos = the state", _read(sc, c, qpos=state[0]), ref, port)
    same = ok & (got["geom"] == cache["geom"].cpu().numpy())
    L = _scale(ref)
    for k in ("distance", "closest", "normal"):
        yard = float(np.abs(port[k].astype(np.float64) - ref[k])[np.broadcast_to(same if got[k].ndim == 2 else same[..., None], got[k].shape)].max())
        allowed = 4.0 * max(yard, 2.0 ** -23 * (1.0 if k == "normal" else L))
        diff = float(np.abs(got[k].astype(np.float64) - cache[k].cpu().numpy())[np.broadcast_to(same if got[k].ndim == 2 else same[..., None], got[k].shape)].max())
        print(f"    {k}: in-kernel FK against the pose cache {diff:.3e} allowed {allowed:.3e}")
        assert diff <= allowed, (name, k, diff, allowed)
    assert same.sum() >= ok.sum() - 2
    # a second configuration: the reference on the oracle's poses at that qpos; afterwards nothing has moved
    version = sc.state_version
    _check(name, "candidate")
    assert sc.state_version == version
    for x, y in zip(sc.get_state(), state):
        assert torch.equal(x, y)
    again = _read(sc, c)
    for k in OUTS:
        assert torch.equal(again[k], cache[k]), k
    if name == "zoo":
        return
    # get_clearance(qpos=...) in the entity's dof order equals the raw call on the scattered rows
    from gym_genesis.backend import models
    from gym_genesis.tasks.views import EntityView

    robot = EntityView(sc, c["sb"], "link0", models.FRANKA_JOINTS)
    cand = torch.as_tensor(dist_cases.candidate(name)["q"], device=sc.device)
    full = state[0].clone()
    full[:, robot._qcols] = cand[:, robot._qcols]
    n = c["n_arm"]
    raw = sc.signed_distance(c["probes"][:n], links=c["links"][:n], qpos=full, max_distance=1.0, skip_geoms=c["skip"], geom=True, closest=True, normal=True, row_min=True)
    det = robot.get_clearance(qpos=cand[:, robot._qcols], return_detail=True)
    assert torch.equal(det["clearance"], raw["row_min"]) and torch.equal(det["sphere"], raw["row_argmin"].long())
    rows = torch.arange(B, device=sc.device)
    assert torch.equal(det["geom"], raw["geom"][rows, det["sphere"]]) and torch.equal(det["closest"], raw["closest"][rows, det["sphere"]])
    assert torch.equal(robot.get_clearance(qpos=cand[:, robot._qcols]), raw["row_min"])
    idx = torch.tensor([3, 1], device=sc.device)
    assert torch.equal(robot.get_clearance(qpos=cand[idx][:, robot._qcols], envs_idx=idx), raw["row_min"][idx])


def test_addressing_and_tails():
    sc, c = _scene("zoo"), dist_cases.case("zoo")
    plain = _read(sc, c)
    assert (plain["geom"] >= 0).float().mean() > 0.2
    for idx in ([4, 3, 2, 1, 0], [2, 2, 0, 4, 2, 2, 1], [3]):
        rows = _read(sc, c, env_idx=torch.tensor(idx, device=sc.device))
        for k in OUTS:
            assert rows[k].shape[0] == len(idx) and torch.equal(rows[k], plain[k][idx]), (idx, k)
    # (probes 250 ..: world and riding probes side by side; every chunk boundary of the wave)
    lo = 250
    for n in (1, 7, 63, 64, 65, 130):
        part = sc.signed_distance(c["probes"][lo:lo + n], links=c["links"][lo:lo + n], max_distance=c["max_distance"], geom=True, closest=True, normal=True, row_min=True)
        for k in ("distance", "geom", "closest", "normal"):
            assert part[k].shape[1] == n and torch.equal(part[k], plain[k][:, lo:lo + n]), (n, k)
        m, a = part["distance"].min(1)
        first = (part["distance"] == m[:, None]).int().argmax(1)   # (the lower index on a tie)
        assert torch.equal(part["row_min"], m) and torch.equal(part["row_argmin"].long(), first), n
    m = plain["distance"].min(1).values
    assert torch.equal(plain["row_min"], m) and torch.equal(plain["row_argmin"].long(), (plain["distance"] == m[:, None]).int().argmax(1))
    # rows of misses
    tiny = _read(sc, dict(c, probes=c["probes"][:64] + np.array([0, 0, 5.0, 0], np.float32), links=None, max_distance=1e-3))
    assert (tiny["geom"] == -1).all() and (tiny["distance"] == 1e-3).all() and (tiny["normal"] == 0).all()
    assert (tiny["row_min"] == 1e-3).all() and (tiny["row_argmin"] == 0).all()
    assert torch.equal(tiny["closest"], torch.as_tensor(c["probes"][:64, :3] + np.array([0, 0, 5.0], np.float32), device=sc.device).expand(B, 64, 3))


def test_scene_view_point_query_and_proximity():
    """SceneView.signed_distance and sensors.Proximity are the raw call with their arguments in place"""
    from gym_genesis.tasks.views import SceneView

    sc, c = _scene("zoo"), dist_cases.case("zoo")
    view = SceneView(sc)
    w = slice(0, 7)   # (world probes)
    raw = sc.signed_distance(c["probes"][w], max_distance=0.8, geom=True, closest=True, normal=True)
    got = view.signed_distance(c["probes"][w, :3], radius=c["probes"][w, 3], max_distance=0.8, geom=True, closest=True, normal=True)
    assert sorted(got) == sorted(raw) and all(torch.equal(got[k], raw[k]) for k in raw)
    body = int(c["links"][300])
    raw = sc.signed_distance(c["probes"][300:301], links=c["links"][300:301], max_distance=0.8, closest=True, normal=True, env_idx=[4, 0])
    got = view.signed_distance(c["probes"][300, :3], radius=float(c["probes"][300, 3]), link=body, envs_idx=[4, 0], max_distance=0.8, closest=True, normal=True)
    assert all(torch.equal(got[k], raw[k]) for k in raw) and got["distance"].shape == (2, 1)
    prox = view.add_sensor(sensors.Proximity(link=body, pos_offset=tuple(c["probes"][300, :3]), radius=float(c["probes"][300, 3]), max_range=0.8, skip_own_entity=False))
    r = prox.read(envs_idx=[4, 0])
    assert torch.equal(r.distance, raw["distance"][:, 0]) and torch.equal(r.point, raw["closest"][:, 0]) and torch.equal(r.normal, raw["normal"][:, 0])
    own = view.add_sensor(sensors.Proximity(link=body, pos_offset=(0.0, 0.0, 0.0), max_range=0.8))
    assert own.skip_geoms == sum(1 << g for g, geom in enumerate(c["sb"].geoms) if geom["body"] == body), "its own body's geoms are skipped"
    seen = sc.signed_distance(np.zeros((1, 4), np.float32), links=[body], max_distance=0.8, skip_geoms=own.skip_geoms)["distance"][:, 0]
    assert torch.equal(own.read().distance, seen) and (seen > sc.signed_distance(np.zeros((1, 4), np.float32), links=[body])["distance"][:, 0]).all(), \
        "the probe sits inside its own geom and does not see it"


def _raw(sc, q, probes, links, idx, R, outs, qpos=None):
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    lk = None if links is None else np.ascontiguousarray(links, np.int32)
    rc = sc.lib.mir_signed_distance(sc.h, None if q is None else C.byref(q), p(probes), None if lk is None else lk.ctypes.data_as(C.c_void_p), p(idx), R, p(qpos),
                                    *[p(outs.get(k)) for k in OUTS], sc._stream())
    torch.cuda.synchronize()
    return rc, sc.lib.mir_last_error()


def test_nullable_outputs():
    sc, c = _scene("pick"), dist_cases.case("pick")
    full = _read(sc, c)
    N = len(c["probes"])
    probes = torch.as_tensor(c["probes"], device=sc.device)
    q = make_dist_query(N, c["max_distance"], c["skip"])
    shapes = {"distance": ((B, N), torch.float32), "geom": ((B, N), torch.int32), "closest": ((B, N, 3), torch.float32), "normal": ((B, N, 3), torch.float32),
              "row_min": ((B,), torch.float32), "row_argmin": ((B,), torch.int32)}
    for k in OUTS:
        one = torch.zeros(shapes[k][0], dtype=shapes[k][1], device=sc.device)
        rc, msg = _raw(sc, q, probes, c["links"], None, 0, {k: one})
        assert rc == 0 and torch.equal(one, full[k]), (k, msg)
    only = sc.signed_distance(c["probes"], links=c["links"], max_distance=c["max_distance"], skip_geoms=c["skip"])
    assert list(only) == ["distance"] and torch.equal(only["distance"], full["distance"])
    before = sc.state_version
    rc, _ = _raw(sc, q, probes, c["links"], None, 0, {})
    assert rc == 0 and sc.state_version == before, "all six NULL: MIR_OK"
    # (an EMPTY tensor's data_ptr() is NULL, which would mean "all envs": the row list is a real address, its length 0)
    idx = torch.zeros(1, dtype=torch.long, device=sc.device)
    nan = torch.full((B, N), float("nan"), device=sc.device)
    rc, _ = _raw(sc, q, probes, c["links"], idx, 0, {"distance": nan})
    assert rc == 0 and torch.isnan(nan).all(), "R == 0: MIR_OK, nothing written"


def test_clearance_tells_collision_from_free():
    from gym_genesis.backend import models
    from gym_genesis.tasks.views import EntityView

    c = dist_cases.case("pick")
    sb = c["sb"]
    from gym_genesis.backend.lib import MirScene

    sc = MirScene(c["spec"], B)
    robot, cube = EntityView(sc, sb, "link0", models.FRANKA_JOINTS), EntityView(sc, sb, "cube", ())
    hand = robot.get_link("hand")
    plane_geom = next(i for i, g in enumerate(sb.geoms) if g["type"] == 0)
    cube_geom = next(i for i, g in enumerate(sb.geoms) if g["body"] == sb.body_index("cube"))
    # configurations built here: the arm's reset pose, the cube where the scene puts it (on the floor, the table top of this scene)
    q0 = torch.zeros((B, sc.nq), device=sc.device)
    q0[:, robot._qcols] = torch.tensor(models.FRANKA_HOME, device=sc.device)
    cq = sc.spec.body[sb.body_index("cube")]
    qa = int(dist_cases.kin_ref.Model(c["spec"]).qadr[sb.body_index("cube")])
    q0[:, qa:qa + 7] = torch.tensor([*cq.pos, 1.0, 0.0, 0.0, 0.0], device=sc.device)
    sc.set_state(qpos=q0, qvel=torch.zeros((B, sc.nv), device=sc.device))
    free = robot.get_clearance()
    print(f"\n[clearance, pick] reset pose: {free.cpu().numpy()}")
    assert (free > 0).all() and not robot.in_collision().any()
    down = torch.tensor([0.0, 1.0, 0.0, 0.0], device=sc.device).expand(B, 4).contiguous()
    cube_pos = torch.tensor(list(cq.pos), device=sc.device)
    targets = {"below the table top": (torch.tensor([0.45, 0.0, -0.05], device=sc.device), plane_geom), "inside the cube": (cube_pos, cube_geom)}
    spheres, links = robot.collision_spheres()
    for label, (pos, want) in targets.items():
        qg = robot.inverse_kinematics(link=hand, pos=pos.expand(B, 3).contiguous(), quat=down)
        det = robot.get_clearance(qpos=qg, return_detail=True)
        flag = robot.in_collision(qpos=qg)
        # the same spheres through dist_ref, on the oracle's poses at that configuration
        full = q0.clone()
        full[:, robot._qcols] = qg
        xp, xq = dist_cases.ray_cases.poses(c["spec"], full.cpu().numpy())
        ref = dist_ref.signed_distance(c["dscene"], xp, xq, spheres, links, 1.0, robot._own_geoms(), with_ambiguous=False)
        print(f"[clearance, pick] hand {label}: GPU {det['clearance'].cpu().numpy()} geom {det['geom'].cpu().numpy()}  reference {ref['row_min']}")
        assert flag.all() and (det["clearance"] < 0).all() and (ref["row_min"] < 0).all()
        # (the deepest sphere may be a finger's against the floor when the hand is in the cube: the cube must be hit by the model)
        hits = robot.get_clearance(qpos=qg, with_entity=cube if want == cube_geom else None, return_detail=True)
        assert (hits["geom"] == want).all(), (label, hits["geom"])
        assert (hits["clearance"] < 0).all()
    assert np.sign(free.cpu().numpy()).tolist() == np.sign(dist_ref.signed_distance(
        c["dscene"], *dist_cases.ray_cases.poses(c["spec"], q0.cpu().numpy()), spheres, links, 1.0, robot._own_geoms(), with_ambiguous=False)["row_min"]).tolist()
    sc.close()


def test_a_call_changes_nothing():
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
    robot = tasks[0].franka
    prox = tasks[0].scene.add_sensor(sensors.Proximity(link=robot.get_link("hand"), pos_offset=(0.0, 0.0, 0.1), radius=0.01, max_range=2.0))
    assert prox.skip_geoms
    A = torch.as_tensor(acts, device=mirs[0].device)
    v0 = [m.state_version for m in mirs]
    qc = robot.get_qpos().clone()
    for t in range(50):
        res = [e.step(A[8 * t % acts.shape[0]]) for e in envs]
        r = prox.read()
        clear = robot.get_clearance(qpos=qc) if t % 2 else robot.get_clearance()
        for k in ("agent_pos", "environment_state"):
            assert torch.equal(res[0][0][k], res[1][0][k]), (t, k)
        assert torch.equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])
        for x, y in zip(mirs[0].get_state(), mirs[1].get_state()):   # qpos, qvel, targets, warm start
            assert torch.equal(x, y), t
        for x, y in zip(mirs[0].get_diag(points=True), mirs[1].get_diag(points=True)):
            assert torch.equal(x, y), t
        assert mirs[0].state_version - v0[0] == mirs[1].state_version - v0[1]
    assert torch.isfinite(r.distance).all() and float(r.distance.min()) < 2.0 and torch.isfinite(clear).all()
    assert (torch.linalg.norm(r.normal, dim=1) - 1).abs().max() < 1e-5
    assert mirs[0].distance_launches == 100
    # ... and between two device-resident rollouts that keep every contact point
    K = 4
    stride = mirs[0].agent_dim + mirs[0].env_dim + 2
    rows = [torch.zeros((K, n, stride), device=m.device) for m in mirs]
    for call in range(2):
        a = A[100 + K * call:100 + K * (call + 1)].contiguous()
        for m, r_ in zip(mirs, rows):
            m.rollout_exact(a, r_)
        prox.read()
        robot.get_clearance(qpos=qc)
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
    probes = torch.as_tensor(dist_cases.case("pick")["probes"][:8], device=sc.device)
    links = np.zeros(8, np.int32)
    dist = torch.full((B, 8), float("nan"), device=sc.device)
    before, launches = sc.state_version, sc.__dict__.get("distance_launches", 0)
    good = lambda **kw: make_dist_query(8, **kw)  # noqa: E731
    assert _raw(sc, good(), probes, links, None, 0, {"distance": dist})[0] == 0 and torch.isfinite(dist).all()
    dist.fill_(float("nan"))
    bad = [_raw(sc, None, probes, links, None, 0, {"distance": dist}), _raw(sc, good(), None, links, None, 0, {"distance": dist})]
    h, sc.h = sc.h, C.c_void_p(0)
    try:
        bad.append(_raw(sc, good(), probes, links, None, 0, {"distance": dist}))
    finally:
        sc.h = h
    q = good(); q.struct_size -= 8; bad.append(_raw(sc, q, probes, links, None, 0, {"distance": dist}))
    q = good(); q.n_probes = 0; bad.append(_raw(sc, q, probes, links, None, 0, {"distance": dist}))
    for md in (0.0, -1.0, float("inf"), float("nan")):
        bad.append(_raw(sc, good(max_distance=md), probes, links, None, 0, {"distance": dist}))
    q = good(); q.flags = 1; bad.append(_raw(sc, q, probes, links, None, 0, {"distance": dist}))
    bad.append(_raw(sc, good(skip_geoms=1 << ngeom), probes, links, None, 0, {"distance": dist}))
    bad.append(_raw(sc, good(skip_geoms=1 << 63), probes, links, None, 0, {"distance": dist}))
    for link in (-1, nbody):
        lk = links.copy(); lk[5] = link
        bad.append(_raw(sc, good(), probes, lk, None, 0, {"distance": dist}))
    for rc, msg in bad:
        assert rc == -1 and b"mir_signed_distance" in msg, (rc, msg)
    assert sc.state_version == before
    # capacity: more probes than a call takes; R x N beyond 2^31 - 1 (nothing is read: nothing is launched)
    idx = torch.zeros(1, dtype=torch.long, device=sc.device)
    q = good(); q.n_probes = S.DIST_MAX_PROBES + 1
    rc, msg = _raw(sc, q, probes, None, None, 0, {"distance": dist})
    assert rc == -2 and b"mir_signed_distance" in msg
    q = good(); q.n_probes = 1024
    rc, msg = _raw(sc, q, probes, None, idx, 1 << 22, {"distance": dist})
    assert rc == -2 and b"mir_signed_distance" in msg
    # between mir_step_begin and mir_step_end
    bufs = (sc.empty(sc.agent_dim), sc.empty(sc.env_dim), sc.empty(), sc.empty(dtype=torch.uint8))
    state = [x.clone() for x in sc.get_state()]
    sc.step_begin(None, *bufs)
    rc, msg = _raw(sc, good(), probes, links, None, 0, {"distance": dist})
    sc.step_end()
    assert rc == -1 and b"mir_signed_distance" in msg and b"pending" in msg
    sc.set_state(*state)   # (the shared scene goes back to the state the other tests compare)
    assert torch.isnan(dist).all(), "a refused call launches nothing"
    with pytest.raises(MirError):
        sc.signed_distance(probes, links=np.full(8, nbody, np.int32))
    assert sc.__dict__.get("distance_launches", 0) == launches
    assert C.sizeof(MirDistQuery) == sc.lib.mir_dist_query_sizeof()
    # a hull without volume: four vertices in one plane
    sb = S.SceneBuilder()
    sb.add_geom(0, S.GEOM_PLANE)
    sb.add_body("flat", 0, pos=(0.0, 0.0, 0.5), jtype=S.JNT_FREE, mass=0.3, inertia=S.sphere_inertia(0.3, 0.1))
    sb.add_geom("flat", S.GEOM_HULL, vertices=[(0.1, 0.1, 0.0), (-0.1, 0.1, 0.0), (-0.1, -0.1, 0.0), (0.1, -0.1, 0.0)])
    sb.task = dict(eef_body=1, obj_body=1, grip_dof=(), reward_z=0.1)
    try:
        flat = MirScene(sb.build(), 2)
    except MirError as e:   # (a scene compiler that refuses the flat hull itself leaves mir_signed_distance nothing to refuse)
        assert "hull" in str(e)
    else:
        out = torch.full((2, 8), float("nan"), device=flat.device)
        for _ in range(2):   # (the verdict is kept: the second call fails the same way)
            rc, msg = _raw(flat, good(), probes, links, None, 0, {"distance": out})
            assert rc == -1 and b"mir_signed_distance" in msg and b"volume" in msg, (rc, msg)
        assert torch.isnan(out).all()
