"""The scenes, seeds, sensors and ray sets of the range-sensing tests, shared by tests/test_ray_cpu.py (which holds the share of
ambiguous rays of every case under 2 %) and tests/test_gpu_raycast.py.  A helper, no test.  States are seeded and SET, never simulated.
"""
from __future__ import annotations

import functools

import numpy as np

import kin_ref
import orc
import ray_ref
from gym_genesis.backend import models
from gym_genesis.backend import spec as S
from gym_genesis.tasks import sensors

B = 5
ZOO_BOX, ZOO_HULL_BOX = (0.15, 0.1, 0.2), (0.12, 0.18, 0.1)
ZOO_SPHERE_R, ZOO_CAPSULE, ZOO_BALL_R = 0.15, (0.08, 0.2), 0.15
ZOO_BODIES = ("box", "sphere", "capsule", "hullbox", "ball")
WORLD_SENSOR_POS = (0.35, 0.17, 2.2)


def zoo_builder():
    """a plane and, on free bodies, a box, a sphere, a capsule, a box given as a hull and a 32-vertex icosphere hull"""
    sb = S.SceneBuilder()
    sb.add_geom(0, S.GEOM_PLANE)
    kinds = (("box", S.GEOM_BOX, ZOO_BOX, None), ("sphere", S.GEOM_SPHERE, (ZOO_SPHERE_R, 0.0, 0.0), None),
             ("capsule", S.GEOM_CAPSULE, ZOO_CAPSULE + (0.0,), None), ("hullbox", S.GEOM_HULL, None, S.box_hull_vertices(ZOO_HULL_BOX)),
             ("ball", S.GEOM_HULL, None, S.icosphere_vertices(ZOO_BALL_R, 1)))
    for i, (name, t, size, verts) in enumerate(kinds):
        sb.add_body(name, 0, pos=(0.4 * i - 0.8, 0.0, 0.6), jtype=S.JNT_FREE, mass=0.3, inertia=S.sphere_inertia(0.3, 0.1))
        if verts is None:
            sb.add_geom(name, t, size=size)
        else:
            sb.add_geom(name, t, vertices=verts)
    sb.task = dict(eef_body=1, obj_body=2, grip_dof=(), reward_z=0.1)
    sb.opt["max_contacts"] = 48
    return sb


def builder(name):
    return {"zoo": zoo_builder, "pick": models.franka_cube_pick_scene, "stack": models.franka_cube_stack_scene}[name]()


SEEDS = {"zoo": 31, "pick": 32, "stack": 33}


def state(name, spec):
    """qpos (B, nq) float32: joints inside their ranges, free bodies at random poses; env 0 of the zoo has its box unrotated under the
    world sensor (rays parallel to its faces with exact zero components)"""
    model = kin_ref.Model(spec)
    box = ((-0.7, -0.7, 0.45), (0.7, 0.7, 1.3)) if name == "zoo" else ((-0.3, -0.3, 0.05), (0.7, 0.3, 0.9))
    q, _ = kin_ref.random_state(spec, model, B, seed=SEEDS[name], cube_box=box)
    if name == "zoo":
        q[0, 0:7] = (0.3, 0.2, 0.5, 1.0, 0.0, 0.0, 0.0)
    return q


def poses(spec, q, f32=False):
    o = orc.Oracle(spec, q.shape[0], f32=f32) if f32 else orc.Oracle(spec, q.shape[0])
    o.write_all(orc.F_QPOS, q.astype(np.float64))
    return ray_ref.oracle_poses(o)


def _aimed(scene, xp, xq, link, pos_offset, quat_offset, max_range):
    """hand-aimed rays for env 0, sensor frame: the axis-parallel directions (zero components), the x axis of the first box (parallel to
    four of its faces), the centre of every geom, and a miss beside every geom by 1e-2 rad (its silhouette edge found by bisection on
    the reference with every other geom skipped), a zero direction"""
    base = ray_ref.raycast_env(scene, xp, xq, link, pos_offset, quat_offset, np.array([[1.0, 0, 0]]), 0.0, max_range, with_ambiguous=False)
    origin, Rs = base["origin"], base["Rs"]
    rays = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, 1, 0), (0, -1, -1), (0, 0, 0)]
    for gi, g in enumerate(scene.geoms):
        if g["type"] == ray_ref.PLANE:
            continue
        c = xp[g["body"]] + ray_ref.qmat(xq[g["body"]]) @ g["pos"]
        Rg = ray_ref.qmat(ray_ref.qmul(xq[g["body"]], g["quat"]))
        to = (c - origin) / np.linalg.norm(c - origin)
        if g["type"] == ray_ref.BOX:
            rays.append(tuple(Rs.T @ Rg[:, 0]))
        rays.append(tuple(Rs.T @ to))
        perp = np.cross(to, [0.3, -0.5, 0.8])
        perp /= np.linalg.norm(perp)
        only = ((1 << scene.ngeom) - 1) & ~(1 << gi)
        hits = lambda a: ray_ref.raycast_env(scene, xp, xq, link, pos_offset, quat_offset, [Rs.T @ (np.cos(a) * to + np.sin(a) * perp)], 0.0, 1e9,  # noqa: E731
                                             skip_geoms=only, with_ambiguous=False)["geom"][0] >= 0
        if not hits(0.0):
            continue  # (the origin is inside this geom)
        lo, hi = 0.0, 1.5
        for _ in range(40):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if hits(mid) else (lo, mid)
        a = hi + 1e-2
        rays.append(tuple(Rs.T @ (np.cos(a) * to + np.sin(a) * perp)))
    return np.array(rays, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(sb, spec, scene, q, xp, xq (float64 oracle poses), xp32, xq32 (the float32 oracle's), sensors=[dict(...)])
    each sensor: link, pos_offset, quat_offset, dirs (N, 3) float32, shape, min_range, max_range, skip, label"""
    sb = builder(name)
    spec = sb.build()
    scene = ray_ref.Scene(spec)
    q = state(name, spec)
    xp, xq = poses(spec, q)
    xp32, xq32 = poses(spec, q, f32=True if name == "pick" else "big")
    out = dict(sb=sb, spec=spec, scene=scene, q=q, xp=xp, xq=xq, xp32=xp32, xq32=xq32, sensors=[])

    def add(label, link, pos_offset, quat_offset, dirs, shape, min_range, max_range, skip=0):
        out["sensors"].append(dict(label=label, link=link, pos_offset=tuple(pos_offset), quat_offset=tuple(quat_offset),
                                   dirs=np.ascontiguousarray(dirs, dtype=np.float32), shape=shape, min_range=min_range, max_range=max_range, skip=skip))

    if name == "zoo":
        grid = sensors.GridPattern(resolution=0.2, size=(1.4, 1.4))
        assert grid.shape == (8, 8)
        ident = (1.0, 0.0, 0.0, 0.0)
        rq = sensors.euler_to_quat((30.0, 20.0, -40.0))
        rider, rpos = sb.body_index("sphere"), (0.05, -0.02, 0.03)   # (inside its own sphere: the sphere is not seen)
        for label, link, po, qo in (("world", 0, WORLD_SENSOR_POS, ident), ("rider", rider, rpos, rq)):
            aimed = _aimed(scene, xp[0], xq[0], link, po, qo, 6.0)
            dirs = np.concatenate([grid.directions().astype(np.float64), aimed])
            add(label, link, po, qo, dirs, None, 0.0, 6.0)
        w = out["sensors"][0]
        add("world, max_range shorter than a hit", 0, WORLD_SENSOR_POS, ident, w["dirs"], None, 0.0, 1.0)
        add("world, min_range longer than a hit", 0, WORLD_SENSOR_POS, ident, w["dirs"], None, 3.0, 6.0)
    else:
        hand = sb.body_index("hand")
        top = lambda b: b if spec.body[b].parent == 0 else top(spec.body[b].parent)  # noqa: E731
        skip = sum(1 << g for g in range(spec.ngeom) if spec.geom[g].body and top(spec.geom[g].body) == top(hand))
        lidar = sensors.SphericalPattern((360.0, 60.0), (32, 8))
        add("hand lidar", hand, (0.0, 0.0, 0.05), sensors.euler_to_quat((0.0, 15.0, 30.0)), lidar.directions(), lidar.shape, 0.0, 5.0, skip)
        cam = sensors.DepthCameraPattern((16, 12), 50.0)
        pos, look = ((1.2, 0.0, 0.9), (0.3, 0.0, 0.2)) if name == "pick" else ((1.2, 0.0, 1.6), (-0.2, 0.0, 0.75))
        add("world depth camera", 0, pos, sensors.lookat_quat(pos, look), cam.directions(), cam.shape, 0.0, 8.0)
    return out


def reference(name, si, world_frame=False, dtype=np.float64):
    """ray_ref of sensor `si` of a case on all B envs: float64 on the oracle's poses, or the float32 port on the float32 oracle's"""
    return _reference(name, si, bool(world_frame), np.dtype(dtype).name)


@functools.lru_cache(maxsize=None)
def _reference(name, si, world_frame, dtname):
    c = case(name)
    s = c["sensors"][si]
    f32 = dtname == "float32"
    return ray_ref.raycast(c["scene"], c["xp32"] if f32 else c["xp"], c["xq32"] if f32 else c["xq"], s["link"], s["pos_offset"], s["quat_offset"],
                           s["dirs"], s["min_range"], s["max_range"], s["skip"], world_frame, np.float32 if f32 else np.float64, with_ambiguous=not f32)
