"""Range sensors on a MirScene: ``scene.add_sensor(Lidar(...))`` + ``sensor.read()`` -> ``points``, ``distances`` (Genesis:
``gs.sensors.Raycaster`` / ``Lidar`` / ``DepthCamera`` with their ray patterns; parity with Genesis unpinned -- the reference's tasks
cast no rays and the package is not in the reference tree, the names follow its sensor API as far as it is remembered).

One sensor = one origin and N ray directions in the sensor's frame, riding on a link (or fixed in the world); a read is ONE launch of
``mir_raycast`` (include/mirigid.h) for the envs asked for.  The sensor frame is x forward, y left, z up.

Patterns (each has ``.shape`` and ``.directions()`` -> float32 ``(prod(shape), 3)`` unit vectors, row-major over ``shape``):
  * ``SphericalPattern(fov=(360, 30), n_points=(64, 16))``: shape (n_h, n_v); azimuths spread over the horizontal field of view about
    +x (a full turn leaves out its end point), elevations from -fov_v / 2 to +fov_v / 2; d = (cos el cos az, cos el sin az, sin el).
  * ``GridPattern(resolution, size, direction=(0, 0, -1))``: shape (n_x, n_y); the rays leave the ONE origin towards the nodes of a
    grid of ``size`` metres with ``resolution`` spacing, centred on the plane one metre along ``direction`` (Genesis's grid casts
    parallel rays from a grid of origins; mir_raycast carries one origin per sensor).
  * ``DepthCameraPattern(res=(W, H), fov_vertical=60)``: shape (H, W); the pinhole camera of include/mirigid.h -- pixel centres, row 0
    at the top, d = F + x R + y U before normalising -- with F = +x, R = -y, U = +z of the sensor frame.

Inertial sensors: ``scene.add_sensor(IMU(entity=robot, link="hand"))`` + ``sensor.read()`` -> ``lin_acc``, ``ang_vel`` (Genesis:
``gs.sensors.IMU``): what an accelerometer and a gyro on the link read, in the sensor's frame; a read is ONE launch of
``mir_link_accelerations`` for the envs asked for.
"""
from __future__ import annotations

import math
from collections import namedtuple
from dataclasses import dataclass, field
from typing import Any, Optional, Sequence, Tuple

import numpy as np
import torch


def _unit(v) -> np.ndarray:
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


class SphericalPattern:
    def __init__(self, fov: Sequence[float] = (360.0, 30.0), n_points: Sequence[int] = (64, 16)):
        self.fov = (float(fov[0]), float(fov[1]))
        self.n_points = (int(n_points[0]), int(n_points[1]))
        if min(self.n_points) < 1:
            raise ValueError("SphericalPattern: n_points must be >= 1")
        self.shape = self.n_points

    def directions(self) -> np.ndarray:
        nh, nv = self.n_points
        fh, fv = math.radians(self.fov[0]), math.radians(self.fov[1])
        az = np.linspace(-0.5 * fh, 0.5 * fh, nh, endpoint=self.fov[0] < 360.0) if nh > 1 else np.zeros(1)
        el = np.linspace(-0.5 * fv, 0.5 * fv, nv) if nv > 1 else np.zeros(1)
        a, e = np.meshgrid(az, el, indexing="ij")
        d = np.stack([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)], axis=-1)
        return _unit(d.reshape(-1, 3)).astype(np.float32)


class GridPattern:
    def __init__(self, resolution: float = 0.1, size: Sequence[float] = (1.0, 1.0), direction: Sequence[float] = (0.0, 0.0, -1.0)):
        self.resolution = float(resolution)
        self.size = (float(size[0]), float(size[1]))
        self.direction = tuple(float(v) for v in direction)
        if not self.resolution > 0.0:
            raise ValueError("GridPattern: resolution must be > 0")
        self.shape = tuple(int(round(s / self.resolution)) + 1 for s in self.size)

    def directions(self) -> np.ndarray:
        f = _unit(self.direction)
        # the grid's axes: x of the sensor frame made perpendicular to the direction (y when the direction is along x), and their cross
        u = np.array([1.0, 0.0, 0.0]) if abs(f[0]) < 0.9 else np.array([0.0, 1.0, 0.0])
        u = _unit(u - (u @ f) * f)
        v = np.cross(f, u)
        xs = (np.arange(self.shape[0]) - 0.5 * (self.shape[0] - 1)) * self.resolution
        ys = (np.arange(self.shape[1]) - 0.5 * (self.shape[1] - 1)) * self.resolution
        x, y = np.meshgrid(xs, ys, indexing="ij")
        d = f[None, None] + x[..., None] * u + y[..., None] * v
        return _unit(d.reshape(-1, 3)).astype(np.float32)


class DepthCameraPattern:
    def __init__(self, res: Sequence[int] = (64, 48), fov_vertical: float = 60.0):
        self.res = (int(res[0]), int(res[1]))
        self.fov_vertical = float(fov_vertical)
        if min(self.res) < 1:
            raise ValueError("DepthCameraPattern: res must be >= 1")
        self.shape = (self.res[1], self.res[0])

    def rays(self) -> np.ndarray:
        """(H, W, 3) float64: d = F + x R + y U, not normalised (its x component is 1: range x d^.x = planar depth)"""
        W, H = self.res
        ty = math.tan(0.5 * math.radians(self.fov_vertical))
        tx = ty * W / H
        xs = (2.0 * (np.arange(W) + 0.5) / W - 1.0) * tx
        ys = (1.0 - 2.0 * (np.arange(H) + 0.5) / H) * ty
        d = np.empty((H, W, 3))
        d[..., 0] = 1.0
        d[..., 1] = -xs[None, :]
        d[..., 2] = ys[:, None]
        return d

    def directions(self) -> np.ndarray:
        return _unit(self.rays().reshape(-1, 3)).astype(np.float32)


def euler_to_quat(euler_deg: Sequence[float]) -> tuple:
    """xyz Euler angles in degrees (rotations about the fixed x, then y, then z axis: R = Rz Ry Rx) -> wxyz"""
    x, y, z = (0.5 * math.radians(float(v)) for v in euler_deg)
    cx, sx, cy, sy, cz, sz = math.cos(x), math.sin(x), math.cos(y), math.sin(y), math.cos(z), math.sin(z)
    return (cz * cy * cx + sz * sy * sx, cz * cy * sx - sz * sy * cx, cz * sy * cx + sz * cy * sx, sz * cy * cx - cz * sy * sx)


def lookat_quat(pos: Sequence[float], lookat: Sequence[float], up: Sequence[float] = (0.0, 0.0, 1.0)) -> tuple:
    """wxyz of the sensor frame (x forward, y left, z up) of a camera at `pos` looking at `lookat`: the camera of scene.add_camera
    with the same arguments (a view parallel to `up` falls back to +y, then +x, as mir_render does)."""
    f = _unit(np.asarray(lookat, float) - np.asarray(pos, float))
    r = np.cross(f, np.asarray(up, float))
    for fb in ((0.0, 1.0, 0.0), (1.0, 0.0, 0.0)):
        if r @ r >= 1e-24:
            break
        r = np.cross(f, np.asarray(fb))
    r = _unit(r)
    u = np.cross(r, f)
    m = np.stack([f, -r, u], axis=1)  # columns: the sensor's x, y, z in world axes
    t = m[0, 0] + m[1, 1] + m[2, 2]
    if t > 0.0:
        s = math.sqrt(t + 1.0) * 2.0
        q = (0.25 * s, (m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s)
    elif m[0, 0] > m[1, 1] and m[0, 0] > m[2, 2]:
        s = math.sqrt(1.0 + m[0, 0] - m[1, 1] - m[2, 2]) * 2.0
        q = ((m[2, 1] - m[1, 2]) / s, 0.25 * s, (m[0, 1] + m[1, 0]) / s, (m[0, 2] + m[2, 0]) / s)
    elif m[1, 1] > m[2, 2]:
        s = math.sqrt(1.0 + m[1, 1] - m[0, 0] - m[2, 2]) * 2.0
        q = ((m[0, 2] - m[2, 0]) / s, (m[0, 1] + m[1, 0]) / s, 0.25 * s, (m[1, 2] + m[2, 1]) / s)
    else:
        s = math.sqrt(1.0 + m[2, 2] - m[0, 0] - m[1, 1]) * 2.0
        q = ((m[1, 0] - m[0, 1]) / s, (m[0, 2] + m[2, 0]) / s, (m[1, 2] + m[2, 1]) / s, 0.25 * s)
    return tuple(float(v) for v in q)


@dataclass
class Raycaster:
    """Options of a ray-cast range sensor.  `link`: a LinkView, or a link name together with `entity`, or None -- then the sensor rides
    on the entity's root link, or is fixed in the world when there is no entity either.  `pos_offset` / `euler_offset` (degrees, xyz;
    or `quat_offset` wxyz, which wins): the sensor frame in the link's frame.  `skip_own_entity`: the geoms of the sensor's own entity
    (the kinematic tree its link belongs to) are not tested."""
    pattern: Any = field(default_factory=SphericalPattern)
    entity: Any = None
    link: Any = None
    pos_offset: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    euler_offset: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    min_range: float = 0.0
    max_range: float = 20.0
    return_world_frame: bool = False
    skip_own_entity: bool = True
    quat_offset: Optional[Tuple[float, float, float, float]] = None


Lidar = Raycaster


@dataclass
class DepthCamera(Raycaster):
    pattern: Any = field(default_factory=DepthCameraPattern)


_READ_TYPES = {}


def _read_type(names: tuple):
    t = _READ_TYPES.get(names)
    if t is None:
        t = _READ_TYPES[names] = namedtuple("RaycastData", names)
    return t


class RaySensor:
    """What SceneView.add_sensor returns.  The pattern's directions are uploaded once."""

    def __init__(self, mir, options):
        self._mir, self.options, self.pattern = mir, options, options.pattern
        self.shape = tuple(int(s) for s in self.pattern.shape)
        spec = mir.spec
        entity = options.entity
        body = _link_body(options)
        if not 0 <= body < spec.nbody:
            raise ValueError(f"link body {body} outside the scene's {spec.nbody} bodies")
        self.link_body = body
        # the sensor's own entity: the links of `entity`, or the kinematic tree the link belongs to (nothing for a world-fixed sensor)
        own = set()
        if entity is not None:
            own = set(int(b) for b in entity.link_idx)
        elif body > 0:
            top = lambda b: b if spec.body[b].parent == 0 else top(spec.body[b].parent)  # noqa: E731
            own = {b for b in range(1, spec.nbody) if top(b) == top(body)}
        self.skip_geoms = 0
        if options.skip_own_entity:
            for g in range(spec.ngeom):
                if spec.geom[g].body in own:
                    self.skip_geoms |= 1 << g
        self.quat_offset = tuple(float(v) for v in options.quat_offset) if options.quat_offset is not None else euler_to_quat(options.euler_offset)
        self.pos_offset = tuple(float(v) for v in options.pos_offset)
        dirs = np.ascontiguousarray(self.pattern.directions(), dtype=np.float32)
        if dirs.shape != (int(np.prod(self.shape)), 3):
            raise ValueError(f"pattern.directions() must be ({int(np.prod(self.shape))}, 3), got {dirs.shape}")
        self._dirs = torch.as_tensor(dirs, device=mir.device)

    def _cast(self, envs_idx, **outs) -> dict:
        from .views import _env_index

        fn = getattr(self._mir, "raycast", None)
        if fn is None:
            raise NotImplementedError("this scene has no range sensing (MirScene.raycast / mir_raycast)")
        o = self.options
        return fn(self._dirs, link=self.link_body, pos_offset=self.pos_offset, quat_offset=self.quat_offset, min_range=float(o.min_range),
                  max_range=float(o.max_range), skip_geoms=self.skip_geoms, env_idx=_env_index(self._mir, envs_idx),
                  world_frame=bool(o.return_world_frame), **outs)

    def read(self, envs_idx=None, geoms: bool = False, normals: bool = False):
        """-> named tuple (points (R, *shape, 3), distances (R, *shape)[, geoms (R, *shape) int32][, normals (R, *shape, 3)])"""
        r = self._cast(envs_idx, distance=True, points=True, geom=bool(geoms), normal=bool(normals))
        R = r["distance"].shape[0]
        names, vals = ["points", "distances"], [r["points"].reshape(R, *self.shape, 3), r["distance"].reshape(R, *self.shape)]
        if geoms:
            names.append("geoms")
            vals.append(r["geom"].reshape(R, *self.shape))
        if normals:
            names.append("normals")
            vals.append(r["normal"].reshape(R, *self.shape, 3))
        return _read_type(tuple(names))(*vals)

    def read_image(self, envs_idx=None) -> torch.Tensor:
        """Planar depth (R, H, W) of a DepthCameraPattern: range x the cosine to the optical axis (+x of the sensor frame), in torch."""
        if not isinstance(self.pattern, DepthCameraPattern):
            raise TypeError("read_image needs a DepthCameraPattern")
        dist = self._cast(envs_idx, distance=True, points=False, geom=False, normal=False)["distance"]
        return (dist * self._dirs[:, 0][None, :]).reshape(dist.shape[0], *self.shape)


@dataclass
class IMU:
    """Options of an inertial measurement unit (Genesis: ``gs.sensors.IMU``; parity with Genesis unpinned): an accelerometer and a gyro on
    a link.  `link`: a LinkView, or a link name together with `entity`, or None -- then the sensor rides on the entity's root link (it
    needs a link: there is nothing to measure in the world's frame).  `pos_offset` / `euler_offset` (degrees, xyz; or `quat_offset`
    wxyz, which wins): the sensor frame in the link's frame.  No noise, bias or delay model: that is torch on the caller's side."""
    entity: Any = None
    link: Any = None
    pos_offset: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    euler_offset: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    quat_offset: Optional[Tuple[float, float, float, float]] = None


ImuData = namedtuple("ImuData", ("lin_acc", "ang_vel"))


def _link_body(options) -> int:
    """the body a sensor's options put it on (0: the world), resolved as for Raycaster"""
    from .views import LinkView

    link, entity = options.link, options.entity
    if isinstance(link, LinkView):
        return link.idx
    if isinstance(link, str):
        if entity is None:
            raise ValueError("a link name needs the entity it belongs to")
        return entity.get_link(link).idx
    if link is None:
        return 0 if entity is None else int(entity.root)
    return int(link)


class ImuSensor:
    """What SceneView.add_sensor returns for IMU options."""

    def __init__(self, mir, options):
        self._mir, self.options = mir, options
        body = _link_body(options)
        if not 1 <= body < mir.spec.nbody:
            raise ValueError(f"an IMU rides on a link: body {body} outside 1 .. {mir.spec.nbody - 1}")
        self.link_body = body
        self.quat_offset = tuple(float(v) for v in options.quat_offset) if options.quat_offset is not None else euler_to_quat(options.euler_offset)
        self.pos_offset = tuple(float(v) for v in options.pos_offset)

    def read(self, envs_idx=None, qacc=None) -> ImuData:
        """-> named tuple (lin_acc (R, 3), ang_vel (R, 3)) in the sensor's frame: the classical acceleration of the sensor's point minus
        gravity (at rest: +9.81 along the world's up axis) and the link's angular velocity.  `qacc` (R, nv): the joint accelerations
        to read at; None: those the next step applies if the targets stay as they are (one forward evaluation)."""
        from .views import _env_index

        fn = getattr(self._mir, "link_accelerations", None)
        if fn is None:
            raise NotImplementedError("this scene has no link accelerations (MirScene.link_accelerations / mir_link_accelerations)")
        r = fn([self.link_body], local_points=self.pos_offset, quat_offsets=self.quat_offset, env_idx=_env_index(self._mir, envs_idx), qacc=qacc,
               acc=False, imu=True)["imu"]
        return ImuData(r[:, 0, 0:3].contiguous(), r[:, 0, 3:6].contiguous())


@dataclass
class Proximity:
    """Options of a proximity sensor (this package's own: parity with Genesis unpinned): the signed distance from one probe sphere to
    the nearest surface, whatever the direction -- negative inside a solid, which a ray never reports.  `link` / `entity` as for
    Raycaster (None: fixed in the world); `pos_offset`: the probe's centre in the link's frame; `radius`: of the probe; `max_range`:
    what is reported when nothing is that near; `skip_own_entity`: the geoms of the link's own entity are not tested."""
    entity: Any = None
    link: Any = None
    pos_offset: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    radius: float = 0.0
    max_range: float = 1.0
    skip_own_entity: bool = True


ProximityData = namedtuple("ProximityData", ("distance", "point", "normal"))


class ProximitySensor:
    """What SceneView.add_sensor returns for Proximity options.  The probe is uploaded once."""

    def __init__(self, mir, options):
        self._mir, self.options = mir, options
        spec = mir.spec
        body = _link_body(options)
        if not 0 <= body < spec.nbody:
            raise ValueError(f"link body {body} outside the scene's {spec.nbody} bodies")
        if not (float(options.radius) >= 0.0 and float(options.max_range) > 0.0):
            raise ValueError("a proximity sensor needs radius >= 0 and max_range > 0")
        self.link_body = body
        own = set()
        if options.entity is not None:
            own = set(int(b) for b in options.entity.link_idx)
        elif body > 0:
            top = lambda b: b if spec.body[b].parent == 0 else top(spec.body[b].parent)  # noqa: E731
            own = {b for b in range(1, spec.nbody) if top(b) == top(body)}
        self.skip_geoms = 0
        if options.skip_own_entity:
            for g in range(spec.ngeom):
                if spec.geom[g].body in own:
                    self.skip_geoms |= 1 << g
        probe = np.array([[*(float(v) for v in options.pos_offset), float(options.radius)]], dtype=np.float32)
        self._probe = torch.as_tensor(probe, device=mir.device)
        self._links = np.array([body], dtype=np.int32)

    def read(self, envs_idx=None) -> ProximityData:
        """-> named tuple (distance (R,), point (R, 3) the nearest surface point in world axes, normal (R, 3) unit, from the surface
        towards the probe); nothing within max_range: max_range, the probe's own centre, 0.  One launch."""
        from .views import _env_index

        fn = getattr(self._mir, "signed_distance", None)
        if fn is None:
            raise NotImplementedError("this scene has no signed distance (MirScene.signed_distance / mir_signed_distance)")
        r = fn(self._probe, links=self._links, env_idx=_env_index(self._mir, envs_idx), max_distance=float(self.options.max_range),
               skip_geoms=self.skip_geoms, closest=True, normal=True)
        return ProximityData(r["distance"][:, 0], r["closest"][:, 0], r["normal"][:, 0])


def make_sensor(mir, options):
    if isinstance(options, IMU):
        return ImuSensor(mir, options)
    if isinstance(options, Proximity):
        return ProximitySensor(mir, options)
    if not isinstance(options, Raycaster):
        raise TypeError(f"add_sensor takes Raycaster / Lidar / DepthCamera options, got {type(options).__name__}")
    return RaySensor(mir, options)
