"""ctypes mirror of include/mirigid.h (MirSceneSpec and friends) plus a small
builder API used to describe a scene the way the reference's tasks do with
``scene.add_entity`` (/root/reference/gym_genesis/tasks/franka/cube_pick.py:50-54).

Pure host-side data: no physics here.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional, Sequence

MIR_VERSION = 3
MIR_MAX_BODY = 32
MIR_MAX_DOF = 48
MIR_MAX_Q = 56
MIR_MAX_GEOM = 40
MIR_MAX_PAIR = 256
MIR_MAX_CONTACT = 48
MIR_MAX_GRIP = 4
MIR_MAX_FREE = 8
# limits of the 16-lanes-per-env kernel (the pick tasks); larger scenes run on the wave-per-env kernel
K16_MAX_CONTACT = 16
REWARD_LIFT, REWARD_STACK = 0, 1
AGENT_EEF, AGENT_QPOS = 0, 1

JNT_FIXED, JNT_REVOLUTE, JNT_PRISMATIC, JNT_FREE = 0, 1, 2, 3
GEOM_PLANE, GEOM_BOX, GEOM_SPHERE, GEOM_CAPSULE = 0, 1, 2, 3  # sphere: size = (radius,); capsule: (radius, half length), axis z
GEOM_HULL = 4  # convex hull of the vertices given to add_geom(vertices=...), geom frame, origin inside the hull
MIR_MAX_HULL_VERT, MIR_MAX_VERT = 32, 96
CTRL_NONE, CTRL_POSITION = 0, 1

DEFAULT_SOLREF = (0.02, 1.0)
DEFAULT_SOLIMP = (0.9, 0.95, 0.001, 0.5, 2.0)


class MirBodySpec(C.Structure):
    _fields_ = [
        ("parent", C.c_int32),
        ("jtype", C.c_int32),
        ("pos", C.c_double * 3),
        ("quat", C.c_double * 4),
        ("axis", C.c_double * 3),
        ("mass", C.c_double),
        ("ipos", C.c_double * 3),
        ("inertia", C.c_double * 6),
    ]


class MirDofSpec(C.Structure):
    _fields_ = [
        ("limited", C.c_int32),
        ("ctrl_mode", C.c_int32),
        ("range", C.c_double * 2),
        ("armature", C.c_double),
        ("damping", C.c_double),
        ("kp", C.c_double),
        ("kv", C.c_double),
        ("frc_range", C.c_double * 2),
        ("solref", C.c_double * 2),
        ("solimp", C.c_double * 5),
    ]


class MirGeomSpec(C.Structure):
    _fields_ = [
        ("body", C.c_int32),
        ("type", C.c_int32),
        ("contype", C.c_int32),
        ("conaffinity", C.c_int32),
        ("size", C.c_double * 3),
        ("pos", C.c_double * 3),
        ("quat", C.c_double * 4),
        ("friction", C.c_double),
        ("solref", C.c_double * 2),
        ("solimp", C.c_double * 5),
    ]


class MirOptions(C.Structure):
    _fields_ = [
        ("dt", C.c_double),
        ("gravity", C.c_double * 3),
        ("tolerance", C.c_double),
        ("ls_tolerance", C.c_double),
        ("iterations", C.c_int32),
        ("ls_iterations", C.c_int32),
        ("enable_collision", C.c_int32),
        ("enable_joint_limit", C.c_int32),
        ("enable_self_collision", C.c_int32),
        ("enable_adjacent_collision", C.c_int32),
        ("max_contacts", C.c_int32),
        ("implicit_damping", C.c_int32),
    ]


class MirTaskSpec(C.Structure):
    _fields_ = [
        ("eef_body", C.c_int32),
        ("obj_body", C.c_int32),
        ("n_grip", C.c_int32),
        ("grip_dof", C.c_int32 * MIR_MAX_GRIP),
        ("reward_z", C.c_double),
        ("obj2_body", C.c_int32),
        ("reward_mode", C.c_int32),
        ("agent_mode", C.c_int32),
        ("_pad", C.c_int32),
        ("reward_xy", C.c_double),
        ("reward_dz", C.c_double),
    ]


class MirSceneSpec(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32),
        ("version", C.c_int32),
        ("nbody", C.c_int32),
        ("ndof", C.c_int32),
        ("ngeom", C.c_int32),
        ("_pad", C.c_int32),
        ("opt", MirOptions),
        ("task", MirTaskSpec),
        ("body", MirBodySpec * MIR_MAX_BODY),
        ("dof", MirDofSpec * MIR_MAX_DOF),
        ("geom", MirGeomSpec * MIR_MAX_GEOM),
        ("nvert", C.c_int32),
        ("_pad2", C.c_int32),
        ("vert", (C.c_double * 3) * MIR_MAX_VERT),
    ]


class MirDims(C.Structure):
    _fields_ = [
        ("num_envs", C.c_int32),
        ("nbody", C.c_int32),
        ("nq", C.c_int32),
        ("nv", C.c_int32),
        ("ngeom", C.c_int32),
        ("npair", C.c_int32),
        ("agent_dim", C.c_int32),
        ("env_dim", C.c_int32),
        ("nfree", C.c_int32),
        ("kernel", C.c_int32),
    ]


class MirCameraSpec(C.Structure):
    """scene.add_camera(res=(W,H), pos, lookat, fov) (reference cube_pick.py:56-63)."""
    _fields_ = [
        ("width", C.c_int32),
        ("height", C.c_int32),
        ("pos", C.c_double * 3),
        ("lookat", C.c_double * 3),
        ("up", C.c_double * 3),
        ("fov_deg", C.c_double),
    ]


MIR_VIS_ROUND_GEOMS = 1  # MirVisualSpec.flags: spheres and capsules drawn as themselves (include/mirigid.h)


class MirVisualSpec(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32),
        ("flags", C.c_int32),
        ("geom_rgb", (C.c_double * 3) * MIR_MAX_GEOM),
        ("light_dir", C.c_double * 3),
        ("ambient", C.c_double),
        ("diffuse", C.c_double),
        ("sky_rgb", C.c_double * 3),
        ("checker_rgb", (C.c_double * 3) * 2),
        ("checker_size", C.c_double),
    ]


class MirIkOptions(C.Structure):
    _fields_ = [
        ("max_iters", C.c_int32),
        ("respect_joint_limit", C.c_int32),
        ("damping", C.c_double),
        ("pos_tol", C.c_double),
        ("rot_tol", C.c_double),
        ("max_step", C.c_double),
    ]


class MirIkRows(C.Structure):
    """include/mirigid.h: MirIkRows (mir_inverse_kinematics_rows)"""
    _fields_ = [
        ("env_idx", C.c_void_p),
        ("n_rows", C.c_int32),
        ("flags", C.c_uint32),
        ("init_col0", C.c_int32),
        ("init_ncols", C.c_int32),
    ]


IK_POS_BY_ENV, IK_QUAT_BY_ENV, IK_QUAT_ONE, IK_INIT_BY_ENV = 1, 2, 4, 8

IK_MAX_LINKS = 4


class MirIkMulti(C.Structure):
    """include/mirigid.h: MirIkMulti (mir_inverse_kinematics_multilink)"""
    _fields_ = [
        ("struct_size", C.c_int32),
        ("n_links", C.c_int32),
        ("link_body", C.c_int32 * IK_MAX_LINKS),
        ("pos_mask", C.c_uint8 * 3),
        ("rot_mask", C.c_uint8 * 3),
        ("reserved", C.c_uint8 * 2),
        ("dof_mask", C.c_void_p),
        ("max_samples", C.c_int32),
        ("seed", C.c_uint32),
        ("rows", MirIkRows),
    ]


def make_ik_multi(links: Sequence[int], pos_mask=(True, True, True), rot_mask=(True, True, True), dof_mask=None, max_samples: int = 1,
                  seed: int = 0, n_arm: int = 0) -> MirIkMulti:
    """links: 1 .. 4 body indices of the spec; pos_mask / rot_mask: three booleans each, shared by the links (rot_mask: 0, 1 or 3 true);
    dof_mask: n_arm booleans over the joint columns, None = every joint on a chain.  The mask's bytes are kept alive by the struct
    (`_dof_mask_buf`); `rows` is left for the caller."""
    q = MirIkMulti()
    q.struct_size = C.sizeof(MirIkMulti)
    links = [int(b) for b in links]
    if not 1 <= len(links) <= IK_MAX_LINKS:
        raise ValueError(f"inverse_kinematics_multilink takes 1 .. {IK_MAX_LINKS} links, got {len(links)}")
    pm, rm = [bool(v) for v in pos_mask], [bool(v) for v in rot_mask]
    if len(pm) != 3 or len(rm) != 3:
        raise ValueError("pos_mask and rot_mask take three entries")
    if sum(rm) == 2:
        raise ValueError("You can only align 0, 1 axis or all 3 axes.")
    if int(max_samples) < 1:
        raise ValueError("max_samples must be at least 1")
    q.n_links = len(links)
    q.link_body[:len(links)] = links
    q.pos_mask[:] = [int(v) for v in pm]
    q.rot_mask[:] = [int(v) for v in rm]
    if dof_mask is not None:
        dm = [1 if v else 0 for v in dof_mask]
        if len(dm) != int(n_arm):
            raise ValueError(f"dof_mask must have one entry per joint column ({n_arm}), got {len(dm)}")
        q._dof_mask_buf = (C.c_uint8 * len(dm))(*dm)
        q.dof_mask = C.addressof(q._dof_mask_buf)
    q.max_samples, q.seed = int(max_samples), int(seed) & 0xFFFFFFFF
    return q


class MirKinQuery(C.Structure):
    """include/mirigid.h: MirKinQuery (mir_link_kinematics)"""
    _fields_ = [
        ("struct_size", C.c_int32),
        ("n_links", C.c_int32),
        ("link_body", C.c_int32 * MIR_MAX_BODY),
        ("local_point", (C.c_float * 3) * MIR_MAX_BODY),
        ("dof0", C.c_int32),
        ("n_dofs", C.c_int32),
    ]


def make_kin_query(links: Sequence[int], local_points=None, dof0: int = 0, n_dofs: int = 0) -> MirKinQuery:
    """links: body indices of the spec; local_points: one point (3,) for every link, or one per link (n_links, 3); None = the origins."""
    q = MirKinQuery()
    q.struct_size = C.sizeof(MirKinQuery)
    links = [int(b) for b in links]
    if not 1 <= len(links) <= MIR_MAX_BODY:
        raise ValueError(f"link_kinematics takes 1 .. {MIR_MAX_BODY} links, got {len(links)}")
    q.n_links = len(links)
    q.link_body[:len(links)] = links
    if local_points is not None:
        pts = local_points.tolist() if hasattr(local_points, "tolist") else list(local_points)
        if pts and not isinstance(pts[0], (list, tuple)):
            pts = [pts] * len(links)
        pts = [[float(v) for v in p] for p in pts]
        if len(pts) != len(links) or any(len(p) != 3 for p in pts):
            raise ValueError("local_points must be (3,) or (n_links, 3)")
        for i, p in enumerate(pts):
            q.local_point[i][:] = p
    q.dof0, q.n_dofs = int(dof0), int(n_dofs)
    return q


class MirAccQuery(C.Structure):
    """include/mirigid.h: MirAccQuery (mir_link_accelerations)"""
    _fields_ = [
        ("struct_size", C.c_int32),
        ("n_links", C.c_int32),
        ("link_body", C.c_int32 * MIR_MAX_BODY),
        ("local_point", (C.c_float * 3) * MIR_MAX_BODY),
        ("quat_offset", (C.c_float * 4) * MIR_MAX_BODY),
        ("flags", C.c_uint32),
    ]


def _per_link(values, n_links: int, width: int, name: str) -> list:
    """one row of `width` floats for every link, or one per link -> n_links rows"""
    rows = values.tolist() if hasattr(values, "tolist") else list(values)
    if rows and not isinstance(rows[0], (list, tuple)):
        rows = [rows] * n_links
    rows = [[float(v) for v in r] for r in rows]
    if len(rows) != n_links or any(len(r) != width for r in rows):
        raise ValueError(f"{name} must be ({width},) or (n_links, {width})")
    return rows


def make_acc_query(links: Sequence[int], local_points=None, quat_offsets=None, flags: int = 0) -> MirAccQuery:
    """links: body indices of the spec; local_points: one point (3,) for every link, or one per link (n_links, 3); None = the origins;
    quat_offsets: the sensors' axes in their links' frames, wxyz, (4,) or (n_links, 4); None (all-zero in the struct) = the links' axes.
    No flag bit is defined yet."""
    q = MirAccQuery()
    q.struct_size = C.sizeof(MirAccQuery)
    links = [int(b) for b in links]
    if not 1 <= len(links) <= MIR_MAX_BODY:
        raise ValueError(f"link_accelerations takes 1 .. {MIR_MAX_BODY} links, got {len(links)}")
    if int(flags) != 0:
        raise ValueError(f"unknown MirAccQuery flag bits {int(flags):#x}")
    q.n_links = len(links)
    q.link_body[:len(links)] = links
    if local_points is not None:
        for i, p in enumerate(_per_link(local_points, len(links), 3, "local_points")):
            q.local_point[i][:] = p
    if quat_offsets is not None:
        for i, p in enumerate(_per_link(quat_offsets, len(links), 4, "quat_offsets")):
            q.quat_offset[i][:] = p
    q.flags = 0
    return q


class MirDynQuery(C.Structure):
    """include/mirigid.h: MirDynQuery (mir_dynamics)"""
    _fields_ = [
        ("struct_size", C.c_int32),
        ("dof0", C.c_int32),
        ("n_dofs", C.c_int32),
        ("flags", C.c_uint32),
    ]


def make_dyn_query(dof0: int = 0, n_dofs: int = 0, flags: int = 0) -> MirDynQuery:
    """The window of scene dofs [dof0, dof0 + n_dofs) of a dynamics query; no flag bit is defined yet."""
    dof0, n_dofs, flags = int(dof0), int(n_dofs), int(flags)
    if dof0 < 0 or n_dofs < 0 or dof0 + n_dofs > MIR_MAX_DOF:
        raise ValueError(f"dynamics window [{dof0}, {dof0 + n_dofs}) outside [0, {MIR_MAX_DOF}]")
    if flags != 0:
        raise ValueError(f"unknown MirDynQuery flag bits {flags:#x}")
    q = MirDynQuery()
    q.struct_size = C.sizeof(MirDynQuery)
    q.dof0, q.n_dofs, q.flags = dof0, n_dofs, flags
    return q


class MirTaskQuery(C.Structure):
    """include/mirigid.h: MirTaskQuery (mir_task_dynamics)"""
    _fields_ = [
        ("struct_size", C.c_int32),
        ("n_links", C.c_int32),
        ("link_body", C.c_int32 * MIR_MAX_BODY),
        ("local_point", (C.c_float * 3) * MIR_MAX_BODY),
        ("dof0", C.c_int32),
        ("n_dofs", C.c_int32),
        ("damping", C.c_float),
        ("flags", C.c_uint32),
    ]


def make_task_query(links: Sequence[int] = (), local_points=None, dof0: int = 0, n_dofs: int = 0, damping: float = 0.0, flags: int = 0) -> MirTaskQuery:
    """links: body indices of the spec, none for a query of minv / solve alone; local_points: one task point (3,) for every link, or
    one per link (n_links, 3), in the link's frame; None = the origins; [dof0, dof0 + n_dofs): the window of scene dofs of the
    dof-indexed outputs; damping >= 0: damping^2 is added to the diagonal of lambda_inv before it is inverted.  No flag bit is defined
    yet."""
    links = [int(b) for b in links]
    dof0, n_dofs, damping, flags = int(dof0), int(n_dofs), float(damping), int(flags)
    if len(links) > MIR_MAX_BODY:
        raise ValueError(f"task_dynamics takes 0 .. {MIR_MAX_BODY} links, got {len(links)}")
    if any(b < 1 for b in links):
        raise ValueError(f"task_dynamics links are body indices >= 1, got {links}")
    if dof0 < 0 or n_dofs < 0 or dof0 + n_dofs > MIR_MAX_DOF:
        raise ValueError(f"task_dynamics window [{dof0}, {dof0 + n_dofs}) outside [0, {MIR_MAX_DOF}]")
    if not math.isfinite(damping) or damping < 0.0:
        raise ValueError(f"damping must be finite and >= 0, got {damping}")
    if flags != 0:
        raise ValueError(f"unknown MirTaskQuery flag bits {flags:#x}")
    q = MirTaskQuery()
    q.struct_size = C.sizeof(MirTaskQuery)
    q.n_links = len(links)
    q.link_body[:len(links)] = links
    if local_points is not None and links:
        for i, p in enumerate(_per_link(local_points, len(links), 3, "local_points")):
            if not all(math.isfinite(v) for v in p):
                raise ValueError("local_points must be finite")
            q.local_point[i][:] = p
    q.dof0, q.n_dofs, q.damping, q.flags = dof0, n_dofs, damping, flags
    return q


MIR_RAY_POINTS_WORLD = 1  # MirRayQuery.flags: points / normal in world axes (include/mirigid.h)


class MirRayQuery(C.Structure):
    """include/mirigid.h: MirRayQuery (mir_raycast)"""
    _fields_ = [
        ("struct_size", C.c_int32),
        ("link_body", C.c_int32),
        ("pos_offset", C.c_float * 3),
        ("quat_offset", C.c_float * 4),
        ("min_range", C.c_float),
        ("max_range", C.c_float),
        ("n_rays", C.c_int32),
        ("flags", C.c_uint32),
        ("skip_geoms", C.c_uint64),
    ]


def make_ray_query(n_rays: int, link: int = 0, pos_offset=(0.0, 0.0, 0.0), quat_offset=(1.0, 0.0, 0.0, 0.0), min_range: float = 0.0,
                   max_range: float = 100.0, skip_geoms=(), world_frame: bool = False) -> MirRayQuery:
    """link: body index of the spec the sensor rides on (0: the world); skip_geoms: geom indices that are not tested, or the bit mask."""
    q = MirRayQuery()
    q.struct_size = C.sizeof(MirRayQuery)
    q.link_body, q.n_rays = int(link), int(n_rays)
    q.pos_offset[:] = [float(v) for v in pos_offset]
    q.quat_offset[:] = [float(v) for v in quat_offset]
    q.min_range, q.max_range = float(min_range), float(max_range)
    q.flags = MIR_RAY_POINTS_WORLD if world_frame else 0
    if isinstance(skip_geoms, int):
        q.skip_geoms = skip_geoms
    else:
        mask = 0
        for g in skip_geoms:
            if not 0 <= int(g) < 64:
                raise ValueError(f"skip_geoms: geom index {g} outside 0 .. 63")
            mask |= 1 << int(g)
        q.skip_geoms = mask
    return q


DIST_MAX_PROBES = 1024  # probes of one mir_signed_distance call (include/mirigid.h)


class MirDistQuery(C.Structure):
    """include/mirigid.h: MirDistQuery (mir_signed_distance)"""
    _fields_ = [
        ("struct_size", C.c_int32),
        ("n_probes", C.c_int32),
        ("max_distance", C.c_float),
        ("flags", C.c_uint32),
        ("skip_geoms", C.c_uint64),
    ]


def _geom_mask(skip_geoms) -> int:
    """geom indices that are not tested, or the bit mask itself"""
    if isinstance(skip_geoms, int):
        return skip_geoms
    mask = 0
    for g in skip_geoms:
        if not 0 <= int(g) < 64:
            raise ValueError(f"skip_geoms: geom index {g} outside 0 .. 63")
        mask |= 1 << int(g)
    return mask


def make_dist_query(n_probes: int, max_distance: float = 1.0, skip_geoms=()) -> MirDistQuery:
    """skip_geoms: geom indices that are not tested, or the bit mask."""
    q = MirDistQuery()
    q.struct_size = C.sizeof(MirDistQuery)
    q.n_probes, q.max_distance, q.flags = int(n_probes), float(max_distance), 0
    q.skip_geoms = _geom_mask(skip_geoms)
    return q


PLAN_MAX_POLY = 128  # MIR_PLAN_MAX_POLY: nodes of the polyline mir_plan_path returns (include/mirigid.h)
PLAN_MAX_DOF = 16
PLAN_IGNORE_COLLISION = 1
PLAN_STATUS = ("OK", "GOAL_OUT_OF_LIMITS", "START_IN_COLLISION", "GOAL_IN_COLLISION", "NODE_LIMIT", "ITERATION_LIMIT", "PATH_TOO_LONG",
               "START_IN_SELF_COLLISION", "GOAL_IN_SELF_COLLISION")
(PLAN_OK, PLAN_GOAL_OUT_OF_LIMITS, PLAN_START_IN_COLLISION, PLAN_GOAL_IN_COLLISION, PLAN_NODE_LIMIT, PLAN_ITERATION_LIMIT,
 PLAN_PATH_TOO_LONG, PLAN_START_IN_SELF_COLLISION, PLAN_GOAL_IN_SELF_COLLISION) = range(9)
PLAN_MAX_GOALS = 8  # MIR_PLAN_MAX_GOALS: goal configurations per row of mir_plan_path_goals
PLAN_NO_VALID_GOAL = 9  # MIR_PLAN_NO_VALID_GOAL: the one row status mir_plan_path_goals adds
PLAN_GOAL_STATUS = PLAN_STATUS + ("NO_VALID_GOAL",)  # the row statuses of mir_plan_path_goals by value (a goal's own status is one of PLAN_STATUS)


class MirPlanQuery(C.Structure):
    """include/mirigid.h: MirPlanQuery (mir_plan_path, mir_path_clearance)"""
    _fields_ = [
        ("struct_size", C.c_int32),
        ("n_probes", C.c_int32),
        ("n_dofs", C.c_int32),
        ("num_waypoints", C.c_int32),
        ("max_nodes", C.c_int32),
        ("max_iterations", C.c_int32),
        ("smooth_passes", C.c_int32),
        ("flags", C.c_uint32),
        ("seed", C.c_uint32),
        ("resolution", C.c_float),
        ("step", C.c_float),
        ("margin", C.c_float),
        ("max_distance", C.c_float),
        ("_pad", C.c_int32),
        ("skip_geoms", C.c_uint64),
    ]


def make_plan_query(n_probes: int, n_dofs: int, num_waypoints: int = 100, max_nodes: int = 256, max_iterations: int = 2000, smooth_passes: int = 64,
                    ignore_collision: bool = False, seed: int = 0, resolution: float = 0.05, step: float = 0.3, margin: float = 0.0,
                    max_distance: float = 1.0, skip_geoms=()) -> MirPlanQuery:
    """skip_geoms: geom indices that are not tested, or the bit mask."""
    q = MirPlanQuery()
    q.struct_size = C.sizeof(MirPlanQuery)
    q.n_probes, q.n_dofs, q.num_waypoints, q.max_nodes = int(n_probes), int(n_dofs), int(num_waypoints), int(max_nodes)
    q.max_iterations, q.smooth_passes, q.flags, q.seed = int(max_iterations), int(smooth_passes), PLAN_IGNORE_COLLISION if ignore_collision else 0, int(seed) & 0xffffffff
    q.resolution, q.step, q.margin, q.max_distance = float(resolution), float(step), float(margin), float(max_distance)
    q.skip_geoms = _geom_mask(skip_geoms)
    return q


class MirSelfQuery(C.Structure):
    """include/mirigid.h: MirSelfQuery (mir_self_distance, mir_plan_path_self, mir_path_clearance_self)"""
    _fields_ = [
        ("struct_size", C.c_int32),
        ("n_extra", C.c_int32),
        ("self_margin", C.c_float),
        ("max_distance", C.c_float),
        ("flags", C.c_uint32),
        ("link_mask", C.c_uint32 * MIR_MAX_BODY),
    ]


def make_self_query(link_mask, n_extra: int = 0, self_margin: float = 0.0, max_distance: float = 1.0) -> MirSelfQuery:
    """link_mask: (32,) words, bit b of word a = the spheres on body a are tested against those on body b (symmetric, zero diagonal);
    None: nothing is tested."""
    q = MirSelfQuery()
    q.struct_size = C.sizeof(MirSelfQuery)
    q.n_extra, q.self_margin, q.max_distance, q.flags = int(n_extra), float(self_margin), float(max_distance), 0
    words = [0] * MIR_MAX_BODY if link_mask is None else [int(w) & 0xffffffff for w in link_mask]
    if len(words) != MIR_MAX_BODY:
        raise ValueError(f"link_mask must hold {MIR_MAX_BODY} words, got {len(words)}")
    q.link_mask[:] = words
    return q


class MirCarryQuery(C.Structure):
    """include/mirigid.h: MirCarryQuery (mir_plan_path_carry, mir_path_clearance_carry)"""
    _fields_ = [
        ("struct_size", C.c_int32),
        ("body", C.c_int32),
        ("link", C.c_int32),
        ("flags", C.c_uint32),
    ]


def make_carry_query(body: int, link: int) -> MirCarryQuery:
    """body: the carried free body C; link: the body it follows by the row's grasp transform (body indices of the scene)"""
    q = MirCarryQuery()
    q.struct_size = C.sizeof(MirCarryQuery)
    q.body, q.link, q.flags = int(body), int(link), 0
    return q


class MirGoalQuery(C.Structure):
    """include/mirigid.h: MirGoalQuery (mir_plan_path_goals)"""
    _fields_ = [
        ("struct_size", C.c_int32),
        ("max_goals", C.c_int32),
        ("flags", C.c_uint32),
        ("_pad", C.c_int32),
    ]


def make_goal_query(max_goals: int) -> MirGoalQuery:
    """max_goals: G, the goal configurations per row (1 .. PLAN_MAX_GOALS, below the planner's max_nodes)"""
    q = MirGoalQuery()
    q.struct_size = C.sizeof(MirGoalQuery)
    q.max_goals, q.flags = int(max_goals), 0
    return q


class MirPoseGoalQuery(C.Structure):
    """include/mirigid.h: MirPoseGoalQuery (mir_plan_path_pose)"""
    _fields_ = [
        ("struct_size", C.c_int32),
        ("link", C.c_int32),
        ("max_goals", C.c_int32),
        ("max_samples", C.c_int32),
        ("flags", C.c_uint32),
        ("dedup", C.c_float),
    ]


def make_pose_goal_query(link: int, max_goals: int = 4, max_samples: int = 16, dedup: float = 0.0) -> MirPoseGoalQuery:
    """link: the body whose pose is the goal; max_goals: G kept IK solutions at most (1 .. PLAN_MAX_GOALS); max_samples: IK seeds tried at
    most; dedup: two kept goals differ by at least this much in some joint (0: the planner's resolution)"""
    q = MirPoseGoalQuery()
    q.struct_size = C.sizeof(MirPoseGoalQuery)
    q.link, q.max_goals, q.max_samples, q.flags, q.dedup = int(link), int(max_goals), int(max_samples), 0, float(dedup)
    return q


RETIME_MAX_WAYPOINTS = 2048  # MIR_RETIME_MAX_WAYPOINTS (include/mirigid.h)
RETIME_MAX_DOF = 16
RETIME_STATUS = ("OK", "NO_MOTION", "TOO_FEW_WAYPOINTS", "NOT_FINITE", "INFEASIBLE", "TRUNCATED")
RETIME_OK, RETIME_NO_MOTION, RETIME_TOO_FEW_WAYPOINTS, RETIME_NOT_FINITE, RETIME_INFEASIBLE, RETIME_TRUNCATED = range(6)


class MirRetimeQuery(C.Structure):
    """include/mirigid.h: MirRetimeQuery (mir_retime_path)"""
    _fields_ = [
        ("struct_size", C.c_int32),
        ("n_dofs", C.c_int32),
        ("n_extra", C.c_int32),
        ("num_waypoints", C.c_int32),
        ("num_samples", C.c_int32),
        ("flags", C.c_uint32),
        ("dt", C.c_float),
        ("max_path_speed", C.c_float),
        ("vmax", C.c_float * RETIME_MAX_DOF),
        ("amax", C.c_float * RETIME_MAX_DOF),
    ]


def make_retime_query(n_dofs: int, num_waypoints: int, vmax, amax, dt: float, num_samples: int = 0, max_path_speed=None,
                      n_extra: int = 0) -> MirRetimeQuery:
    """vmax, amax: a scalar or n_dofs values; max_path_speed None: 1 / dt, at most one waypoint per sample."""
    q = MirRetimeQuery()
    q.struct_size = C.sizeof(MirRetimeQuery)
    q.n_dofs, q.n_extra, q.num_waypoints, q.num_samples, q.flags = int(n_dofs), int(n_extra), int(num_waypoints), int(num_samples), 0
    q.dt = float(dt)
    q.max_path_speed = (1.0 / q.dt if q.dt != 0.0 else math.inf) if max_path_speed is None else float(max_path_speed)   # (q.dt: the float32 the kernel reads)
    n = max(0, min(int(n_dofs), RETIME_MAX_DOF))
    for name, lim in (("vmax", vmax), ("amax", amax)):
        v = [float(x) for x in lim] if hasattr(lim, "__len__") else [float(lim)] * n
        if len(v) != n:
            raise ValueError(f"{name} must be a scalar or {n} values, got {len(v)}")
        getattr(q, name)[:n] = v
    return q


CART_STATUS = {0: "OK", 2: "START_IN_COLLISION", 7: "START_IN_SELF_COLLISION", 16: "TOO_MANY_POINTS", 17: "NOT_FINITE", 18: "IK_FAILED",
               19: "JOINT_JUMP", 20: "BLOCKED", 21: "BLOCKED_SELF"}   # mir_cartesian_path: MIR_PLAN_* for the start, MIR_CART_* (include/mirigid.h)
CART_TOO_MANY_POINTS, CART_NOT_FINITE, CART_IK_FAILED, CART_JOINT_JUMP, CART_BLOCKED, CART_BLOCKED_SELF = range(16, 22)


class MirCartQuery(C.Structure):
    """include/mirigid.h: MirCartQuery (mir_cartesian_path)"""
    _fields_ = [
        ("struct_size", C.c_int32),
        ("link_body", C.c_int32),
        ("num_targets", C.c_int32),
        ("max_points", C.c_int32),
        ("num_waypoints", C.c_int32),
        ("flags", C.c_uint32),
        ("max_pos_step", C.c_float),
        ("max_rot_step", C.c_float),
        ("jump_threshold", C.c_float),
    ]


def make_cart_query(link_body: int, num_targets: int, max_points: int = 256, num_waypoints: int = 0, max_pos_step: float = 0.01,
                    max_rot_step: float = 0.05, jump_threshold: float = 0.5) -> MirCartQuery:
    """link_body: the body that follows the line; steps in metres / radians between two samples; jump_threshold per sample and joint."""
    q = MirCartQuery()
    q.struct_size = C.sizeof(MirCartQuery)
    q.link_body, q.num_targets, q.max_points, q.num_waypoints, q.flags = int(link_body), int(num_targets), int(max_points), int(num_waypoints), 0
    q.max_pos_step, q.max_rot_step, q.jump_threshold = float(max_pos_step), float(max_rot_step), float(jump_threshold)
    return q


BLEND_STATUS = {0: "OK", 2: "START_IN_COLLISION", 7: "START_IN_SELF_COLLISION", 32: "NO_MOTION", 33: "NOT_FINITE",
                34: "TOO_MANY_POINTS"}   # mir_blend_path: MIR_PLAN_* for the start, MIR_BLEND_* (include/mirigid.h)
BLEND_NO_MOTION, BLEND_NOT_FINITE, BLEND_TOO_MANY_POINTS = range(32, 35)


class MirBlendQuery(C.Structure):
    """include/mirigid.h: MirBlendQuery (mir_blend_path)"""
    _fields_ = [
        ("struct_size", C.c_int32),
        ("num_nodes", C.c_int32),
        ("blend_points", C.c_int32),
        ("max_shrinks", C.c_int32),
        ("max_points", C.c_int32),
        ("num_waypoints", C.c_int32),
        ("flags", C.c_uint32),
        ("max_deviation", C.c_float),
    ]


def blend_max_points(num_nodes: int, blend_points: int) -> int:
    """the dense points a polyline of `num_nodes` nodes can need: 2 + (K - 2)(m + 1)"""
    return 2 + max(int(num_nodes) - 2, 0) * (int(blend_points) + 1)


def make_blend_query(num_nodes: int, max_deviation: float = 0.05, blend_points: int = 8, max_shrinks: int = 4, max_points=None,
                     num_waypoints: int = 0) -> MirBlendQuery:
    """max_deviation: the blend's largest L2 distance from its corner; blend_points chords per blend; max_points None: the worst case."""
    q = MirBlendQuery()
    q.struct_size = C.sizeof(MirBlendQuery)
    q.num_nodes, q.blend_points, q.max_shrinks, q.num_waypoints, q.flags = int(num_nodes), int(blend_points), int(max_shrinks), int(num_waypoints), 0
    q.max_points = blend_max_points(num_nodes, blend_points) if max_points is None else int(max_points)
    q.max_deviation = float(max_deviation)
    return q


OPT_STATUS = {0: "OK", 48: "BLOCKED", 49: "BLOCKED_SELF", 50: "NOT_FINITE", 51: "NO_MOTION", 52: "OUT_OF_LIMITS"}   # mir_optimize_path
OPT_BLOCKED, OPT_BLOCKED_SELF, OPT_NOT_FINITE, OPT_NO_MOTION, OPT_OUT_OF_LIMITS = range(48, 53)
OPT_STOP = {0: "NONE", 1: "ITERATIONS", 2: "CONVERGED", 3: "STALLED"}
OPT_STOP_NONE, OPT_STOP_ITERATIONS, OPT_STOP_CONVERGED, OPT_STOP_STALLED = range(4)
# the defaults of optimize_path: parameters, chosen on the float64 reference (Trajectory optimisation, "the defaults")
OPT_DEFAULTS = dict(smooth_weight=1.0, obstacle_weight=5.0, activation=0.05, step=0.25, max_iterations=50, max_halvings=6, ftol=1e-4)


class MirOptQuery(C.Structure):
    """include/mirigid.h: MirOptQuery (mir_optimize_path)"""
    _fields_ = [
        ("struct_size", C.c_int32),
        ("num_waypoints", C.c_int32),
        ("max_iterations", C.c_int32),
        ("max_halvings", C.c_int32),
        ("flags", C.c_uint32),
        ("smooth_weight", C.c_float),
        ("obstacle_weight", C.c_float),
        ("step", C.c_float),
        ("activation", C.c_float),
        ("ftol", C.c_float),
    ]


def make_opt_query(num_waypoints: int, smooth_weight=None, obstacle_weight=None, activation=None, step=None, max_iterations=None,
                   max_halvings=None, ftol=None) -> MirOptQuery:
    """None: the value of OPT_DEFAULTS"""
    given = dict(smooth_weight=smooth_weight, obstacle_weight=obstacle_weight, activation=activation, step=step, max_iterations=max_iterations,
                 max_halvings=max_halvings, ftol=ftol)
    v = {k: OPT_DEFAULTS[k] if x is None else x for k, x in given.items()}
    q = MirOptQuery()
    q.struct_size = C.sizeof(MirOptQuery)
    q.num_waypoints, q.max_iterations, q.max_halvings, q.flags = int(num_waypoints), int(v["max_iterations"]), int(v["max_halvings"]), 0
    q.smooth_weight, q.obstacle_weight, q.step = float(v["smooth_weight"]), float(v["obstacle_weight"]), float(v["step"])
    q.activation, q.ftol = float(v["activation"]), float(v["ftol"])
    return q


CERT_STATUS = {0: "CLEAR", 1: "UNDECIDED", 2: "DEPTH", 3: "BUDGET", 4: "BLOCKED", 5: "NOT_FINITE"}   # mir_certify_path, by severity
CERT_CLEAR, CERT_UNDECIDED, CERT_DEPTH, CERT_BUDGET, CERT_BLOCKED, CERT_NOT_FINITE = range(6)
CERT_BRACKET = 1


class MirCertQuery(C.Structure):
    """include/mirigid.h: MirCertQuery (mir_certify_path, mir_certify_path_self, mir_certify_path_carry)"""
    _fields_ = [
        ("struct_size", C.c_int32),
        ("num_points", C.c_int32),
        ("max_depth", C.c_int32),
        ("max_evaluations", C.c_int32),
        ("max_leaves", C.c_int32),
        ("flags", C.c_uint32),
        ("tol", C.c_float),
        ("guard", C.c_float),
    ]


def make_cert_query(num_points: int, tol: float = 0.002, guard: float = 1e-5, max_depth: int = 12, max_evaluations: int = 4096,
                    bracket: bool = False, max_leaves: int = 0) -> MirCertQuery:
    """tol: the width a bracket is closed to; guard: subtracted from every bound; bracket: close every bracket, not only decide the margin."""
    q = MirCertQuery()
    q.struct_size = C.sizeof(MirCertQuery)
    q.num_points, q.max_depth, q.max_evaluations, q.max_leaves = int(num_points), int(max_depth), int(max_evaluations), int(max_leaves)
    q.flags = CERT_BRACKET if bracket else 0
    q.tol, q.guard = float(tol), float(guard)
    return q


IK_DEFAULTS = dict(max_iters=20, respect_joint_limit=1, damping=0.05, pos_tol=5e-4, rot_tol=5e-3, max_step=0.5)

RENDER_PER_ENV, RENDER_GLOBAL = 0, 1


def make_camera(width, height, pos, lookat, fov, up=(0.0, 0.0, 1.0)) -> MirCameraSpec:
    c = MirCameraSpec()
    c.width, c.height, c.fov_deg = int(width), int(height), float(fov)
    c.pos[:], c.lookat[:], c.up[:] = [float(v) for v in pos], [float(v) for v in lookat], [float(v) for v in up]
    return c


def quat_normalize(q: Sequence[float]) -> tuple:
    n = math.sqrt(sum(x * x for x in q))
    return tuple(x / n for x in q)


def box_hull_vertices(half: Sequence[float]) -> list:
    """The 8 corners of a box as hull vertices, in the corner order of the plane - box narrowphase (bit 0 = +x, bit 1 = +y,
    bit 2 = +z): a GEOM_HULL of these reproduces the GEOM_BOX contact points."""
    return [((1 if c & 1 else -1) * half[0], (1 if c & 2 else -1) * half[1], (1 if c & 4 else -1) * half[2]) for c in range(8)]


def icosphere_vertices(radius: float, level: int = 0) -> list:
    """Vertices on the sphere of `radius`: the icosahedron's 12 (level 0), or those plus its 20 face centres pushed out to the
    sphere (level 1: 32 vertices = MIR_MAX_HULL_VERT, the pentakis dodecahedron)."""
    t = (1.0 + 5 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    norm = lambda p: tuple(radius * c / (p[0] ** 2 + p[1] ** 2 + p[2] ** 2) ** 0.5 for c in p)  # noqa: E731
    out = [norm(p) for p in v]
    if level >= 1:
        out += [norm(tuple(v[a][i] + v[b][i] + v[c][i] for i in range(3))) for a, b, c in f]
    return out


def box_inertia(mass: float, half: Sequence[float]) -> tuple:
    """Solid-box inertia about its centre, (xx, yy, zz, xy, xz, yz)."""
    x, y, z = (2 * h for h in half)
    return (mass * (y * y + z * z) / 12, mass * (x * x + z * z) / 12, mass * (x * x + y * y) / 12, 0.0, 0.0, 0.0)


def sphere_inertia(mass: float, radius: float) -> tuple:
    i = 0.4 * mass * radius * radius
    return (i, i, i, 0.0, 0.0, 0.0)


def capsule_inertia(mass: float, radius: float, half: float) -> tuple:
    """Solid capsule (cylinder of length 2 half + two hemispherical caps) of total mass `mass`, axis z, about its centre."""
    r, h = radius, 2.0 * half
    vc, vs = math.pi * r * r * h, 4.0 / 3.0 * math.pi * r ** 3
    mc, ms = mass * vc / (vc + vs), mass * vs / (vc + vs)
    izz = 0.5 * mc * r * r + 0.4 * ms * r * r
    ixx = mc * (h * h / 12 + r * r / 4) + ms * (0.4 * r * r + h * h / 4 + 3.0 / 8.0 * h * r)
    return (ixx, ixx, izz, 0.0, 0.0, 0.0)


class SceneBuilder:
    """Accumulates bodies / dofs / geoms, then emits a MirSceneSpec.

    Body 0 is the world.  Names are kept host-side only (``get_link`` lookups).
    """

    def __init__(self):
        self.bodies: List[dict] = [dict(name="world", parent=0, jtype=JNT_FIXED, pos=(0, 0, 0), quat=(1, 0, 0, 0),
                                        axis=(0, 0, 1), mass=0.0, ipos=(0, 0, 0), inertia=(0,) * 6)]
        self.dofs: List[dict] = []
        self.geoms: List[dict] = []
        self.verts: List[tuple] = []   # vertex pool of the GEOM_HULL geoms
        self.dof_names: List[str] = []
        self.opt = dict(dt=0.01, gravity=(0.0, 0.0, -9.81), tolerance=1e-8, ls_tolerance=0.01, iterations=50,
                        ls_iterations=50, enable_collision=1, enable_joint_limit=1, enable_self_collision=0,
                        enable_adjacent_collision=0, max_contacts=K16_MAX_CONTACT, implicit_damping=1)
        self.task = dict(eef_body=0, obj_body=0, grip_dof=(), reward_z=0.1)

    # -- bodies -----------------------------------------------------------------------------
    def add_body(self, name: str, parent: str | int, pos=(0, 0, 0), quat=(1, 0, 0, 0), jtype=JNT_FIXED,
                 axis=(0, 0, 1), mass=0.0, ipos=(0, 0, 0), inertia=(0,) * 6, joint_name: Optional[str] = None,
                 **dof_kw) -> int:
        pidx = parent if isinstance(parent, int) else self.body_index(parent)
        idx = len(self.bodies)
        self.bodies.append(dict(name=name, parent=pidx, jtype=jtype, pos=tuple(pos), quat=quat_normalize(quat),
                                axis=tuple(axis), mass=float(mass), ipos=tuple(ipos), inertia=tuple(inertia)))
        ndof = {JNT_FIXED: 0, JNT_REVOLUTE: 1, JNT_PRISMATIC: 1, JNT_FREE: 6}[jtype]
        for k in range(ndof):
            d = dict(limited=0, ctrl_mode=CTRL_NONE, range=(0.0, 0.0), armature=0.0, damping=0.0, kp=0.0, kv=0.0,
                     frc_range=(-1e30, 1e30), solref=DEFAULT_SOLREF, solimp=DEFAULT_SOLIMP)
            if jtype != JNT_FREE:
                d.update(dof_kw)
            self.dofs.append(d)
            self.dof_names.append(joint_name or name if ndof == 1 else f"{name}/{k}")
        return idx

    def body_index(self, name: str) -> int:
        for i, b in enumerate(self.bodies):
            if b["name"] == name:
                return i
        raise KeyError(name)

    def dof_index(self, joint_name: str) -> int:
        return self.dof_names.index(joint_name)

    # -- geoms ------------------------------------------------------------------------------
    def add_geom(self, body: str | int, gtype: int, size=(0, 0, 0), pos=(0, 0, 0), quat=(1, 0, 0, 0),
                 friction=1.0, contype=1, conaffinity=1, solref=DEFAULT_SOLREF, solimp=DEFAULT_SOLIMP,
                 rgb=(0.8, 0.8, 0.8), vertices=None) -> int:
        bidx = body if isinstance(body, int) else self.body_index(body)
        if gtype == GEOM_HULL:
            verts = [tuple(float(c) for c in v) for v in vertices]
            if not 4 <= len(verts) <= MIR_MAX_HULL_VERT:
                raise ValueError("a hull geom takes 4 .. MIR_MAX_HULL_VERT vertices")
            if len(self.verts) + len(verts) > MIR_MAX_VERT:
                raise ValueError("scene exceeds MIR_MAX_VERT hull vertices")
            size = (float(len(self.verts)), float(len(verts)), 0.0)
            self.verts.extend(verts)
        self.geoms.append(dict(body=bidx, type=gtype, size=tuple(size), pos=tuple(pos), quat=quat_normalize(quat),
                               friction=float(friction), contype=contype, conaffinity=conaffinity,
                               solref=tuple(solref), solimp=tuple(solimp), rgb=tuple(rgb)))
        return len(self.geoms) - 1

    def visual(self, light_dir=(0.3, -0.4, 0.85), ambient=0.35, diffuse=0.65, sky_rgb=(0.55, 0.7, 0.9),
               checker_rgb=((0.82, 0.82, 0.82), (0.42, 0.42, 0.45)), checker_size=0.5, round_geoms=False) -> "MirVisualSpec":
        """Appearance used by mir_render: per-geom albedo from add_geom(rgb=...), one directional light.  round_geoms: draw spheres
        and capsules as themselves instead of their bounding boxes (MIR_VIS_ROUND_GEOMS)."""
        v = MirVisualSpec()
        v.struct_size = C.sizeof(MirVisualSpec)
        v.flags = MIR_VIS_ROUND_GEOMS if round_geoms else 0
        for i, g in enumerate(self.geoms):
            v.geom_rgb[i][:] = g["rgb"]
        v.light_dir[:] = light_dir
        v.ambient, v.diffuse, v.checker_size = ambient, diffuse, checker_size
        v.sky_rgb[:] = sky_rgb
        v.checker_rgb[0][:], v.checker_rgb[1][:] = checker_rgb[0], checker_rgb[1]
        return v

    # -- emit -------------------------------------------------------------------------------
    def build(self) -> MirSceneSpec:
        if len(self.bodies) > MIR_MAX_BODY or len(self.dofs) > MIR_MAX_DOF or len(self.geoms) > MIR_MAX_GEOM:
            raise ValueError("scene exceeds MIR_MAX_* capacity")
        s = MirSceneSpec()
        s.struct_size = C.sizeof(MirSceneSpec)
        s.version = MIR_VERSION
        s.nbody, s.ndof, s.ngeom = len(self.bodies), len(self.dofs), len(self.geoms)
        o = self.opt
        s.opt.dt = o["dt"]
        s.opt.gravity[:] = o["gravity"]
        for k in ("tolerance", "ls_tolerance", "iterations", "ls_iterations", "enable_collision", "enable_joint_limit",
                  "enable_self_collision", "enable_adjacent_collision", "max_contacts", "implicit_damping"):
            setattr(s.opt, k, o[k])
        t = self.task
        s.task.eef_body, s.task.obj_body = t["eef_body"], t["obj_body"]
        s.task.n_grip = len(t["grip_dof"])
        for i, g in enumerate(t["grip_dof"]):
            s.task.grip_dof[i] = g
        s.task.reward_z = t["reward_z"]
        s.task.obj2_body = t.get("obj2_body", -1)
        s.task.reward_mode = t.get("reward_mode", REWARD_LIFT)
        s.task.agent_mode = t.get("agent_mode", AGENT_EEF)
        s.task.reward_xy, s.task.reward_dz = t.get("reward_xy", 0.05), t.get("reward_dz", 0.03)
        for i, b in enumerate(self.bodies):
            sb = s.body[i]
            sb.parent, sb.jtype, sb.mass = b["parent"], b["jtype"], b["mass"]
            sb.pos[:], sb.quat[:], sb.axis[:] = b["pos"], b["quat"], b["axis"]
            sb.ipos[:], sb.inertia[:] = b["ipos"], b["inertia"]
        for i, d in enumerate(self.dofs):
            sd = s.dof[i]
            sd.limited, sd.ctrl_mode = d["limited"], d["ctrl_mode"]
            sd.range[:] = d["range"]
            sd.armature, sd.damping, sd.kp, sd.kv = d["armature"], d["damping"], d["kp"], d["kv"]
            sd.frc_range[:] = d["frc_range"]
            sd.solref[:], sd.solimp[:] = d["solref"], d["solimp"]
        for i, g in enumerate(self.geoms):
            sg = s.geom[i]
            sg.body, sg.type, sg.contype, sg.conaffinity = g["body"], g["type"], g["contype"], g["conaffinity"]
            sg.size[:], sg.pos[:], sg.quat[:] = g["size"], g["pos"], g["quat"]
            sg.friction = g["friction"]
            sg.solref[:], sg.solimp[:] = g["solref"], g["solimp"]
        s.nvert = len(self.verts)
        for i, v in enumerate(self.verts):
            s.vert[i][:] = v
        return s
