"""The scenes, start rows and goals of the motion-planning tests, shared by tests/test_plan_cpu.py (which holds the conditions the GPU
tests lean on) and tests/test_gpu_plan.py.  A helper, no test.  B = 5 rows, built with the project's SceneBuilder; states are SET.

    "post"    the Franka of the pick scene, the ground, the cube and one fixed box post between a start and a goal that differ mainly in
              joint 1: start and goal are clear by >= 2 cm, the straight segment penetrates the post by >= 1 cm (float64).
    "clear"   the same scene and starts with a goal whose straight edge is clear by >= 2 cm.
    "sealed"  two fixed half walls in the plane y = 0 from the ground to above the arm's reach, with a slot about the base's axis that
              only the base column fits: the goal configuration (the mirror image of the start) is clear, but nothing leads there.

The sphere model is the entity's own (EntityView.collision_spheres) at a coarser spacing, so that the NumPy reference stays fast.
"""
from __future__ import annotations

import functools

import numpy as np

import plan_ref
from gym_genesis.backend import models
from gym_genesis.backend import spec as S
from gym_genesis.tasks.views import EntityView

B = 5
SPACING = 0.12
BUDGET = dict(max_nodes=128, max_iterations=512, W=16)
RESOLUTION, STEP, MARGIN = 0.05, 0.3, 0.0
POST = dict(size=(0.04, 0.04, 0.25), pos=(0.45, 0.0, 0.25))
WALLS = (dict(size=(1.0, 0.005, 1.0), pos=(1.11, 0.0, 1.0)), dict(size=(1.0, 0.005, 1.0), pos=(-1.11, 0.0, 1.0)))
START = (-0.9, -0.4, 0.0, -2.2, 0.0, 2.0, 0.8, 0.04, 0.04)
GOAL = (0.9, -0.35, 0.05, -2.1, 0.0, 1.9, 0.7, 0.04, 0.04)
CLEAR_GOAL = (-1.4, -0.2, 0.1, -1.9, 0.1, 1.8, 0.6, 0.02, 0.02)
SEALED_START = (-1.3, -0.4, 0.0, -2.2, 0.0, 2.0, 0.8, 0.04, 0.04)
SEALED_GOAL = (1.3, -0.4, 0.0, -2.2, 0.0, 2.0, 0.8, 0.04, 0.04)
CUBE = (0.65, 0.0, 0.02, 1.0, 0.0, 0.0, 0.0)


def builder(name):
    sb = models.franka_cube_pick_scene()
    for box in (WALLS if name == "sealed" else (POST,)):
        sb.add_geom(0, S.GEOM_BOX, size=box["size"], pos=box["pos"], rgb=(0.5, 0.5, 0.55))
    return sb


def arm(sb, mir=None):
    """the Franka as an entity view (without a scene behind it: the sphere model is host-side) with the coarse sphere model in place"""
    robot = EntityView(mir, sb, "link0", models.FRANKA_JOINTS)
    robot.set_collision_spheres(*robot.collision_spheres(spacing=SPACING))
    return robot


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(sb, spec, probes (N, 4), links (N,), skip, qadr (D,), q (B, nq) float32 start rows, start (B, D), goal (B, D) float32)"""
    sb = builder(name)
    spec = sb.build()
    robot = arm(sb)
    probes, links = robot.collision_spheres()
    rng = np.random.default_rng({"post": 71, "clear": 71, "sealed": 73}[name])
    base_s, base_g = {"post": (START, GOAL), "clear": (START, CLEAR_GOAL), "sealed": (SEALED_START, SEALED_GOAL)}[name]
    jit = np.zeros((2, B, 9))
    jit[:, 1:, :7] = rng.uniform(-0.04, 0.04, (2, B - 1, 7))   # (row 0 is the base pair itself)
    start = (np.array(base_s) + jit[0]).astype(np.float32)
    goal = (np.array(base_g) + (jit[0] if name == "sealed" else jit[1]) * ([-1] + [1] * 8 if name == "sealed" else 1)).astype(np.float32)
    model = plan_ref.kin_ref.Model(spec)
    q = np.zeros((B, model.nq), np.float32)
    qadr = np.array(robot._qcols, np.int32)
    q[:, qadr] = start
    qa = model.qadr[sb.body_index("cube")]
    q[:, qa:qa + 7] = CUBE
    return dict(sb=sb, spec=spec, probes=probes, links=links, skip=robot._own_geoms(), qadr=qadr, q=q, start=start, goal=goal)


def problem(name, dtype=np.float64, skip=None):
    c = case(name)
    return plan_ref.Problem(c["spec"], c["probes"], c["links"], c["qadr"], c["skip"] if skip is None else skip, 1.0, dtype)


@functools.lru_cache(maxsize=None)
def reference(name, row, seed=0, dtname="float64", smooth_passes=64, max_nodes=BUDGET["max_nodes"], max_iterations=BUDGET["max_iterations"],
              margin=MARGIN):
    """plan_ref.plan of one row of a case at the test budgets (computed once, shared)"""
    c = case(name)
    return plan_ref.plan(problem(name, np.dtype(dtname).type), c["q"][row], c["goal"][row], row, W=BUDGET["W"], max_nodes=max_nodes,
                         max_iterations=max_iterations, smooth_passes=smooth_passes, seed=seed, resolution=RESOLUTION, step=STEP, margin=margin)


def valid_polyline(name, row, poly, margin=MARGIN, tol=0.0):
    """the validator: every edge of the polyline, sampled by the edge rule in float64, keeps clearance >= margin - tol; it starts at the
    row's start and ends at its goal -> (ok, lowest clearance)"""
    c = case(name)
    poly = np.asarray(poly, np.float64)
    seg, _ = plan_ref.polyline_clearance(problem(name), c["q"][row], poly, RESOLUTION)
    ends = np.array_equal(poly[0].astype(np.float32), c["start"][row]) and np.array_equal(poly[-1].astype(np.float32), c["goal"][row])
    return bool(ends and seg.min() >= margin - tol), float(seg.min())
