"""The cases of the self-collision tests, shared by tests/test_self_cpu.py (which holds the conditions the GPU tests lean on) and
tests/test_gpu_self.py.  A helper, no test.  B = 5 rows; states are SET.

The scene is the Franka of the pick scene with the ground and the cube (at plan_cases.CUBE; its geom is skipped, as the cube the hand
reaches for) and NO post: nothing of the scene is in the way.  The sphere model is the coarse one of plan_cases (SPACING) plus the
spheres of the bolted base, which take part in the self test only; the pair filter is the entity's own (EntityView.self_collision_model).

    "fold"   start and goal differ in joints 2 and 5: the straight segment stays >= 12 cm from the scene and folds the forearm into the
             upper arm and the base.
    "swing"  start and goal differ in joints 3 and 5: >= 6.7 cm from the scene, the hand swings through the base column.

Row 0 is the base pair; rows 1 - 4 add uniform +-0.04 rad jitter on the seven arm joints, as plan_cases does.  In float64, on every row:
both ends keep >= 2 cm from the scene and from the arm itself, the straight edge keeps >= 2 cm from the scene and reaches <= -1 cm
into the arm (tests/test_self_cpu.py asserts it).
"""
from __future__ import annotations

import functools

import numpy as np

import plan_cases as pc
import plan_ref
import self_ref
from gym_genesis.backend import models

B = pc.B
BUDGET, RESOLUTION, STEP, MARGIN, SELF_MARGIN = pc.BUDGET, pc.RESOLUTION, pc.STEP, 0.0, 0.0
PAIRS = {
    "fold": ((0.555, 1.615, 1.991, -2.857, 2.636, 1.037, -0.416, 0.04, 0.04), (0.555, -0.399, 1.991, -2.857, -2.142, 1.037, -0.416, 0.04, 0.04)),
    "swing": ((-2.846, 0.043, 1.69, -2.897, 1.211, 1.627, 0.05, 0.04, 0.04), (-2.846, 0.043, 0.184, -2.897, -1.463, 1.627, 0.05, 0.04, 0.04)),
}
# two configurations for the status tests (float64, any row's scene): IN_GROUND is 35 cm into the ground and 3.9 cm clear of itself,
# IN_BOTH 5 cm into the ground and 8 cm into itself
IN_GROUND = (-0.345, 1.603, -0.001, -1.795, 0.697, 3.734, 2.601, 0.04, 0.04)
IN_BOTH = (0.794, -0.812, -2.66, -3.022, 1.815, 3.424, 0.618, 0.04, 0.04)
JITTER_SEED = {"fold": 81, "swing": 88}   # (chosen so that every jittered row meets the conditions above; 83 left a goal at 1.9 cm)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(sb, spec, probes (N + E, 4), links (N + E,), n_extra, mask (32,), skip, qadr (D,), q (B, nq) float32 start rows,
    start (B, D), goal (B, D) float32)"""
    sb = models.franka_cube_pick_scene()
    spec = sb.build()
    robot = pc.arm(sb)
    probes, links, n_extra, mask = robot.self_collision_model(spacing=pc.SPACING)
    rng = np.random.default_rng(JITTER_SEED[name])
    jit = np.zeros((2, B, 9))
    jit[:, 1:, :7] = rng.uniform(-0.04, 0.04, (2, B - 1, 7))   # (row 0 is the base pair itself)
    start = (np.array(PAIRS[name][0]) + jit[0]).astype(np.float32)
    goal = (np.array(PAIRS[name][1]) + jit[1]).astype(np.float32)
    model = plan_ref.kin_ref.Model(spec)
    q = np.zeros((B, model.nq), np.float32)
    qadr = np.array(robot._qcols, np.int32)
    q[:, qadr] = start
    qa = model.qadr[sb.body_index("cube")]
    q[:, qa:qa + 7] = pc.CUBE
    cube_geoms = sum(1 << g for g, geom in enumerate(sb.geoms) if geom["body"] == sb.body_index("cube"))
    return dict(sb=sb, spec=spec, probes=probes, links=links, n_extra=n_extra, mask=mask, skip=robot._own_geoms() | cube_geoms, qadr=qadr, q=q,
                start=start, goal=goal)


def arm(c, mir=None):
    """the Franka as an entity view over the case's scene with the case's models in place"""
    robot = pc.arm(c["sb"], mir)
    robot.self_collision_model(spacing=pc.SPACING)
    return robot


def problem(name, dtype=np.float64, self_margin=SELF_MARGIN, mask=None, n_extra=None):
    c = case(name)
    return self_ref.SelfProblem(c["spec"], c["probes"], c["links"], c["qadr"], c["n_extra"] if n_extra is None else n_extra,
                                c["mask"] if mask is None else mask, c["skip"], 1.0, self_margin, 1.0, dtype)


@functools.lru_cache(maxsize=None)
def reference(name, row, seed=0, dtname="float64"):
    """self_ref.plan of one row of a case at the test budgets (computed once, shared)"""
    c = case(name)
    return self_ref.plan(problem(name, np.dtype(dtname).type), c["q"][row], c["goal"][row], row, margin=MARGIN, W=BUDGET["W"],
                         max_nodes=BUDGET["max_nodes"], max_iterations=BUDGET["max_iterations"], seed=seed, resolution=RESOLUTION, step=STEP)


def straight(name, row):
    """the configurations of the straight edge start -> goal (the start included), float64"""
    c = case(name)
    a, b = c["start"][row].astype(np.float64), c["goal"][row].astype(np.float64)
    return [a] + plan_ref.edge_samples(a, b, RESOLUTION, np.float64)


@functools.lru_cache(maxsize=None)
def deepest(name, row):
    """the configuration of the straight edge deepest in self-collision (float32, as a test hands it to the GPU)"""
    c = case(name)
    pb = problem(name)
    pb.set_row(c["q"][row])
    return min(straight(name, row), key=lambda q: pb.both(q)[1]).astype(np.float32)
