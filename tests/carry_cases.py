"""The cases of the carried-object tests, shared by tests/test_carry_cpu.py (which holds the conditions the GPU tests lean on) and
tests/test_gpu_carry.py.  A helper, no test.  B = 5 rows; states are SET; budgets, resolution and sphere spacing are those of
plan_cases.py.  The arm is the Franka of the pick scene with the coarse sphere model of plan_cases (SPACING), the attach link is the
hand, and the model handed to the library is EntityView.carried_model(): arm spheres, the carried body's spheres (its own
collision_spheres()), the spheres of the bolted base behind them; the pair filter holds the carried body against the default links
only (arm against arm is off).

    "under"  the pick scene plus a fixed post whose top passes UNDER the hand on the straight edge (joint 1 sweeps the hand across it;
             rows differ in joint 1).  The cube sits between the finger pads, centred 2 mm beyond the finger tips, so its sphere hangs
             about 3.5 cm below the arm's lowest sphere; each row has its own small grasp offset and yaw.  In float64, on every row:
             start and goal are clear by >= 2 cm with the carried spheres; on the straight edge the arm's own spheres keep >= 1 cm
             (the plain planner returns the straight line) and the carried spheres penetrate the post by >= 1 cm.
    "rod"    the pick scene (cube at plan_cases.CUBE, its geom skipped) plus a free box of 4 x 4 x 30 cm, held across the finger pads
             with its long axis along the hand's x; nothing of the scene is in the way (>= 2 cm everywhere).  The elbow is folded and
             the straight edge turns joint 5 by 3.6 rad, which sweeps the rod at least 1 cm into the spheres of links that
             attached_links_default() enables; start and goal are clear of the scene and of the arm by >= 2 cm.

The carried body's start pose is computed in float64 from the hand's pose at each start row and the row's nominal grasp (`grasp`), then
stored in the float32 row: with grasp = NULL the kernel recovers it from there.
"""
from __future__ import annotations

import functools

import numpy as np

import carry_ref
import plan_cases as pc
import plan_ref
from gym_genesis.backend import models
from gym_genesis.backend import spec as S
from gym_genesis.tasks.views import EntityView

B = pc.B
BUDGET, RESOLUTION, STEP, MARGIN, SELF_MARGIN = pc.BUDGET, pc.RESOLUTION, pc.STEP, 0.0, 0.0
NAMES = ("under", "rod")
CARRIED = {"under": "cube", "rod": "rod"}
UNDER_POST = dict(size=(0.04, 0.04, 0.2175), pos=(0.48, 0.0, 0.2175))   # (top at z = 0.435)
ROD_HALF = (0.02, 0.02, 0.15)
PAIRS = {
    "under": (pc.START, pc.GOAL),
    "rod": ((0.0, -0.3, 0.0, -2.782, 1.309, 0.873, 2.405, 0.04, 0.04), (0.0, -0.3, 0.0, -2.782, -2.313, 0.593, 2.405, 0.04, 0.04)),
}
# the nominal grasp of each row: offset of the carried body's centre from (0, 0, GRASP_Z) in the hand's frame, yaw about the hand's z
GRASP_Z = 0.119
OFFSETS = ((0.0, 0.0, 0.0, 0.0), (0.002, 0.001, 0.002, 0.15), (-0.002, -0.001, 0.001, -0.2), (0.001, -0.002, 0.003, 0.3), (-0.001, 0.002, -0.001, -0.1))
JITTER_SEED = {"under": 91, "rod": 92}


def builder(name):
    sb = models.franka_cube_pick_scene()
    if name == "under":
        sb.add_geom(0, S.GEOM_BOX, size=UNDER_POST["size"], pos=UNDER_POST["pos"], rgb=(0.5, 0.5, 0.55))
    else:
        mass = 200.0 * 8.0 * ROD_HALF[0] * ROD_HALF[1] * ROD_HALF[2]
        sb.add_body("rod", 0, pos=(0.0, 0.6, 0.02), quat=(1, 0, 0, 0), jtype=S.JNT_FREE, mass=mass, inertia=models.box_inertia(mass, ROD_HALF))
        sb.add_geom("rod", S.GEOM_BOX, size=ROD_HALF, rgb=(0.2, 0.4, 0.8))
    return sb


def views(name, sb, mir=None):
    """(the Franka with the coarse models in place, the carried entity, the cube) as entity views over the case's scene"""
    robot = pc.arm(sb, mir)
    robot.self_collision_model(spacing=pc.SPACING)
    return robot, EntityView(mir, sb, CARRIED[name], ()), EntityView(mir, sb, "cube", ())


def nominal_grasp(name, row):
    """(7,) float64: the carried body in the hand's frame"""
    dx, dy, dz, yaw = OFFSETS[row]
    qz = np.array([np.cos(0.5 * yaw), 0.0, 0.0, np.sin(0.5 * yaw)])
    if name == "rod":   # (the rod's long axis, its z, along the hand's x: a quarter turn about y, then the yaw about the hand's z)
        qz = plan_ref._qmul(qz, np.array([np.sqrt(0.5), 0.0, np.sqrt(0.5), 0.0]))
        dx = 10.0 * dx   # (the rod sticks out further on one side, differently per row)
    return np.concatenate([[dx, dy, GRASP_Z + dz], qz])


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(sb, spec, probes (N + E, 4), links (N + E,), n_extra, mask (32,), n_arm (the arm's spheres in front of the carried ones),
    body C, link Lk, skip (the arm's, the carried body's and, in "rod", the cube's geoms: also what ignore_entities gives the plain planner),
    qadr (D,), q (B, nq) float32 start rows, start (B, D), goal (B, D) float32, grasp (B, 7) float64)"""
    sb = builder(name)
    spec = sb.build()
    robot, obj, cube = views(name, sb)
    probes, links, n_extra, mask, C, Lk = robot.carried_model(obj, "hand", self_collision=False)
    n_arm = len(robot.collision_spheres()[1])
    rng = np.random.default_rng(JITTER_SEED[name])
    jit = np.zeros((2, B, 9))
    jit[:, 1:, 0] = rng.uniform(-0.04, 0.04, (2, B - 1))   # (row 0 is the base pair itself; joint 1 turns the arm about the vertical)
    start = (np.array(PAIRS[name][0]) + jit[0]).astype(np.float32)
    goal = (np.array(PAIRS[name][1]) + jit[1]).astype(np.float32)
    model = plan_ref.kin_ref.Model(spec)
    q = np.zeros((B, model.nq), np.float32)
    qadr = np.array(robot._qcols, np.int32)
    q[:, qadr] = start
    qa = model.qadr[sb.body_index("cube")]
    q[:, qa:qa + 7] = pc.CUBE
    q[:, model.qadr[C] + 3] = 1.0
    skip = robot._own_geoms() | obj._own_geoms() | (cube._own_geoms() if name == "rod" else 0)
    fk = plan_ref.Problem(spec, probes[:1], links[:1], qadr, skip, 1.0, np.float64)
    grasp = np.stack([nominal_grasp(name, r) for r in range(B)])
    qc = model.qadr[C]
    for r in range(B):   # the carried body where the hand and the nominal grasp put it
        fk.set_row(q[r])
        q[r, qc:qc + 3] = fk.xp[Lk] + plan_ref._qrot(fk.xq[Lk], grasp[r, :3])
        q[r, qc + 3:qc + 7] = plan_ref._qmul(fk.xq[Lk], grasp[r, 3:])
    return dict(sb=sb, spec=spec, probes=probes, links=links, n_extra=n_extra, mask=mask, n_arm=n_arm, body=C, link=Lk, skip=skip, qadr=qadr, q=q,
                start=start, goal=goal, grasp=grasp)


def problem(name, dtype=np.float64, mask=None):
    c = case(name)
    return carry_ref.CarryProblem(c["spec"], c["probes"], c["links"], c["qadr"], c["n_extra"], c["mask"] if mask is None else mask, c["body"],
                                  c["link"], c["skip"], 1.0, SELF_MARGIN, 1.0, dtype)


def plain_problem(name, dtype=np.float64):
    """the arm alone, the carried body ignored: what plan_path(ignore_entities=(carried,)) tests"""
    c = case(name)
    return plan_ref.Problem(c["spec"], c["probes"][:c["n_arm"]], c["links"][:c["n_arm"]], c["qadr"], c["skip"], 1.0, dtype)


@functools.lru_cache(maxsize=None)
def reference(name, row, seed=0, dtname="float64"):
    """self_ref.plan of one row with the carried body attached (grasp from the start row), at the test budgets (computed once, shared)"""
    c = case(name)
    return carry_ref.self_ref.plan(problem(name, np.dtype(dtname).type), c["q"][row], c["goal"][row], row, margin=MARGIN, W=BUDGET["W"],
                                   max_nodes=BUDGET["max_nodes"], max_iterations=BUDGET["max_iterations"], seed=seed, resolution=RESOLUTION, step=STEP)


def straight(name, row):
    """the configurations of the straight edge start -> goal (the start included), float64"""
    c = case(name)
    a, b = c["start"][row].astype(np.float64), c["goal"][row].astype(np.float64)
    return [a] + plan_ref.edge_samples(a, b, RESOLUTION, np.float64)


def valid_polyline(name, row, poly, tol=0.0):
    """the validator: every edge of the polyline, sampled by the edge rule in float64 with the carried body attached, keeps the scene
    clearance >= MARGIN - tol and the carried-against-arm clearance >= SELF_MARGIN - tol; it starts at the row's start and ends at its
    goal -> (ok, lowest scene clearance, lowest self clearance, the samples)"""
    c = case(name)
    poly = np.asarray(poly, np.float64)
    seg, seg_self, samples = carry_ref.self_ref.polyline_clearances(problem(name), c["q"][row], poly, RESOLUTION)
    ends = np.array_equal(poly[0].astype(np.float32), c["start"][row]) and np.array_equal(poly[-1].astype(np.float32), c["goal"][row])
    return bool(ends and seg.min() >= MARGIN - tol and seg_self.min() >= SELF_MARGIN - tol), float(seg.min()), float(seg_self.min()), samples
