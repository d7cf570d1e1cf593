"""The scenes, seeds and probe sets of the signed-distance tests, shared by tests/test_dist_cpu.py (which holds the share of ambiguous
probes of every case under 2 %) and tests/test_gpu_distance.py.  A helper, no test.  The scenes, the seeded states and the float64 /
float32 oracle poses are those of tests/ray_cases.py (B = 5); states are SET, never simulated.
"""
from __future__ import annotations

import functools
import itertools

import numpy as np

import dist_ref
import kin_ref
import ray_cases
from gym_genesis.backend import models
from gym_genesis.tasks.views import EntityView

B = ray_cases.B
MAX_DISTANCE = 0.5
ZOO_BOX = ((-1.2, -0.9, -0.05), (1.2, 0.9, 1.4))
RADII = (0.0, 0.02, 0.05)
CANDIDATE_SEEDS = {"zoo": 51, "pick": 52, "stack": 53}


def _box_features(h):
    """unit directions from a box's centre to its 6 faces, 12 edges and 8 vertices, and a surface point of each (faces off-centre)"""
    out = []
    for sg in itertools.product((-1, 0, 1), repeat=3):
        if not any(sg):
            continue
        sg = np.array(sg, float)
        on = np.where(sg != 0, sg * h, np.array([0.03, 0.02, -0.025]))
        out.append((on, sg / np.linalg.norm(sg)))
    return out


def _hull_features(g):
    """(surface point, outward direction) of every face, edge and vertex of a hull geom of dist_ref.Scene"""
    v, (pn, pd) = g["verts"], g["planes"]
    tol = 1e-9
    on = [[i for i in range(len(v)) if abs(pn[f] @ v[i] - pd[f]) < tol] for f in range(len(pd))]
    out = [(v[ix].mean(0), pn[f]) for f, ix in enumerate(on)]
    for i, j in itertools.combinations(range(len(v)), 2):
        fs = [f for f, ix in enumerate(on) if i in ix and j in ix]
        if len(fs) == 2:
            n = pn[fs[0]] + pn[fs[1]]
            out.append((0.5 * (v[i] + v[j]), n / np.linalg.norm(n)))
    for i in range(len(v)):
        n = sum(pn[f] for f, ix in enumerate(on) if i in ix)
        out.append((v[i], n / np.linalg.norm(n)))
    return out


def _zoo_probes(c):
    """512 seeded uniform probes, half in the world and half riding on the zoo's bodies, then the hand-aimed ones -> probes, links,
    degenerate ((probe, geom) of the hand-aimed probes that have no unique answer where that geom wins)"""
    rng = np.random.default_rng(61)
    sb = c["sb"]
    lo, hi = np.array(ZOO_BOX[0]), np.array(ZOO_BOX[1])
    world = rng.uniform(lo, hi, (256, 3))
    # the riders: on the box, the sphere, the capsule and the box given as a hull.  None rides on the 60-face ball: next to it a tenth
    # of all uniform probes lies within the band where two of its faces are NEAR as nearest (dist_ref), which alone would take the
    # case past the 2 % of ambiguous probes tests/test_dist_cpu.py allows; the ball gets the world probes that fall next to it and a
    # hand-aimed probe at every face, edge and vertex and inside instead
    bodies = [sb.body_index(n) for n in ray_cases.ZOO_BODIES]
    ride = rng.uniform(-0.3, 0.3, (256, 3))   # (the geoms are 0.08 .. 0.2 across: inside and outside their own geom)
    probes = [np.append(p, rng.choice(RADII)) for p in world] + [np.append(p, rng.choice(RADII)) for p in ride]
    links = [0] * 256 + [bodies[i % 5] for i in range(256)]
    degenerate = []

    def add(p, link, flagged=False):
        if flagged:
            degenerate.append((len(probes), gi))
        probes.append(np.append(np.asarray(p, float), 0.0))
        links.append(link)

    scene = dist_ref.Scene(c["spec"])
    for gi, g in enumerate(scene.geoms):
        b = g["body"]
        if g["type"] == dist_ref.PLANE:
            add((0.3, 0.3, -0.03), 0)            # below the plane
            add((-0.9, 0.7, 0.0), 0)             # on it
            continue
        # the centre: no unique normal for a sphere, a capsule's axis, the ball (every face equally far)
        add((0, 0, 0), b, flagged=g["type"] in (dist_ref.SPHERE, dist_ref.CAPSULE) or (g["type"] == dist_ref.HULL and len(g["verts"]) > 8))
        if g["type"] == dist_ref.SPHERE:
            add((0, g["size"][0], 0), b)
        elif g["type"] == dist_ref.CAPSULE:
            add((g["size"][0], 0, 0.05), b)
            add((0, 0, 0.1), b, flagged=True)    # on the axis
        elif g["type"] == dist_ref.BOX:
            h = g["size"]
            add((h[0] - 0.05, h[1] - 0.05, 0.0), b, flagged=True)   # an inside bisector
            for on, out in _box_features(h):
                add(on + 1e-3 * out, b)
            add((h[0], 0.03, 0.02), b, flagged=True)                # on the surface
        else:
            feats = _hull_features(g)
            for on, out in feats:
                add(on + 1e-3 * out, b)
            for on, _ in feats[:4]:
                add(0.7 * on, b)                                     # inside, under one face
            add(feats[0][0], b, flagged=True)                        # on the surface
    return np.array(probes, np.float32), np.array(links, np.int32), np.array(degenerate)


def arm(name):
    """the Franka of a pick / stack case as an entity view without a scene behind it (the sphere model is host-side)"""
    return EntityView(None, ray_cases.case(name)["sb"], "link0", models.FRANKA_JOINTS)


def _arm_probes(c, name):
    """the arm's collision_spheres() and a 6 x 6 x 4 world grid of points over the table area; the arm's geoms are skipped"""
    robot = arm(name)
    p, lk = robot.collision_spheres()
    z0 = 0.0 if name == "pick" else models.ISLAND_TOP_Z
    grid = np.array([(x, y, z, 0.0) for x in np.linspace(0.15, 0.85, 6) for y in np.linspace(-0.33, 0.33, 6) for z in np.linspace(z0 - 0.02, z0 + 0.3, 4)])
    return np.concatenate([p, grid.astype(np.float32)]), np.concatenate([lk, np.zeros(len(grid), np.int32)]), robot._own_geoms(), len(p)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> the dict of ray_cases.case(name) plus dscene (dist_ref.Scene), probes (N, 4) float32, links (N,) int32, skip, max_distance,
    degenerate (zoo: (probe, geom) of the hand-aimed probes without a unique answer), n_arm (pick / stack: the leading arm spheres)"""
    c = dict(ray_cases.case(name))
    c["dscene"] = dist_ref.Scene(c["spec"])
    c["max_distance"] = MAX_DISTANCE
    if name == "zoo":
        c["probes"], c["links"], c["degenerate"] = _zoo_probes(c)
        c["skip"], c["n_arm"] = 0, 0
    else:
        c["probes"], c["links"], c["skip"], c["n_arm"] = _arm_probes(c, name)
        c["degenerate"] = np.zeros((0, 2), int)
    return c


@functools.lru_cache(maxsize=None)
def candidate(name):
    """a second seeded configuration that differs from the state in every joint and in the free bodies' poses, with its oracle poses
    -> dict(q, xp, xq, xp32, xq32)"""
    c = ray_cases.case(name)
    box = ((-0.7, -0.7, 0.45), (0.7, 0.7, 1.3)) if name == "zoo" else ((-0.3, -0.3, 0.05), (0.7, 0.3, 0.9))
    q, _ = kin_ref.random_state(c["spec"], kin_ref.Model(c["spec"]), B, seed=CANDIDATE_SEEDS[name], cube_box=box)
    xp, xq = ray_cases.poses(c["spec"], q)
    xp32, xq32 = ray_cases.poses(c["spec"], q, f32=True if name == "pick" else "big")
    return dict(q=q, xp=xp, xq=xq, xp32=xp32, xq32=xq32)


def reference(name, at="state", dtype=np.float64):
    """dist_ref of a case on all B envs, at the case's state or at its candidate configuration: float64 on the oracle's poses, or the
    float32 port on the float32 oracle's"""
    return _reference(name, at, np.dtype(dtype).name)


@functools.lru_cache(maxsize=None)
def _reference(name, at, dtname):
    c = case(name)
    src = c if at == "state" else candidate(name)
    f32 = dtname == "float32"
    return dist_ref.signed_distance(c["dscene"], src["xp32"] if f32 else src["xp"], src["xq32"] if f32 else src["xq"], c["probes"], c["links"],
                                    c["max_distance"], c["skip"], np.float32 if f32 else np.float64, with_ambiguous=not f32)
