"""Five synthetic scenes for the query kernels (mir_link_kinematics, mir_link_accelerations, mir_dynamics, mir_task_dynamics): trees the
two Franka scenes never show them.  A helper, no test.  Deterministic, `SceneBuilder` only, a ground plane and no other geometry; nothing
is ever stepped.

Every joint body draws from np.random.default_rng(seed): a unit quat, a unit oblique axis, pos in +-0.2, ipos in +-0.05, mass in 0.2 .. 2,
a full six-entry inertia (the principal moments of a box with half extents in 0.02 .. 0.12, turned by a random rotation), limited = 1 with
range +-2 rad (revolute) or +-0.15 m (prismatic), armature in 0 .. 0.1, CTRL_POSITION with kp 50 .. 500, kv 5 .. 50 and a force range of
+-40, so that `ctrl_force` clamps on some dofs and not on others (dyn_ref.random_targets_and_acc).

    oblique_chain  fixed base (rotated, offset), below it R P R F R P R R F P                     nbody 12, nv  8   16-lane model
    deep           one chain of 15 joint bodies, prismatic at every fourth                          nbody 16, nv 15   16-lane model
    bushy          a revolute root, then a binary tree three levels deep, mixed R / P               nbody 16, nv 15   16-lane model
    floating       a free root (mass 3, ipos != 0, full inertia), three limbs of three joints       nbody 11, nv 15   16-lane model
    many           bodies 1-9 the chain F R P R F R R P R; body 10 a free root with limbs of 2 and  nbody 17, nv 24   wave model
                   3 joints (bodies 11-15); body 16 a free 4 cm cube
"""
from __future__ import annotations

import numpy as np

from gym_genesis.backend.spec import CTRL_POSITION, GEOM_PLANE, JNT_FIXED, JNT_FREE, JNT_PRISMATIC, JNT_REVOLUTE, SceneBuilder, box_inertia

CASES = ("oblique_chain", "deep", "bushy", "floating", "many")
KERNEL = dict(oblique_chain=16, deep=16, bushy=16, floating=16, many=64)
DIMS = dict(oblique_chain=(12, 8), deep=(16, 15), bushy=(16, 15), floating=(11, 15), many=(17, 24))   # (nbody, nv)
SEED = dict(oblique_chain=101, deep=102, bushy=103, floating=104, many=105)
F, R, P = JNT_FIXED, JNT_REVOLUTE, JNT_PRISMATIC


def _unit(rng, n):
    u = rng.normal(size=n)
    return u / np.linalg.norm(u)


def _rot(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _inertial(rng, mass=None):
    """mass, ipos, (xx, yy, zz, xy, xz, yz) of a box turned by a random rotation"""
    mass = float(rng.uniform(0.2, 2.0)) if mass is None else float(mass)
    ipos = tuple(rng.uniform(-0.05, 0.05, 3))
    Rm = _rot(_unit(rng, 4))
    I = Rm @ np.diag(box_inertia(mass, rng.uniform(0.02, 0.12, 3))[:3]) @ Rm.T
    return dict(mass=mass, ipos=ipos, inertia=(I[0, 0], I[1, 1], I[2, 2], I[0, 1], I[0, 2], I[1, 2]))


def _body(sb, rng, name, parent, jtype):
    """one body of a tree: fixed, revolute or prismatic, everything random"""
    kw = dict(pos=tuple(rng.uniform(-0.2, 0.2, 3)), quat=tuple(_unit(rng, 4)), jtype=jtype, **_inertial(rng))
    if jtype != F:
        lim = 2.0 if jtype == R else 0.15
        kw.update(axis=tuple(_unit(rng, 3)), limited=1, range=(-lim, lim), armature=float(rng.uniform(0.0, 0.1)), ctrl_mode=CTRL_POSITION,
                  kp=float(rng.uniform(50.0, 500.0)), kv=float(rng.uniform(5.0, 50.0)), frc_range=(-40.0, 40.0))
    return sb.add_body(name, parent, **kw)


def _chain(sb, rng, prefix, parent, kinds):
    for i, jt in enumerate(kinds):
        parent = _body(sb, rng, f"{prefix}{i}", parent, jt)
    return parent


def _free_root(sb, rng, name):
    return sb.add_body(name, 0, pos=(0.0, 0.0, 0.5), jtype=JNT_FREE, **_inertial(rng, mass=3.0))


def build(name: str):
    """-> (SceneBuilder, MirSceneSpec) of the case `name`"""
    rng = np.random.default_rng(SEED[name])
    sb = SceneBuilder()
    sb.add_geom(0, GEOM_PLANE)
    if name == "oblique_chain":
        _chain(sb, rng, "c", _body(sb, rng, "base", 0, F), (R, P, R, F, R, P, R, R, F, P))
    elif name == "deep":
        _chain(sb, rng, "d", 0, [P if i % 4 == 3 else R for i in range(15)])
    elif name == "bushy":
        def grow(parent, depth, tag):   # depth-first preorder, the body order the 16-lane compiler asks for
            for k in range(2):
                b = _body(sb, rng, f"{tag}{k}", parent, P if (depth + len(sb.bodies) + k) % 3 == 0 else R)
                if depth < 2:
                    grow(b, depth + 1, f"{tag}{k}")

        grow(_body(sb, rng, "root", 0, R), 0, "b")
    elif name == "floating":
        root = _free_root(sb, rng, "torso")
        for l, kinds in enumerate(((R, R, R), (R, P, R), (R, R, R))):
            _chain(sb, rng, f"limb{l}_", root, kinds)
    elif name == "many":
        _chain(sb, rng, "a", 0, (F, R, P, R, F, R, R, P, R))
        root = _free_root(sb, rng, "torso")
        _chain(sb, rng, "limb0_", root, (R, P))
        _chain(sb, rng, "limb1_", root, (R, R, R))
        m = 200.0 * 0.04 ** 3
        sb.add_body("cube", 0, pos=(0.5, 0.0, 0.02), jtype=JNT_FREE, mass=m, inertia=box_inertia(m, (0.02, 0.02, 0.02)))
    else:
        raise KeyError(name)
    spec = sb.build()
    assert (spec.nbody, spec.ndof) == DIMS[name], (name, spec.nbody, spec.ndof)
    return sb, spec


def links_on_long_paths(model, n_min=6):
    """links with at least n_min dofs on their path world -> link, deepest first"""
    nd = {0: 0, 1: 1, 2: 1, 3: 6}
    count = {b: sum(nd[model.jtype[c]] for c in model.path(b)) for b in range(1, model.nbody)}
    return sorted((b for b in count if count[b] >= n_min), key=lambda b: (-count[b], b))
