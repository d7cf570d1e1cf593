"""Reference for mir_link_kinematics (include/mirigid.h): link poses, velocities and geometric Jacobians restated in NumPy from the
oracle's own forward kinematics.  A helper, no test.

Inputs are the oracle's XPOS / XQUAT after `Oracle.fk` and its QVEL, plus the parents, joint types and joint axes of the spec; the
function is the table of the header, nothing else:

    p = o_link + R_link local_point
    revolute dof of body b on the path world -> link, a = R_b axis:   [a x (p - o_b); a]
    prismatic:                                                        [a; 0]
    free, linear dof k:                                               [e_k; 0]
    free, angular dof k:                                              [e_k x (p - o_b); e_k]
    dofs of bodies off the path:                                      0
    vel = J qvel

`dtype=np.float64` on the float64 oracle is the reference; `dtype=np.float32` on the poses of `Oracle(f32=...)` is the float32 port
the GPU tests use as their yardstick: the same formulas with every intermediate rounded to float32.
"""
from __future__ import annotations

import numpy as np

import orc

FIXED, REVOLUTE, PRISMATIC, FREE = 0, 1, 2, 3


class Model:
    """parents, joint types, axes and dof addresses of a MirSceneSpec (dofs in body order: 1 per scalar joint, 6 per free joint)"""

    def __init__(self, spec):
        self.nbody = spec.nbody
        self.parent = [spec.body[b].parent for b in range(spec.nbody)]
        self.jtype = [spec.body[b].jtype if b else FIXED for b in range(spec.nbody)]
        self.axis = np.array([list(spec.body[b].axis) for b in range(spec.nbody)], dtype=np.float64)
        self.dofadr, self.qadr, nv, nq = [], [], 0, 0
        for b in range(spec.nbody):
            self.dofadr.append(nv)
            self.qadr.append(nq)
            nv += {FIXED: 0, REVOLUTE: 1, PRISMATIC: 1, FREE: 6}[self.jtype[b]]
            nq += {FIXED: 0, REVOLUTE: 1, PRISMATIC: 1, FREE: 7}[self.jtype[b]]
        self.nv, self.nq = nv, nq

    def path(self, link: int) -> list:
        """bodies on the path world -> link, root first.  A free body's pose is its qpos whatever is above it (orc_fk): the path starts
        there (the spec compilers accept free joints under the world only)."""
        out, b = [], int(link)
        while b > 0:
            out.append(b)
            if self.jtype[b] == FREE:
                break
            b = self.parent[b]
        return out[::-1]

    def limits(self, spec):
        """(lo, hi) per scalar dof from the spec, None where the joint has no range"""
        return [(spec.dof[d].range[0], spec.dof[d].range[1]) if spec.dof[d].limited else None for d in range(self.nv)]


def quat_to_mat(q, dtype=np.float64):
    w, x, y, z = (dtype(v) for v in q)
    one, two = dtype(1), dtype(2)
    return np.array([[one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)],
                     [two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)],
                     [two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)]], dtype=dtype)


def link_kinematics(model: Model, xpos, xquat, qvel, link: int, local_point=(0.0, 0.0, 0.0), dtype=np.float64) -> dict:
    """pos (3,), quat (4,) wxyz normalised, vel (6,), jac (6, nv) of `link` from world poses xpos (nbody,3) / xquat (nbody,4)."""
    xpos, xquat, qvel = (np.asarray(a).astype(dtype) for a in (xpos, xquat, qvel))
    ql = xquat[link] / np.sqrt((xquat[link] * xquat[link]).sum(dtype=dtype))
    p = xpos[link] + quat_to_mat(ql, dtype) @ np.asarray(local_point).astype(dtype)
    J = np.zeros((6, model.nv), dtype=dtype)
    for b in model.path(link):
        d, jt = model.dofadr[b], model.jtype[b]
        r = p - xpos[b]
        if jt in (REVOLUTE, PRISMATIC):
            qb = xquat[b] / np.sqrt((xquat[b] * xquat[b]).sum(dtype=dtype))
            a = quat_to_mat(qb, dtype) @ model.axis[b].astype(dtype)
            if jt == REVOLUTE:
                J[0:3, d], J[3:6, d] = np.cross(a, r), a
            else:
                J[0:3, d] = a
        elif jt == FREE:
            for k in range(3):
                e = np.zeros(3, dtype=dtype)
                e[k] = 1
                J[k, d + k] = 1
                J[0:3, d + 3 + k], J[3 + k, d + 3 + k] = np.cross(e, r), 1
    return {"pos": p, "quat": ql, "vel": J @ qvel, "jac": J}


def oracle_kinematics(o: orc.Oracle, model: Model, links, local_points=None, envs=None, dtype=np.float64) -> dict:
    """The batched result in the shapes of MirScene.link_kinematics -- pos (R,L,3), quat (R,L,4), vel (R,L,6), jac (R,L,6,nv) -- from
    the oracle's state: `Oracle.fk` on every env asked for, then the table.  local_points (3,) or (L,3)."""
    links = [int(b) for b in links]
    envs = range(o.B) if envs is None else [int(e) for e in envs]
    lp = np.zeros((len(links), 3)) if local_points is None else np.broadcast_to(np.asarray(local_points, dtype=np.float64), (len(links), 3))
    out = {"pos": [], "quat": [], "vel": [], "jac": []}
    for e in envs:
        o.fk(e)
        xp, xq, qv = o.read(orc.F_XPOS, e).reshape(-1, 3), o.read(orc.F_XQUAT, e).reshape(-1, 4), o.read(orc.F_QVEL, e)
        rows = [link_kinematics(model, xp, xq, qv, b, lp[i], dtype) for i, b in enumerate(links)]
        for k in out:
            out[k].append(np.stack([r[k] for r in rows]))
    return {k: np.stack(v) for k, v in out.items()}


def random_state(spec, model: Model, n: int, seed: int, cube_box=((-0.3, -0.3, 0.05), (0.7, 0.3, 0.9))):
    """Seeded states for the parity tests: scalar joints uniform inside their ranges (+-1 where a joint has none), free bodies at
    uniform positions in `cube_box` with uniform random unit quaternions, qvel uniform in [-1, 1].  float32 values, so that the GPU and
    the oracles hold the same bits.  -> qpos (n, nq), qvel (n, nv) float32."""
    rng = np.random.default_rng(seed)
    lim = model.limits(spec)
    q = np.zeros((n, model.nq), np.float32)
    for b in range(1, model.nbody):
        qa, jt = model.qadr[b], model.jtype[b]
        if jt in (REVOLUTE, PRISMATIC):
            lo, hi = lim[model.dofadr[b]] or (-1.0, 1.0)
            q[:, qa] = rng.uniform(lo, hi, n)
        elif jt == FREE:
            q[:, qa:qa + 3] = rng.uniform(cube_box[0], cube_box[1], (n, 3))
            u = rng.normal(size=(n, 4))
            q[:, qa + 3:qa + 7] = u / np.linalg.norm(u, axis=1, keepdims=True)
    v = rng.uniform(-1.0, 1.0, (n, model.nv)).astype(np.float32)
    return q, v
