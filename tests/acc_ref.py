"""Reference for mir_link_accelerations (include/mirigid.h): link accelerations, Jdot qvel and IMU readings restated in NumPy from the
oracle's own forward kinematics.  A helper, no test.

Inputs are the oracle's XPOS / XQUAT after `Oracle.fk`, its QVEL and a qacc, plus the parents, joint types and joint axes of the spec
(kin_ref.Model).  One walk down the path world -> link, root first, carrying the angular velocity w, the angular acceleration and the
acceleration of the current body's origin, the last two split into the part without qacc (b) and the part linear in it (a):

    free root:   w = qvel[3:6], alpha_a = qacc[3:6], o''_a = qacc[0:3]                      (its qvel IS the world velocity of its origin)
    body j below body j-1, d = o_j - o_{j-1} (fixed in j-1 up to a prismatic slide):
        o''_b += alpha_b x d + w x (w x d),   o''_a += alpha_a x d                          (w, alpha: those of j-1)
        revolute, a = R_j axis:  alpha_b += (w x a) qd,  alpha_a += a qdd,  w += a qd       (the axis turns with j-1: da/dt = w x a)
        prismatic:               o''_b += 2 (w x a) qd,  o''_a += a qdd
    the point p = o + r, r = R local_point:  p''_b = o''_b + alpha_b x r + w x (w x r),  p''_a = o''_a + alpha_a x r

    bias_acc = [p''_b; alpha_b]   acc = bias_acc + [p''_a; alpha_a]   imu = [R_s^T (acc_lin - g); R_s^T w],  R_s = R R(quat_offset)

`dtype=np.float64` on the float64 oracle is the reference; `dtype=np.float32` on the poses of `Oracle(f32=...)` is the float32 port the
GPU tests use as their yardstick: the same formulas with every intermediate rounded to float32.
"""
from __future__ import annotations

import numpy as np

import kin_ref
import orc
from kin_ref import FREE, PRISMATIC, REVOLUTE, quat_to_mat


def _unit(q, dtype):
    q = np.asarray(q).astype(dtype)
    return q / np.sqrt((q * q).sum(dtype=dtype))


def link_accelerations(model: kin_ref.Model, xpos, xquat, qvel, qacc, link: int, local_point=(0.0, 0.0, 0.0), quat_offset=(1.0, 0.0, 0.0, 0.0),
                       gravity=(0.0, 0.0, -9.81), dtype=np.float64) -> dict:
    """acc (6,), bias_acc (6,), imu (6,) of `link` from world poses xpos (nbody,3) / xquat (nbody,4), qvel (nv,) and qacc (nv,)."""
    xpos, xquat, qvel, qacc = (np.asarray(a).astype(dtype) for a in (xpos, xquat, qvel, qacc))
    z = np.zeros(3, dtype=dtype)
    w, alb, ala, ob, oa, prev = z, z, z, z, z, z
    for b in model.path(link):
        d, jt = model.dofadr[b], model.jtype[b]
        if jt == FREE:
            w, alb, ala, ob, oa = qvel[d + 3:d + 6], z, qacc[d + 3:d + 6], z, qacc[d:d + 3]
        else:
            dd = xpos[b] - prev
            ob = ob + np.cross(alb, dd) + np.cross(w, np.cross(w, dd))
            oa = oa + np.cross(ala, dd)
            if jt in (REVOLUTE, PRISMATIC):
                a = quat_to_mat(_unit(xquat[b], dtype), dtype) @ model.axis[b].astype(dtype)
                wxa = np.cross(w, a)
                if jt == REVOLUTE:
                    alb, ala, w = alb + qvel[d] * wxa, ala + qacc[d] * a, w + qvel[d] * a
                else:
                    ob, oa = ob + (dtype(2) * qvel[d]) * wxa, oa + qacc[d] * a
        prev = xpos[b]
    R = quat_to_mat(_unit(xquat[link], dtype), dtype)
    r = R @ np.asarray(local_point).astype(dtype)
    lb = ob + np.cross(alb, r) + np.cross(w, np.cross(w, r))
    lin = lb + (oa + np.cross(ala, r))
    Rs = R @ quat_to_mat(_unit(quat_offset, dtype), dtype)
    g = np.asarray(gravity).astype(dtype)
    return {"acc": np.concatenate([lin, alb + ala]), "bias_acc": np.concatenate([lb, alb]), "imu": np.concatenate([Rs.T @ (lin - g), Rs.T @ w])}


def oracle_accelerations(o: orc.Oracle, model: kin_ref.Model, links, qacc, local_points=None, quat_offsets=None, envs=None, dtype=np.float64) -> dict:
    """The batched result in the shapes of MirScene.link_accelerations -- acc, bias_acc, imu (R,L,6) -- from the oracle's state: `Oracle.fk`
    on every env asked for, then the walk.  qacc (R, nv): row k goes with envs[k].  local_points (3,) or (L,3), quat_offsets (4,) or (L,4)."""
    links = [int(b) for b in links]
    envs = range(o.B) if envs is None else [int(e) for e in envs]
    lp = np.zeros((len(links), 3)) if local_points is None else np.broadcast_to(np.asarray(local_points, dtype=np.float64), (len(links), 3))
    qo = np.broadcast_to(np.asarray((1.0, 0.0, 0.0, 0.0) if quat_offsets is None else quat_offsets, dtype=np.float64), (len(links), 4))
    g = tuple(o.spec.opt.gravity)
    qacc = np.asarray(qacc, dtype=np.float64).reshape(len(envs), model.nv)
    out = {"acc": [], "bias_acc": [], "imu": []}
    for k, e in enumerate(envs):
        o.fk(e)
        xp, xq, qv = o.read(orc.F_XPOS, e).reshape(-1, 3), o.read(orc.F_XQUAT, e).reshape(-1, 4), o.read(orc.F_QVEL, e)
        rows = [link_accelerations(model, xp, xq, qv, qacc[k], b, lp[i], qo[i], g, dtype) for i, b in enumerate(links)]
        for n in out:
            out[n].append(np.stack([r[n] for r in rows]))
    return {n: np.stack(v) for n, v in out.items()}


def _qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def integrate(model: kin_ref.Model, q, qvel, h: float) -> np.ndarray:
    """qpos after the time h at the constant qvel, float64: scalar joints q <- q + h qvel; a free body position <- position + h v,
    quaternion <- exp(w h) (x) q (the integrator's rule, world angular velocity)."""
    q, qvel = np.array(q, dtype=np.float64), np.asarray(qvel, dtype=np.float64)
    for b in range(1, model.nbody):
        qa, d, jt = model.qadr[b], model.dofadr[b], model.jtype[b]
        if jt in (REVOLUTE, PRISMATIC):
            q[qa] += h * qvel[d]
        elif jt == FREE:
            q[qa:qa + 3] += h * qvel[d:d + 3]
            th = h * qvel[d + 3:d + 6]
            ang = np.linalg.norm(th)
            dq = np.concatenate([[np.cos(0.5 * ang)], (np.sin(0.5 * ang) / ang if ang > 1e-300 else 0.5) * th])
            q[qa + 3:qa + 7] = _qmul(dq, q[qa + 3:qa + 7])
    return q
