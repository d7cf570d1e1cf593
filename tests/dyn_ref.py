"""Reference for mir_dynamics (include/mirigid.h): mass matrix, bias forces, gravity forces, inverse dynamics and PD control forces
from the in-repo oracle.  A helper, no test.

The oracle is driven, not restated: qpos / qvel are written, the PD targets set, `forward()` called, and M (`F_M`: composite rigid
bodies, armature on the diagonal, no dt (damping + kv)), `F_QFRC_BIAS` (recursive Newton-Euler at qacc = 0 with gravity) and
`F_QFRC_ACT` (the clamped PD torque) read.  `gravity` is a second evaluation at qvel = 0; tau = M @ qacc + bias is NumPy float64 on
what was read.  On `Oracle(f32=...)` the same calls give the float32 port the GPU tests use as their yardstick (tau then sums the
float32 values in float32, the way a float32 implementation does).

tests/test_dyn_cpu.py pins this reference from first principles (potential-energy differences, kinetic energy, tree structure).
"""
from __future__ import annotations

import numpy as np

import orc

OUTS = ("mass", "bias", "gravity", "tau", "ctrl_force")


def oracle_dynamics(o: orc.Oracle, qpos, qvel, targets=None, qacc=None, f32: bool = False) -> dict:
    """mass (B,nv,nv), bias, gravity, ctrl_force (B,nv) and, with qacc (B,nv), tau (B,nv) of the states qpos (B,nq) / qvel (B,nv) with the
    PD targets `targets` (B,nu) (None: as they are in the oracle).  The oracle is left at (qpos, qvel)."""
    qpos, qvel = np.asarray(qpos, dtype=np.float64), np.asarray(qvel, dtype=np.float64)
    nv = o.nv
    o.write_all(orc.F_QPOS, qpos)
    if targets is not None:
        o.set_targets(np.asarray(targets, dtype=np.float64))
    o.write_all(orc.F_QVEL, np.zeros_like(qvel))
    for e in range(o.B):
        o.forward(e)
    out = {"gravity": o.read_all(orc.F_QFRC_BIAS, nv).copy()}
    o.write_all(orc.F_QVEL, qvel)
    for e in range(o.B):
        o.forward(e)
    out["mass"] = o.read_all(orc.F_M, nv * nv).reshape(o.B, nv, nv).copy()
    out["bias"] = o.read_all(orc.F_QFRC_BIAS, nv).copy()
    out["ctrl_force"] = o.read_all(orc.F_QFRC_ACT, nv).copy()
    if qacc is not None:
        if f32:
            M, a, c = out["mass"].astype(np.float32), np.asarray(qacc, dtype=np.float32), out["bias"].astype(np.float32)
            out["tau"] = (np.einsum("bij,bj->bi", M, a, dtype=np.float32) + c).astype(np.float64)
        else:
            out["tau"] = np.einsum("bij,bj->bi", out["mass"], np.asarray(qacc, dtype=np.float64)) + out["bias"]
    return out


def pd_margin(spec, qpos, qvel, targets) -> np.ndarray:
    """For every position-controlled dof of every env: |unclamped PD torque - nearest force limit| / (force range), float64.  A clamp
    that is active in one evaluation and not in another is a legitimate O(range) difference; the tests keep this above 1e-3."""
    qpos, qvel, targets = (np.asarray(a, dtype=np.float64) for a in (qpos, qvel, targets))
    m, u = [], 0
    nd = {0: 0, 1: 1, 2: 1, 3: 6}
    nq_of = {0: 0, 1: 1, 2: 1, 3: 7}
    qadr, dof_q, nq = [], {}, 0
    d = 0
    for b in range(spec.nbody):
        jt = spec.body[b].jtype if b else 0
        if jt in (1, 2):
            dof_q[d] = nq
        d += nd[jt]
        nq += nq_of[jt]
    for i in range(spec.ndof):
        s = spec.dof[i]
        if s.ctrl_mode != 1:
            continue
        f = np.float32(s.kp) * (targets[:, u] - qpos[:, dof_q[i]]) - np.float32(s.kv) * qvel[:, i]
        lo, hi = float(np.float32(s.frc_range[0])), float(np.float32(s.frc_range[1]))
        m.append(np.minimum(np.abs(f - lo), np.abs(f - hi)) / (hi - lo))
        u += 1
    return np.stack(m, 1)


def random_targets_and_acc(spec, qpos, qvel, seed: int):
    """Seeded PD targets (B,nu) around the joint positions and accelerations (B,nv) in [-2, 2], float32.  A target whose unclamped PD
    torque comes within 1e-3 of the force range of a limit is moved away from it (towards the joint position), so that no evaluation
    in float32 sits on the other side of a clamp than the float64 reference."""
    rng = np.random.default_rng(seed)
    B = qpos.shape[0]
    ctrl = [i for i in range(spec.ndof) if spec.dof[i].ctrl_mode == 1]
    d, nq, dof_q = 0, 0, {}
    for b in range(spec.nbody):
        jt = spec.body[b].jtype if b else 0
        if jt in (1, 2):
            dof_q[d] = nq
        d += {0: 0, 1: 1, 2: 1, 3: 6}[jt]
        nq += {0: 0, 1: 1, 2: 1, 3: 7}[jt]
    tgt = np.stack([qpos[:, dof_q[i]] for i in ctrl], 1).astype(np.float64)
    # offsets wide enough that some dofs clamp (range / kp) and some do not
    for k, i in enumerate(ctrl):
        s = spec.dof[i]
        span = (s.frc_range[1] - s.frc_range[0]) / max(s.kp, 1e-9)
        tgt[:, k] += rng.uniform(-1.0, 1.0, B) * span
    tgt = tgt.astype(np.float32)
    for _ in range(8):
        bad = pd_margin(spec, qpos, qvel, tgt) < 2e-3
        if not bad.any():
            break
        base = np.stack([qpos[:, dof_q[i]] for i in ctrl], 1)
        tgt = np.where(bad, (base + 0.9 * (tgt - base)).astype(np.float32), tgt)
    qacc = rng.uniform(-2.0, 2.0, (B, spec.ndof)).astype(np.float32)
    return tgt, qacc
