"""Reference for mir_inverse_kinematics_multilink (include/mirigid.h): the multi-link damped-least-squares iteration restated in NumPy on
the oracle's own forward kinematics (`Oracle.fk`).  A helper, no test.

The iteration is the one of mir_inverse_kinematics (accept / reject / stall, the lambda^2 schedule, max_step, the clamp, max_iters) over
the stacked task rows of up to four links:

    per link l:  ep_l = pos_mask o (p*_l - p_l); the linear Jacobian rows masked alike
                 rot_mask all true:  er_l = rotvec(q*_l q_l^-1), rows J_w
                 one true entry k:   a = R_l e_k, a* = R*_l e_k, er_l = atan2(|a x a*|, a . a*) (a x a*) / |a x a*| (0 below 1e-9),
                                     rows (I - a a^T) J_w
                 none / no target quaternion: no orientation rows
    m = sum_l |ep_l| / pos_tol + |er_l| / rot_tol;  converged: every |ep_l| < pos_tol and |er_l| < rot_tol at the accepted iterate
    limit rule (respect_joint_limit), when an iterate is accepted, g = J^T e:  a limited moving joint with q == lo and g < 0, or
                 q == hi and g > 0, has a zero Jacobian column until the next accepted iterate
    dq = J^T (J J^T + lambda^2 I)^-1 e, by a pivoted solve (np.linalg.solve)
    samples: sample 0 from the seed; sample s >= 1 draws every limited moving joint of column k at lo + (hi - lo) u(seed, env, s, k);
                 the first converged sample wins, else the smallest final m (the lower s on a tie)

`dtype=np.float64` on the float64 oracle is the reference; `dtype=np.float32` on `Oracle(f32=...)` is the float32 port the GPU tests use
as their yardstick: the same formulas with every intermediate rounded to float32.  The joint ranges are the float32 values the compiled
models hold (so that "q == lo" means the same on both sides of a comparison with the kernel).
"""
from __future__ import annotations

import numpy as np

import kin_ref
import orc

FIXED, REVOLUTE, PRISMATIC, FREE = 0, 1, 2, 3
DEFAULTS = dict(max_iters=20, respect_joint_limit=1, damping=0.05, pos_tol=5e-4, rot_tol=5e-3, max_step=0.5)
M32 = 0xFFFFFFFF


def hash_u(seed: int, env: int, s: int, k: int) -> float:
    """u in [0, 1) of sample s >= 1, column k, env `env`: uint32 arithmetic, u = (x >> 8) 2^-24"""
    x = (seed * 0x9E3779B1 + env * 0x85EBCA77 + s * 0xC2B2AE3D + k * 0x27D4EB2F + 0x165667B1) & M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return (x >> 8) * 2.0 ** -24


class Arm:
    """the scalar joints of a spec in body order (= the columns of the (rows, n_arm) arrays), their ranges, the chains of the links"""

    def __init__(self, spec):
        self.model = kin_ref.Model(spec)
        m = self.model
        self.bodies = [b for b in range(1, m.nbody) if m.jtype[b] in (REVOLUTE, PRISMATIC)]
        self.n_arm = len(self.bodies)
        self.qadr = [m.qadr[b] for b in self.bodies]
        lim = m.limits(spec)
        self.limited = np.array([lim[m.dofadr[b]] is not None for b in self.bodies])
        rng = [lim[m.dofadr[b]] or (0.0, 0.0) for b in self.bodies]
        self.lo = np.array([np.float32(r[0]) for r in rng], np.float64)
        self.hi = np.array([np.float32(r[1]) for r in rng], np.float64)

    def chain_cols(self, link: int) -> list:
        """columns of the scalar joints on the chain world -> link"""
        out, b = [], int(link)
        while b > 0:
            if self.model.jtype[b] == FREE:
                raise ValueError("the link hangs off a free body")
            if b in self.bodies:
                out.append(self.bodies.index(b))
            b = self.model.parent[b]
        return out[::-1]


def _qmul(p, q):
    return np.array([p[0] * q[0] - p[1] * q[1] - p[2] * q[2] - p[3] * q[3], p[0] * q[1] + p[1] * q[0] + p[2] * q[3] - p[3] * q[2],
                     p[0] * q[2] - p[1] * q[3] + p[2] * q[0] + p[3] * q[1], p[0] * q[3] + p[1] * q[2] - p[2] * q[1] + p[3] * q[0]], dtype=p.dtype)


def _norm(v, dtype):
    return np.sqrt((v * v).sum(dtype=dtype))


def _fk(o: orc.Oracle, arm: Arm, q, dtype):
    full = o.read(orc.F_QPOS, 0)
    full[arm.qadr] = q
    o.write(orc.F_QPOS, full, 0)
    o.fk(0)
    xp = o.read(orc.F_XPOS, 0).reshape(-1, 3).astype(dtype)
    xq = o.read(orc.F_XQUAT, 0).reshape(-1, 4).astype(dtype)
    return xp, xq / np.sqrt((xq * xq).sum(1, dtype=dtype))[:, None]


def task_error(xp, xq, links, tpos, tquat, pos_mask, rot_mask, dtype):
    """-> e (stacked selected rows), per-link |ep|, |er|, and per link the data the Jacobian rows need"""
    pm = np.array(pos_mask, bool)
    rm = np.array(rot_mask, bool) if tquat is not None else np.zeros(3, bool)
    e, epn, ern, aux = [], [], [], []
    for l, b in enumerate(links):
        ep = np.where(pm, tpos[l].astype(dtype) - xp[b], dtype(0)).astype(dtype)
        er, a = np.zeros(3, dtype), None
        if rm.all():
            tq = tquat[l].astype(dtype)
            tq = tq / _norm(tq, dtype)
            qc = xq[b] * np.array([1, -1, -1, -1], dtype)
            d = _qmul(tq, qc)
            if d[0] < 0:
                d = -d
            sn = _norm(d[1:], dtype)
            kk = dtype(2) * np.arctan2(sn, d[0]).astype(dtype) / sn if sn > 1e-9 else dtype(2)
            er = (kk * d[1:]).astype(dtype)
        elif rm.any():
            k = int(np.argmax(rm))
            tq = tquat[l].astype(dtype)
            tq = tq / _norm(tq, dtype)
            a = kin_ref.quat_to_mat(xq[b], dtype)[:, k]
            at = kin_ref.quat_to_mat(tq, dtype)[:, k]
            c = np.cross(a, at).astype(dtype)
            s = _norm(c, dtype)
            if s >= 1e-9:
                er = (np.arctan2(s, (a * at).sum(dtype=dtype)).astype(dtype) / s * c).astype(dtype)
        e.append(ep[pm])
        if rm.any():
            e.append(er)
        epn.append(_norm(ep, dtype))
        ern.append(_norm(er, dtype))
        aux.append(a)
    return np.concatenate(e).astype(dtype), np.array(epn, dtype), np.array(ern, dtype), aux


def task_jacobian(arm: Arm, xp, xq, links, aux, moving, pos_mask, rot_mask, userot, dtype):
    """the stacked selected rows x n_arm; columns of joints that do not move are zero"""
    m = arm.model
    pm = np.array(pos_mask, bool)
    rm = np.array(rot_mask, bool) if userot else np.zeros(3, bool)
    blocks = []
    for l, b in enumerate(links):
        Jv, Jw = np.zeros((3, arm.n_arm), dtype), np.zeros((3, arm.n_arm), dtype)
        for k in arm.chain_cols(b):
            if not moving[k]:
                continue
            jb = arm.bodies[k]
            ax = kin_ref.quat_to_mat(xq[jb], dtype) @ m.axis[jb].astype(dtype)
            if m.jtype[jb] == REVOLUTE:
                Jv[:, k], Jw[:, k] = np.cross(ax, xp[b] - xp[jb]), ax
            else:
                Jv[:, k] = ax
        blocks.append(Jv[pm])
        if rm.all():
            blocks.append(Jw)
        elif rm.any():
            a = aux[l]
            blocks.append((Jw - np.outer(a, a @ Jw)).astype(dtype))
    return np.concatenate(blocks).astype(dtype)


def solve_row(o, arm: Arm, links, tpos, tquat, seed_q, env=0, pos_mask=(True,) * 3, rot_mask=(True,) * 3, dof_mask=None, max_samples=1,
              seed=0, dtype=np.float64, **opts):
    """one row.  tpos (L,3), tquat (L,4) or None, seed_q (n_arm).  -> q (n_arm, float64 holding dtype values), err (L,2), iters, sample,
    converged"""
    op = {**DEFAULTS, **opts}
    links = [int(b) for b in links]
    nrot = int(np.sum(np.array(rot_mask, bool)))
    if nrot == 2:
        raise ValueError("You can only align 0, 1 axis or all 3 axes.")
    userot = tquat is not None
    onchain = np.zeros(arm.n_arm, bool)
    for b in links:
        onchain[arm.chain_cols(b)] = True
    moving = onchain & (np.ones(arm.n_arm, bool) if dof_mask is None else np.asarray(dof_mask, bool))
    lo, hi = arm.lo.astype(dtype), arm.hi.astype(dtype)
    lim = moving & arm.limited & bool(op["respect_joint_limit"])
    pos_tol, rot_tol, max_step = dtype(op["pos_tol"]), dtype(op["rot_tol"]), dtype(op["max_step"])
    d2 = dtype(op["damping"] * op["damping"])
    lam2_min, lam2_max = d2 * dtype(1.0 / 256.0), d2 * dtype(64.0)
    seed_q = np.asarray(seed_q).astype(dtype)
    best, total_iters = None, 0
    for s in range(int(max_samples)):
        q = seed_q.copy()
        if s > 0:
            for k in np.nonzero(moving & arm.limited)[0]:
                q[k] = lo[k] + (hi[k] - lo[k]) * dtype(hash_u(int(seed), int(env), s, int(k)))
        q_acc, lam2, stall, iters = q.copy(), d2, 0, 0
        m_acc = epn = ern = e_acc = J = None
        for it in range(op["max_iters"] + 1):
            xp, xq = _fk(o, arm, q, dtype)
            e, epn_c, ern_c, aux = task_error(xp, xq, links, tpos, tquat, pos_mask, rot_mask, dtype)
            metric = (epn_c / pos_tol + ern_c / rot_tol).sum(dtype=dtype)
            if it == 0 or metric < m_acc:
                if it > 0:
                    stall = stall + 1 if metric > dtype(0.99) * m_acc else 0
                    lam2 = max(lam2 * dtype(0.25), lam2_min)
                m_acc, epn, ern, e_acc, q_acc = metric, epn_c, ern_c, e, q.copy()
                J = task_jacobian(arm, xp, xq, links, aux, moving, pos_mask, rot_mask, userot, dtype)
                g = J.T @ e_acc
                blocked = lim & (((q_acc == lo) & (g < 0)) | ((q_acc == hi) & (g > 0)))
                J[:, blocked] = 0
            else:
                stall += 1
                lam2 = min(lam2 * dtype(8.0), lam2_max)
            conv = bool((epn < pos_tol).all() and (ern < rot_tol).all())
            if conv or it == op["max_iters"] or stall >= 3:
                break
            iters = it + 1
            A = (J @ J.T + lam2 * np.eye(J.shape[0], dtype=dtype)).astype(dtype)
            dq = (J.T @ np.linalg.solve(A, e_acc)).astype(dtype)
            big = np.abs(dq).max()
            sc = max_step / big if big > max_step else dtype(1)
            q = q_acc.copy()
            q[moving] = (q_acc + sc * dq)[moving]
            q[lim] = np.minimum(np.maximum(q[lim], lo[lim]), hi[lim])
        total_iters += iters
        if conv or best is None or m_acc < best["m"]:
            best = dict(q=q_acc.astype(np.float64), err=np.stack([epn, ern], 1).astype(np.float64), m=m_acc, sample=s, converged=conv)
        if conv:
            break
    best["iters"] = total_iters
    return best


def solve(o, spec_or_arm, links, poss, quats, seed_q, envs=None, **kw):
    """rows.  poss (R,L,3), quats (R,L,4) or None, seed_q (R,n_arm), envs (R) env index per row (None: the row).
    -> dict q (R,n_arm), err (R,L,2), iters (R), sample (R), converged (R)"""
    arm = spec_or_arm if isinstance(spec_or_arm, Arm) else Arm(spec_or_arm)
    poss = np.asarray(poss, np.float64)
    R = poss.shape[0]
    envs = np.arange(R) if envs is None else np.asarray(envs)
    rows = [solve_row(o, arm, links, poss[r], None if quats is None else np.asarray(quats, np.float64)[r], np.asarray(seed_q)[r], env=int(envs[r]), **kw)
            for r in range(R)]
    return {"q": np.stack([r["q"] for r in rows]), "err": np.stack([r["err"] for r in rows]), "iters": np.array([r["iters"] for r in rows]),
            "sample": np.array([r["sample"] for r in rows]), "converged": np.array([r["converged"] for r in rows])}


def link_poses(o, arm: Arm, links, q, dtype=np.float64):
    """(L,3), (L,4): the links' world poses at the joint row q"""
    xp, xq = _fk(o, arm, np.asarray(q).astype(dtype), dtype)
    return xp[list(links)], xq[list(links)]


def masked_errors(o, arm: Arm, links, tpos, tquat, q, pos_mask=(True,) * 3, rot_mask=(True,) * 3, dtype=np.float64):
    """(L,2): |ep_l|, |er_l| of the header's definitions at the joint row q"""
    xp, xq = _fk(o, arm, np.asarray(q).astype(dtype), dtype)
    _, epn, ern, _ = task_error(xp, xq, [int(b) for b in links], np.asarray(tpos), None if tquat is None else np.asarray(tquat), pos_mask, rot_mask, dtype)
    return np.stack([epn, ern], 1)


# ---- the cases of the GPU tier (tests/test_gpu_ikm.py), whose convergence in this reference and in the float32 port the CPU tier
# asserts (tests/test_ikm_cpu.py): that is what lets the GPU test demand convergence on every row
GPU_CASES = (
    dict(name="hand+link4 position", links=("hand", "link4"), quats=False),
    dict(name="hand+link4 pose", links=("hand", "link4")),
    dict(name="hand z axis", links=("hand",), rot_mask=(False, False, True)),
    dict(name="hand x axis, xy position", links=("hand",), rot_mask=(True, False, False), pos_mask=(True, True, False)),
    dict(name="fingers pose, arm dofs", links=("left_finger", "right_finger"), dofs=(0, 1, 2, 3, 4, 5, 6)),
    dict(name="fingers pose, all dofs", links=("left_finger", "right_finger"), fingers="uniform"),
    dict(name="hand position, dofs 0-3", links=("hand",), quats=False, dofs=(0, 1, 2, 3)),
)


def arm_configs(home, n, rng, fingers=None, finger_hi=0.04):
    """home +- 0.5 rad on the seven arm joints, joint 4 clipped to [-2.9, -0.3] (tests/test_ik_cpu.py); fingers at home, or uniform in
    [0, finger_hi] (0.04, or the scene's finger range where that is narrower: the stack scene's fingers open to 0.024)"""
    qt = np.tile(np.asarray(home, np.float64), (n, 1))
    qt[:, :7] += rng.uniform(-0.5, 0.5, (n, 7))
    qt[:, 3] = np.clip(qt[:, 3], -2.9, -0.3)
    if fingers == "uniform":
        qt[:, 7:9] = rng.uniform(0.0, 1.0, (n, 2)) * finger_hi
    return qt


def build_case(builder, spec, o64, arm: Arm, case: dict, home, n: int, seed: int) -> dict:
    """targets = the float64 poses of the case's links at seeded configurations, rounded to float32 (what every solver is given); the
    seed of the solve is the home pose"""
    rng = np.random.default_rng(seed)
    links = [builder.body_index(nm) for nm in case["links"]]
    qt = arm_configs(home, n, rng, case.get("fingers"), min(0.04, float(arm.hi[7])))
    full = np.concatenate([qt, np.zeros((n, arm.n_arm - qt.shape[1]))], 1) if arm.n_arm > qt.shape[1] else qt
    poses = [link_poses(o64, arm, links, full[r]) for r in range(n)]
    poss = np.stack([p for p, _ in poses]).astype(np.float32)
    quats = np.stack([q for _, q in poses]).astype(np.float32) if case.get("quats", True) else None
    seed_q = np.zeros((n, arm.n_arm), np.float32)
    seed_q[:, :len(home)] = np.asarray(home, np.float32)
    dof_mask = None
    if case.get("dofs") is not None:
        dof_mask = np.zeros(arm.n_arm, bool)
        dof_mask[list(case["dofs"])] = True
    onchain = np.zeros(arm.n_arm, bool)
    for b in links:
        onchain[arm.chain_cols(b)] = True
    return dict(name=case["name"], links=links, poss=poss, quats=quats, seed_q=seed_q, dof_mask=dof_mask, dofs=case.get("dofs"),
                pos_mask=tuple(case.get("pos_mask", (True,) * 3)), rot_mask=tuple(case.get("rot_mask", (True,) * 3)),
                moving=onchain if dof_mask is None else onchain & dof_mask)


def kwargs(case: dict) -> dict:
    return dict(pos_mask=case["pos_mask"], rot_mask=case["rot_mask"], dof_mask=case["dof_mask"])


def restart_case(builder, spec, o64, arm: Arm, home, n: int = 32, seed: int = 7) -> dict:
    """hand poses at configurations uniform over the whole ranges of the seven arm joints (fingers at home); the seed is the home pose"""
    rng = np.random.default_rng(seed)
    hand = builder.body_index("hand")
    full = np.zeros((n, arm.n_arm))
    full[:, :len(home)] = np.asarray(home, np.float64)
    full[:, :7] = rng.uniform(arm.lo[:7], arm.hi[:7], (n, 7))
    poses = [link_poses(o64, arm, [hand], full[r]) for r in range(n)]
    seed_q = np.zeros((n, arm.n_arm), np.float32)
    seed_q[:, :len(home)] = np.asarray(home, np.float32)
    return dict(links=[hand], poss=np.stack([p for p, _ in poses]).astype(np.float32), quats=np.stack([q for _, q in poses]).astype(np.float32),
                seed_q=seed_q)
