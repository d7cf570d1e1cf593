"""The paths, limits and extra rows of the time-parameterisation tests, shared by tests/test_retime_cpu.py (which holds the conditions
the GPU tests lean on) and tests/test_gpu_retime.py.  A helper, no test.  R = 5 rows per case, fixed seeds.

Paths: D-dof polylines through four random nodes in [-1.5, 1.5]^D, resampled to K waypoints at equal arc length (what mir_plan_path
returns).  dt = 0.01 s, max_path_speed = None (1 / dt).  T = the reference's largest n_samples + 3, one more if that is a multiple of 64.

    name        D   E   K    bound by
    "acc"       9   0   100  acceleration: vmax 2, amax 3
    "vel"       9   0   65   velocity: dofs 2 and 5 at vmax 0.2
    "one"       1   0   16   one dof that turns round twice (a lane mapping of two rows)
    "extra"     9   9   100  synthetic random extra rows with lo < 0 < hi: limits on random combinations of the dofs' accelerations
    "full"      16  16  65   the same with all 64 lanes holding a row
    "three"     9   0   3    the shortest path that can be timed

The known answers: one dof, waypoints 0.01 apart, v = 1, a = 2.5: K = 101 is a trapezoid whose switch points fall on waypoints
(duration 1 / v + v / a = 1.4 s), K = 11 a triangle (2 sqrt(0.1 / 2.5) = 0.4 s).  No float32 holds k / 100: the float64 reference takes
the float64 waypoints, the float32 port and the GPU their float32 roundings, and that difference is part of the port's error.

The torque case: the Franka of the pick scene along a three-node polyline of K = 16 waypoints; rows from tests/dyn_ref.py in float64.
"""
from __future__ import annotations

import functools

import numpy as np

import retime_ref as rr

R, DT = 5, 0.01
CASES = {"acc": (9, 0, 100), "vel": (9, 0, 65), "one": (1, 0, 16), "extra": (9, 9, 100), "full": (16, 16, 65), "three": (9, 0, 3)}
KNOWN = {101: 1.4, 11: 0.4}


def polyline(rng, K, D, nodes=4, span=1.5):
    """K waypoints at equal arc length on the polyline through `nodes` random nodes, float32"""
    P = rng.uniform(-span, span, (nodes, D))
    seg = np.linalg.norm(np.diff(P, axis=0), axis=1)
    cum = np.concatenate([[0.0], np.cumsum(seg)])
    out = np.empty((K, D))
    for w in range(K):
        s = cum[-1] * w / (K - 1)
        k = min(int(np.searchsorted(cum, s, side="right")) - 1, nodes - 2)
        out[w] = P[k] + (s - cum[k]) / seg[k] * (P[k + 1] - P[k])
    out[0], out[-1] = P[0], P[-1]
    return out.astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(paths (R, K, D) float32, vmax (D,), amax (D,), dt, extra: None or four (R, K, E) float32)"""
    D, E, K = CASES[name]
    rng = np.random.default_rng(1000 + sorted(CASES).index(name))
    paths = np.stack([polyline(rng, K, D) for _ in range(R)])
    vmax, amax = np.full(D, 2.0, np.float32), np.full(D, 3.0, np.float32)
    if name == "vel":
        vmax[[2, 5]] = 0.2
    extra = None
    if E:   # extra row e of a row: a random combination w of the dofs' accelerations, |sum_j w_j (m_ij u + c_ij x)| <= limit_e
        w = rng.uniform(-1.0, 1.0, (R, E, D))
        lim = rng.uniform(1.5, 4.0, (R, 1, E))
        mc = [rr.compact_differences(p) for p in paths]
        ea = np.stack([mc[r][0] @ w[r].T for r in range(R)])
        eb = np.stack([mc[r][1] @ w[r].T for r in range(R)])
        extra = tuple(e.astype(np.float32) for e in (ea, eb, np.broadcast_to(-lim, ea.shape), np.broadcast_to(lim * rng.uniform(0.5, 1.0, (R, 1, E)), ea.shape)))
    return dict(paths=paths, vmax=vmax, amax=amax, dt=DT, extra=extra)


@functools.lru_cache(maxsize=None)
def capacity(name):
    """T of a case: no row is truncated, and T is no multiple of 64"""
    T = int(reference(name, "float64", samples=False)["n_samples"].max()) + 3
    return T + 1 if T % 64 == 0 else T


@functools.lru_cache(maxsize=None)
def reference(name, dtname="float64", samples=True):
    """retime_ref.retime of a case in float64 or as the float32 port (computed once, shared; leave it unchanged)"""
    c = case(name)
    return rr.retime(c["paths"], c["vmax"], c["amax"], c["dt"], capacity(name) if samples else 0, None, c["extra"], np.dtype(dtname).type, samples)


def known_path(K, dtype=np.float64):
    """(K, 1): waypoints 0.01 apart"""
    return (np.arange(K, dtype=np.float64) * 0.01).astype(dtype)[:, None]


@functools.lru_cache(maxsize=None)
def known(K, dtname="float64"):
    """the known-answer row: the float64 reference on the float64 waypoints, the port on their float32 roundings"""
    F = np.dtype(dtname).type
    return rr.retime_row(known_path(K, F), [1.0], [2.5], DT, 160, None, None, F)


def yardstick(name, keys=("x", "t", "duration")):
    """tol per output = 4 x max(float32 port against float64 on the same inputs, 2^-23 x scale), scale = the largest value of that
    output in the float64 reference (max x; the duration for t and duration) -> dict, and the printed line"""
    ref, port = reference(name, "float64"), reference(name, "float32")
    tol, parts = {}, []
    for k in keys:
        scale = float(np.abs(ref["duration" if k == "t" else k]).max())
        err = float(np.abs(port[k].astype(np.float64) - ref[k]).max())
        tol[k] = 4.0 * max(err, 2.0 ** -23 * scale)
        parts.append(f"{k}: port {err:.3e} scale {scale:.3e} tol {tol[k]:.3e}")
    return tol, f"[retime, {name}] " + "; ".join(parts)


# ---- the torque case
TORQUE_NODES = ((-0.9, -0.4, 0.0, -2.2, 0.0, 2.0, 0.8, 0.04, 0.04), (0.0, 0.3, 0.2, -1.6, 0.3, 1.7, 0.2, 0.04, 0.04),
                (0.9, -0.35, 0.05, -2.1, 0.0, 1.9, 0.7, 0.04, 0.04))
TORQUE_K, TORQUE_VMAX, TORQUE_AMAX, TORQUE_MULTIPLE = 16, 3.0, 12.0, 1.25


def torque_path():
    """(K, 9) float32: the Franka through TORQUE_NODES at equal steps per segment (K odd segments apart: the middle node is a waypoint)"""
    n = np.asarray(TORQUE_NODES, np.float64)
    half = (TORQUE_K - 1) // 2
    a = [n[0] + (n[1] - n[0]) * k / half for k in range(half)]
    b = [n[1] + (n[2] - n[1]) * k / (TORQUE_K - 1 - half) for k in range(TORQUE_K - half)]
    return np.asarray(a + b).astype(np.float32)


@functools.lru_cache(maxsize=None)
def torque_rows():
    """-> (path (K, 9), extra: four (K, 9) arrays, tmax): the rows of EntityView.retime_path(torque_limits=tmax), computed in float64 (and
    rounded to the float32 the entry point takes) from
    the oracle (tests/dyn_ref.py): alpha = ID(q, 0, m) - g, beta = ID(q, m, c) - g, (lo, hi) = (-tmax - g, tmax - g), g = ID(q, 0, 0);
    tmax = TORQUE_MULTIPLE x the largest gravity torque along the path, on every dof"""
    import orc
    from dyn_ref import oracle_dynamics
    from gym_genesis.backend import models

    P = torque_path()
    K = P.shape[0]
    sb = models.franka_cube_pick_scene()
    spec = sb.build()
    o = orc.Oracle(spec, K)
    cols = [sb.dof_index(j) for j in models.FRANKA_JOINTS]
    q = np.zeros((K, o.nq))
    q[:, 9:] = (0.65, 0.0, 0.02, 1.0, 0.0, 0.0, 0.0)
    q[:, cols] = P
    m, c = rr.compact_differences(P)

    def ID(v, a):
        full_v, full_a = np.zeros((K, o.nv)), np.zeros((K, o.nv))
        full_v[:, cols], full_a[:, cols] = v, a
        return oracle_dynamics(o, q, full_v, qacc=full_a)["tau"][:, cols]

    zero = np.zeros_like(m)
    g = ID(zero, zero)
    tmax = TORQUE_MULTIPLE * float(np.abs(g).max())
    return P, tuple(e.astype(np.float32) for e in (ID(zero, m) - g, ID(m, c) - g, -tmax - g, tmax - g)), tmax
