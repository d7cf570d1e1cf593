"""Reference for mir_task_dynamics (include/mirigid.h): M^-1, M^-1 x, the task-space mobility J M^-1 J^T, the operational-space
inertia (J M^-1 J^T + damping^2 I)^-1 and J-bar = M^-1 J^T lambda.  A helper, no test.

The float64 reference: the oracle's M (dyn_ref.oracle_dynamics) and J (kin_ref.oracle_kinematics) combined in NumPy float64; the 6 x 6
matrix goes through a Cholesky without pivoting written out here, so that the NaN rule of the header (a pivot <= 1e-5 x the largest
diagonal entry: lambda and jbar are NaN) is applied to the same pivots the product looks at, and `relpivot` reports them.

The float32 port (`f32=True`, or "big" for the wave-kernel scenes: the argument of orc.Oracle): the same formulas on the M of
`Oracle(f32=...)` and a float32 J, with a serial float32 Cholesky M = L L^T, forward and backward substitutions, y = L^-1 J^T,
lambda_inv = y^T y, the 6 x 6 Cholesky and its substitutions, all written out with float32 scalars per env (every product and every
partial sum rounded to float32, in index order): no np.linalg.  It is the yardstick of the GPU tests: what a float32 implementation
that walks serially gets.

tests/test_task_cpu.py pins the float64 reference from first principles.
"""
from __future__ import annotations

import numpy as np

import dyn_ref
import kin_ref
import orc

OUTS = ("minv", "solve", "lambda_inv", "lambda", "jbar")
PIVOT = 1e-5


def _chol(A):
    """Serial Cholesky without pivoting of the batch A (B, n, n), in A's dtype -> L (lower), pivots (B, n): the remainders
    a_jj - sum_k l_jk^2 of which the square root is taken"""
    B, n, _ = A.shape
    L = np.zeros_like(A)
    piv = np.zeros((B, n), A.dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(n):
            s = A[:, j, j].copy()
            for k in range(j):
                s = s - L[:, j, k] * L[:, j, k]
            piv[:, j] = s
            L[:, j, j] = np.sqrt(s)
            for i in range(j + 1, n):
                u = A[:, i, j].copy()
                for k in range(j):
                    u = u - L[:, i, k] * L[:, j, k]
                L[:, i, j] = u / L[:, j, j]
    return L, piv


def _forward(L, Bm):
    """L y = Bm for the batch, rows in order, every sum serial in index order"""
    n = L.shape[1]
    Y = np.zeros_like(Bm)
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(n):
            s = Bm[:, i, :].copy()
            for k in range(i):
                s = s - L[:, i, k, None] * Y[:, k, :]
            Y[:, i, :] = s / L[:, i, i, None]
    return Y


def _backward(L, Y):
    """L^T z = Y"""
    n = L.shape[1]
    Z = np.zeros_like(Y)
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(n - 1, -1, -1):
            s = Y[:, i, :].copy()
            for k in range(i + 1, n):
                s = s - L[:, k, i, None] * Z[:, k, :]
            Z[:, i, :] = s / L[:, i, i, None]
    return Z


def _matmul_serial(A, Bm):
    """A @ Bm with the sum over the inner index serial, in the arrays' dtype"""
    out = np.zeros((A.shape[0], A.shape[1], Bm.shape[2]), A.dtype)
    for k in range(A.shape[2]):
        out = out + A[:, :, k, None] * Bm[:, None, k, :]
    return out


def relative_pivots(A):
    """(B,): the smallest pivot of the Cholesky of A (B,6,6) up to and including the first one at or below the rule, over the largest
    diagonal entry of A"""
    _, piv = _chol(A)
    dmax = np.einsum("bii->bi", A).max(1)
    rel = piv / dmax[:, None]
    out = np.empty(A.shape[0], A.dtype)
    for b in range(A.shape[0]):
        bad = np.nonzero(~(rel[b] > PIVOT))[0]
        out[b] = rel[b, :bad[0] + 1].min() if bad.size else rel[b].min()
    return out


def combine(M, J, x=None, damping=0.0):
    """The outputs from M (B,nv,nv) and J (B,L,6,nv), in their dtype (float64: the reference; float32: the port) -> dict over all nv
    dofs, plus relpivot (B,L)."""
    dt = M.dtype
    B, nv, _ = M.shape
    Lk = J.shape[1]
    d2 = dt.type(damping) * dt.type(damping)
    out = {}
    if dt == np.float64:
        minv = np.linalg.inv(M)
        minv = 0.5 * (minv + minv.transpose(0, 2, 1))
        out["minv"] = minv
        if x is not None:
            out["solve"] = np.einsum("bij,bj->bi", minv, np.asarray(x, dt))
        mjt = [minv @ J[:, l].transpose(0, 2, 1) for l in range(Lk)]
        lam_inv = [J[:, l] @ mjt[l] for l in range(Lk)]
        lam_inv = [0.5 * (a + a.transpose(0, 2, 1)) for a in lam_inv]
    else:
        Lm, _ = _chol(M)
        eye = np.broadcast_to(np.eye(nv, dtype=dt), (B, nv, nv)).copy()
        out["minv"] = _backward(Lm, _forward(Lm, eye))
        if x is not None:
            out["solve"] = _backward(Lm, _forward(Lm, np.asarray(x, dt)[:, :, None]))[:, :, 0]
        ys = [_forward(Lm, np.ascontiguousarray(J[:, l].transpose(0, 2, 1))) for l in range(Lk)]
        mjt = [_backward(Lm, y) for y in ys]
        lam_inv = [_matmul_serial(np.ascontiguousarray(y.transpose(0, 2, 1)), y) for y in ys]
    lam, jbar, rel = [], [], []
    eye6 = np.broadcast_to(np.eye(6, dtype=dt), (B, 6, 6)).copy()
    for l in range(Lk):
        A = lam_inv[l] + d2 * eye6
        rel.append(relative_pivots(A))
        if dt == np.float64:
            with np.errstate(all="ignore"):
                C, _ = _chol(A)
                la = _backward(C, _forward(C, eye6))
            jb = mjt[l] @ la
        else:
            C, _ = _chol(A)
            la = _backward(C, _forward(C, eye6))
            jb = _matmul_serial(mjt[l], la)
        sing = ~(rel[-1] > PIVOT)
        la[sing], jb[sing] = np.nan, np.nan
        lam.append(la)
        jbar.append(jb)
    out["lambda_inv"] = np.stack(lam_inv, 1) if Lk else np.zeros((B, 0, 6, 6), dt)
    out["lambda"] = np.stack(lam, 1) if Lk else np.zeros((B, 0, 6, 6), dt)
    out["jbar"] = np.stack(jbar, 1) if Lk else np.zeros((B, 0, nv, 6), dt)
    out["relpivot"] = np.stack(rel, 1) if Lk else np.zeros((B, 0), dt)
    return out


def oracle_mass_and_jacobian(spec, model, qpos, links, local_points=None, f32=False):
    """M (B,nv,nv) and J (B,L,6,nv) at the states qpos (B,nq) from a fresh oracle (`f32`: the argument of orc.Oracle); float64 arrays
    from the float64 oracle, float32 arrays from its float32 build"""
    qpos = np.asarray(qpos)
    B = qpos.shape[0]
    o = orc.Oracle(spec, B, f32=f32) if f32 else orc.Oracle(spec, B)
    dt = np.float32 if f32 else np.float64
    M = dyn_ref.oracle_dynamics(o, qpos, np.zeros((B, model.nv)))["mass"].astype(dt)
    links = [int(b) for b in links]
    if links:
        J = kin_ref.oracle_kinematics(o, model, links, local_points, dtype=dt)["jac"].astype(dt)
    else:
        J = np.zeros((B, 0, 6, model.nv), dt)
    return M, J


def oracle_task_dynamics(spec, model, qpos, links=(), local_points=None, x=None, damping=0.0, f32=False) -> dict:
    """minv (B,nv,nv), solve (B,nv) (with x (B,nv)), lambda_inv, lambda (B,L,6,6), jbar (B,L,nv,6), relpivot (B,L), as float64 arrays:
    the float64 reference, or with `f32` the float32 port."""
    M, J = oracle_mass_and_jacobian(spec, model, qpos, links, local_points, f32)
    out = combine(M, J, x, damping)
    return {k: np.asarray(v, dtype=np.float64) for k, v in out.items()}
