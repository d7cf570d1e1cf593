"""Reference of mir_retime_path (include/mirigid.h, "time parameterisation"): time-optimal path parameterisation by reachability
analysis on the caller's waypoints, one row at a time, in NumPy.  `retime_row(..., dtype=np.float64)` is the reference; the same code
with dtype=np.float32 is the float32 port whose distance from the reference is the yardstick of the GPU tier (every operation is
written in the order the kernel takes it, one rounding per operation, no fused multiply-add).  The small LPs are solved by bisection
on x with a fixed trip count, as the kernel does: 32 halvings in float32, 64 in float64.

Also here: the geometry of step 2 and the rows of steps 3 - 5 on their own (what the tests judge an (x, u) by), steps 8 and 9 applied
to a given x (what the GPU's t and samples are compared with), and the compacted central differences the torque rows are built from.
"""
import numpy as np

OK, NO_MOTION, TOO_FEW_WAYPOINTS, NOT_FINITE, INFEASIBLE, TRUNCATED = range(6)
STATUS = ("OK", "NO_MOTION", "TOO_FEW_WAYPOINTS", "NOT_FINITE", "INFEASIBLE", "TRUNCATED")
MAX_WAYPOINTS = 2048


def compact(P):
    """step 1 -> the caller's indices of the kept waypoints: waypoint k is dropped when all its values compare equal to the last kept"""
    kept = [0]
    for k in range(1, P.shape[0]):
        if np.any(P[k] != P[kept[-1]]):
            kept.append(k)
    return np.asarray(kept, np.int64)


def geometry(Q):
    """step 2 on the kept waypoints Q (M >= 2, D), in Q's dtype -> d (M-1, D), m (M, D), c (M, D)"""
    F = Q.dtype.type
    d = Q[1:] - Q[:-1]
    m, c = np.zeros_like(Q), np.zeros_like(Q)
    m[0], m[-1] = d[0], d[-1]
    c[1:-1] = d[1:] - d[:-1]
    m[1:-1] = (d[1:] + d[:-1]) * F(0.5)
    return d, m, c


def speed_cap(d, vmax, max_path_speed):
    """step 3 -> cap (M,), in d's dtype: min(max_path_speed^2, (vmax_j / |d_ej|)^2) over the adjacent intervals and the moving dofs"""
    F = d.dtype.type
    vs2 = F(max_path_speed) * F(max_path_speed)
    with np.errstate(divide="ignore"):
        r = np.where(d != 0, vmax.astype(d.dtype)[None, :] / np.abs(d), F(np.inf))
    per = np.minimum(vs2, (r * r).min(1))          # per interval
    cap = np.empty(d.shape[0] + 1, d.dtype)
    cap[0], cap[-1] = per[0], per[-1]
    cap[1:-1] = np.minimum(per[:-1], per[1:])
    return cap


def grid_rows(m, c, amax, extra, i):
    """step 4: the rows (alpha, beta, lo, hi) of gridpoint i, D acceleration rows then E extra rows; extra = None or the four (M, E)
    arrays at the kept waypoints"""
    a, b, lo, hi = m[i], c[i], -amax.astype(m.dtype), amax.astype(m.dtype)
    if extra is not None:
        a, b, lo, hi = (np.concatenate([v, e[i].astype(m.dtype)]) for v, e in zip((a, b, lo, hi), extra))
    return a, b, lo, hi


def interval_rows(m, c, amax, extra, i):
    """step 5: the rows of interval i in (u, x): gridpoint i, then gridpoint i + 1 at (x + 2 u, u)"""
    F = m.dtype.type
    a0, b0, lo0, hi0 = grid_rows(m, c, amax, extra, i)
    a1, b1, lo1, hi1 = grid_rows(m, c, amax, extra, i + 1)
    return np.concatenate([a0, a1 + F(2) * b1]), np.concatenate([b0, b1]), np.concatenate([lo0, lo1]), np.concatenate([hi0, hi1])


def _normalise(a, b, lo, hi):
    """a row as bounds on u that are linear in x: p - r x <= u <= q - r x (a != 0), or as a bound on x alone (a == 0)"""
    F = a.dtype.type
    pos, nz = a > 0, a != 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        p = np.where(nz, np.where(pos, lo, hi) / a, F(-np.inf))
        q = np.where(nz, np.where(pos, hi, lo) / a, F(np.inf))
        r = np.where(nz, b / a, F(0))
    return p, q, r, nz


def _feasible(rows, norm, x, kn):
    """is there a u at x under step 5?  (np.fmax / np.fmin pass over a NaN as the kernel's v_max / v_min do)"""
    F = x.dtype.type
    a, b, lo, hi = rows
    p, q, r, nz = norm
    with np.errstate(invalid="ignore", over="ignore"):
        rx = r * x
        low = np.fmax(np.fmax.reduce(p - rx), F(-0.5) * x)
        up = np.fmin(np.fmin.reduce(q - rx), F(0.5) * (kn - x))
        bx = b * x
    xonly = np.any(~nz & ~((lo <= bx) & (bx <= hi)))
    return bool(low <= up) and not xonly


def retime_row(P, vmax, amax, dt, T=0, max_path_speed=None, extra=None, dtype=np.float64, want_samples=True):
    """One row.  P (K, D): float32, the caller's bits (a float64 P is taken as it is by the float64 reference -- the known answers, whose
    waypoints 0.01 apart no float32 holds -- and rounded to float32 by the port); extra = None or (ea, eb, elo, ehi), each (K, E) ->
    dict with status, x (K,), t (K,), duration, n_samples, and -- with want_samples -- samples (T, D) and sample_vel (T, D).
    Everything in `dtype`."""
    F = np.dtype(dtype).type
    nb = 32 if F is np.float32 else 64
    P = np.asarray(P)
    P = P.astype(np.float32) if F is np.float32 or P.dtype != np.float64 else P
    K, D = P.shape
    vmax, amax = np.asarray(vmax, np.float32).astype(F), np.asarray(amax, np.float32).astype(F)
    dt = F(np.float32(dt))
    vs = F(np.float32(1.0) / np.float32(dt)) if max_path_speed is None else F(np.float32(max_path_speed))
    out = {"status": OK, "x": np.zeros(K, F), "t": np.zeros(K, F), "duration": F(0), "n_samples": 1}

    def fail(status):
        out["status"] = status
        if want_samples:
            out["samples"], out["sample_vel"] = np.tile(P[0].astype(F), (T, 1)), np.zeros((T, D), F)
        return out

    if not np.all(np.isfinite(P)):
        return fail(NOT_FINITE)
    kept = compact(P)
    M = len(kept)
    ex = None
    if extra is not None and extra[0].shape[1] > 0:
        ex = tuple(np.asarray(e, np.float32)[kept] for e in extra)
        if not all(np.all(np.isfinite(e)) for e in ex):
            return fail(NOT_FINITE)
    if M == 1:
        out["status"] = NO_MOTION
        if want_samples:
            out["samples"], out["sample_vel"] = np.tile(P[-1].astype(F), (T, 1)), np.zeros((T, D), F)
            if T > 0:
                out["samples"][0] = P[0]
        return out
    if M == 2:
        return fail(TOO_FEW_WAYPOINTS)
    if ex is not None and not np.all((ex[2] < 0) & (ex[3] > 0)):
        return fail(INFEASIBLE)
    Q = P[kept].astype(F)
    d, m, c = geometry(Q)
    cap = speed_cap(d, vmax, vs)
    # ---- 6. backward pass
    kmax = np.zeros(M, F)
    for i in range(M - 2, 0, -1):
        rows = interval_rows(m, c, amax, ex, i)
        norm = _normalise(*rows)
        kn = kmax[i + 1]
        if _feasible(rows, norm, cap[i], kn):
            kmax[i] = cap[i]
            continue
        lo_x, hi_x = F(0), cap[i]
        for _ in range(nb):
            mid = F(0.5) * (lo_x + hi_x)
            if _feasible(rows, norm, mid, kn):
                lo_x = mid
            else:
                hi_x = mid
        kmax[i] = lo_x
    # ---- 7. forward pass, 8. times
    x, t = np.zeros(M, F), np.zeros(M, F)
    for i in range(M - 1):
        rows = interval_rows(m, c, amax, ex, i)
        p, q, r, nz = _normalise(*rows)
        xi = x[i]
        with np.errstate(invalid="ignore", over="ignore"):
            u = np.fmin(np.fmin.reduce(q - r * xi), F(0.5) * (kmax[i + 1] - xi))
        u = max(u, F(-0.5) * xi)
        xn = max(xi + F(2) * u, F(0))
        if i + 1 == M - 1:
            xn = F(0)
        x[i + 1] = xn
        den = np.sqrt(xi) + np.sqrt(xn)
        if not den > 0:
            return fail(INFEASIBLE)
        t[i + 1] = t[i] + F(2) / den
    return finish(out, P, kept, x, t, dt, T, want_samples)


def expand(v, kept, K):
    """a value per kept waypoint in the caller's indexing: a dropped waypoint repeats the waypoint kept before it"""
    pos = np.searchsorted(kept, np.arange(K), side="right") - 1
    return v[pos]


def finish(out, P, kept, x, t, dt, T, want_samples=True):
    """steps 8 (the duration) and 9 on a given x and t over the kept waypoints, in their dtype"""
    F = x.dtype.type
    K, D = P.shape
    M = len(kept)
    out["x"], out["t"], out["duration"] = expand(x, kept, K), expand(t, kept, K), t[-1]
    ns = int(np.ceil(t[-1] / dt)) + 1
    out["n_samples"] = ns
    if not want_samples:
        return out
    if ns > T:
        out["status"] = TRUNCATED
    Q = P[kept].astype(F)
    S, V = np.zeros((T, D), F), np.zeros((T, D), F)   # (the port's samples are float32, the reference's float64)
    for n in range(T):
        tau = F(n) * dt
        if n == 0:
            S[n] = P[0]   # (x_0 = 0: at rest)
            continue
        if not tau < t[-1]:
            S[n] = P[-1]
            continue
        i = min(int(np.searchsorted(t, tau, side="right")) - 1, M - 2)
        delta = tau - t[i]
        sx, u = np.sqrt(x[i]), (x[i + 1] - x[i]) * F(0.5)
        f = min(max(sx * delta + (u * delta) * delta * F(0.5), F(0)), F(1))
        di = Q[i + 1] - Q[i]
        S[n] = Q[i] + f * di
        V[n] = di * (sx + u * delta)
    out["samples"], out["sample_vel"] = S, V
    return out


def times_from_x(xk, F=np.float64):
    """step 8 in F on an x over the kept waypoints"""
    s = np.sqrt(xk.astype(F))
    t = np.zeros(len(xk), F)
    t[1:] = np.cumsum(F(2) / (s[:-1] + s[1:]))
    return t


def retime(paths, vmax, amax, dt, T=0, max_path_speed=None, extra=None, dtype=np.float64, want_samples=True):
    """all rows of a call: paths (R, K, D), extra = None or four (R, K, E) arrays -> dict of stacked results"""
    rows = [retime_row(paths[r], vmax, amax, dt, T, max_path_speed, None if extra is None else tuple(e[r] for e in extra), dtype, want_samples)
            for r in range(paths.shape[0])]
    return {k: np.stack([np.asarray(o[k]) for o in rows]) for k in rows[0]}


def row_violation(P, x, vmax, amax, max_path_speed, extra=None):
    """An x (K,) in the caller's indexing judged in float64 on its own: with u_i = (x_{i+1} - x_i) / 2 on the kept waypoints, the
    largest overshoot of a row of step 5 relative to that row's limit, and the largest x_i / cap_i - 1.  -> (rows, cap)"""
    P = np.asarray(P)
    kept = compact(P)
    Q = P[kept].astype(np.float64)
    xk = np.asarray(x, np.float64)[kept]
    d, m, c = geometry(Q)
    cap = speed_cap(d, np.asarray(vmax, np.float64), float(max_path_speed))
    ex = None if extra is None or extra[0].shape[1] == 0 else tuple(np.asarray(e, np.float64)[kept] for e in extra)
    worst = 0.0
    for i in range(len(kept) - 1):
        a, b, lo, hi = interval_rows(m, c, np.asarray(amax, np.float64), ex, i)
        u = 0.5 * (xk[i + 1] - xk[i])
        v = a * u + b * xk[i]
        worst = max(worst, float(np.max(np.maximum((v - hi) / np.abs(hi), (lo - v) / np.abs(lo)))))
    return worst, float(np.max(xk / cap - 1.0))


def refine(P, r):
    """every segment of P (K, D) split into r equal parts: ((K - 1) r + 1, D), the points stay on the polyline"""
    P = np.asarray(P, np.float32)
    f = (np.arange(r, dtype=np.float32) / np.float32(r))[None, :, None]
    body = P[:-1, None, :] + f * (P[1:, None, :] - P[:-1, None, :])
    return np.concatenate([body.reshape(-1, P.shape[1]), P[-1:]], 0)


def compact_differences(P):
    """m and c of step 2 at every waypoint of the caller's path P (K, D), in float64, taken over the KEPT waypoints (the neighbours of a
    kept waypoint are the waypoints kept before and after it); at a dropped waypoint the values of the waypoint kept before it"""
    P = np.asarray(P, np.float32)
    kept = compact(P)
    if len(kept) < 2:
        z = np.zeros(P.shape, np.float64)
        return z, z.copy()
    _, m, c = geometry(P[kept].astype(np.float64))
    return expand(m, kept, P.shape[0]), expand(c, kept, P.shape[0])
