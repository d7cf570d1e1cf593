"""The scenes, start rows, models and paths of the tests of mir_certify_path_self / mir_certify_path_carry, shared by
tests/test_certrel_cpu.py (which holds the conditions the GPU tests lean on) and tests/test_gpu_certrel.py.  A helper, no test.
R = B = 5 rows, K <= 8; the arm is the Franka of the pick scene with the coarse sphere model of tests/plan_cases.py (57 spheres) plus the 8
spheres of its bolted base, which take part in the self test only; states are SET.  Every row is judged in every case.

    self_clear   the first 47 % of self_cases "fold" (joints 2 and 5 fold the forearm towards the upper arm) in two segments, K = 3:
                 CLEAR, the self clearance stays >= 1 cm.
    self_thin    the path of cert_cases "thin" (row 0 of plan_cases "clear" five times, jittered by 0.4 mrad) on the scene WITHOUT that
                 case's thin geom; instead a self-only sphere of radius 1 cm rides on the base link (link0) where cert_cases.THIN is:
                 a finger sphere sweeps through it between samples 3 and 4 of the edge rule at resolution 0.1.  Sampled clear,
                 certified BLOCKED through self_upper.
    common       only joint 1 moves, by 2 rad, K = 2, from the start rows of "fold"; every geom is skipped, max_distance = 4 (the scene
                 test closes at its first node: 4 - v / 2 - guard >= 0 for any v <= 7.9) and the base link is masked off, so every
                 enabled pair hangs below joint 1 and every v_ij is 0: three evaluations per row.  "common_capped" is the same call
                 with self_max = 2^-5, below the lowest pair distance, where the three evaluations return the same bits.
    carry_clear  carry_cases "under" (the cube in the fingers, a post beside it): start -> the goal of plan_cases "clear", which takes
                 the cube away from the post: CLEAR.   carry_given: the same with the grasp handed over as (R, 7).
    carry_under  the straight edge of "under", which drags the cube through the post the hand itself clears: BLOCKED by the scene test
                 of a carried sphere.
    carry_arm    carry_cases "rod": a segment of 0.1998 rad (two samples at resolution 0.1) on which a rod sphere dips 1.5 mm into a
                 sphere of link1 (the shoulder link the folded elbow brings the hand back to; on this sweep the rod stays 10 cm from
                 the forearm links) at t = 1/4, between the start and the first sample.  Found by derive_carry_arm() below (float64): the
                 configuration where the rod leaves the arm on the straight edge of "rod", left along the joint-space direction,
                 tangent to the clearance, that keeps the rule's samples clearest.  Sampled clear, certified BLOCKED through self_upper.
    budget, depth, nan   self_clear with max_evaluations = 8, with max_depth = 2 and tol = 1e-4, with a NaN in one waypoint.
    nan_grasp    carry_given with a NaN in the grasp of row 2: every segment of that row NOT_FINITE.

Jitter: rows 1 - 4 of self_thin and carry_arm differ from row 0 by 0.4 mrad (seeds 77 and 95), because the thin sphere and the tangent
direction are placed for row 0; every other case takes the +-0.04 rad rows of the case it is made from.  With these seeds the float64
reference alone meets the conditions of tests/test_certrel_cpu.py (minima >= 2.9 mm clear of the margins, witnesses >= 1 mm under) on all
five rows.
"""
from __future__ import annotations

import functools

import numpy as np

import carry_cases
import carry_ref
import cert_cases
import certrel_ref
import plan_cases as pc
import plan_ref
import self_cases
import self_ref

B = pc.B
TOL, GUARD, MAX_DEPTH, MAX_EVAL = 0.002, 1e-5, 12, 4096
THIN_RADIUS, THIN_RESOLUTION, THIN = cert_cases.THIN_RADIUS, cert_cases.THIN_RESOLUTION, cert_cases.THIN
BASE_LINK = 1   # link0, bolted to the floor
SELF_CLEAR_T = (0.0, 0.235, 0.47)
COMMON_TURN, COMMON_MAX_DISTANCE, COMMON_CAP = 2.0, 4.0, 2.0 ** -5
# derive_carry_arm(): the configuration of the dip and the direction of the segment (row 0 of "rod")
ARM_Q = (0.0, -0.30000001192092896, 0.0, -2.7820000648498535, -0.9297581717729568, 0.6999320065915584, 2.4049999713897705, 0.04, 0.04)
ARM_U = (-0.11631635382451012, -0.9980585206814375, -0.3013168237568464, 0.9997585844257582, 0.40511304769004486, 1.0, 0.9989002028551975, 0.0, 0.0)
ARM_BACK, ARM_AHEAD, ARM_RESOLUTION = 0.04995, 0.14985, 0.1
NAMES = ("self_clear", "self_thin", "common", "common_capped", "carry_clear", "carry_given", "carry_under", "carry_arm", "budget", "depth", "nan",
         "nan_grasp")


def _rod_rows(c, start, grasp):
    """the start rows of a carry case with the arm at `start` (B, D) and the carried body where the hand and `grasp` (B, 7) put it"""
    q = c["q"].copy()
    q[:, c["qadr"]] = start
    model = plan_ref.kin_ref.Model(c["spec"])
    fk = plan_ref.Problem(c["spec"], c["probes"][:1], c["links"][:1], c["qadr"], c["skip"], 1.0, np.float64)
    qc = model.qadr[c["body"]]
    for r in range(B):
        fk.set_row(q[r])
        q[r, qc:qc + 3] = fk.xp[c["link"]] + plan_ref._qrot(fk.xq[c["link"]], grasp[r, :3])
        q[r, qc + 3:qc + 7] = plan_ref._qmul(fk.xq[c["link"]], grasp[r, 3:])
    return q


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(sb, spec, probes (N + E, 4), links, n_extra, mask (32,) or None (no self query), carry (body, link) or None, grasp (B, 7)
    float32 or None (from the start row), skip, qadr, q (B, nq) float32, paths (B, K, D) float32, par: the keywords of the call,
    max_distance, self_margin, self_max, base: the case whose scene, rows and dense minima it shares, kind: "self" or the carry case)"""
    par = dict(margin=0.0, tol=TOL, guard=GUARD, max_depth=MAX_DEPTH, max_evaluations=MAX_EVAL, bracket=False)
    out = dict(carry=None, grasp=None, max_distance=1.0, self_margin=0.0, self_max=1.0, base=name)
    if name in ("self_clear", "budget", "depth", "nan"):
        c = self_cases.case("fold")
        d = c["goal"].astype(np.float64) - c["start"].astype(np.float64)
        paths = np.stack([c["start"].astype(np.float64) + t * d for t in SELF_CLEAR_T], 1)
        paths[:, 0] = c["start"]
        out.update(c, kind="self", base="self_clear")
        if name == "budget":
            par.update(max_evaluations=8)
        elif name == "depth":
            par.update(max_depth=2, tol=1e-4)
        elif name == "nan":
            paths[1, 1, 3] = np.nan
    elif name == "self_thin":
        c, t = self_cases.case("fold"), cert_cases.case("thin")
        out.update(c, kind="self", q=t["q"], start=t["start"], goal=t["goal"])
        out["probes"] = np.concatenate([c["probes"], [[*THIN, THIN_RADIUS]]]).astype(np.float32)   # (link0 stands at the world's origin)
        out["links"] = np.concatenate([c["links"], [BASE_LINK]]).astype(np.int32)
        out["n_extra"] = c["n_extra"] + 1
        paths = t["paths"]
    elif name in ("common", "common_capped"):
        c = self_cases.case("fold")
        goal = c["start"].copy()
        goal[:, 0] += np.float32(COMMON_TURN)
        mask = c["mask"].copy()
        mask[BASE_LINK] = 0
        mask &= ~np.uint32(1 << BASE_LINK)
        out.update(c, kind="self", mask=mask, skip=(1 << len(c["sb"].geoms)) - 1, max_distance=COMMON_MAX_DISTANCE, base="common")
        if name == "common_capped":
            out["self_max"] = COMMON_CAP
        paths = np.stack([c["start"], goal], 1)
    elif name in ("carry_clear", "carry_given", "carry_under", "nan_grasp"):
        c = carry_cases.case("under")
        out.update(c, kind="under", carry=(c["body"], c["link"]), grasp=None, base="carry_under" if name == "carry_under" else "carry_clear")
        paths = np.stack([c["start"], c["goal"] if name == "carry_under" else pc.case("clear")["goal"]], 1)
        if name in ("carry_given", "nan_grasp"):
            out["grasp"] = given_grasp()
            if name == "nan_grasp":
                out["grasp"] = out["grasp"].copy()
                out["grasp"][2, 1] = np.nan
                out["base"] = "nan_grasp"
    elif name == "carry_arm":
        c = carry_cases.case("rod")
        jit = np.zeros((B, 9))
        jit[1:, :7] = np.random.default_rng(95).uniform(-4e-4, 4e-4, (B - 1, 7))
        at, u = np.array(ARM_Q)[None] + jit, np.array(ARM_U)
        paths = np.stack([at - ARM_BACK * u, at + ARM_AHEAD * u], 1).astype(np.float32)
        out.update(c, kind="rod", carry=(c["body"], c["link"]), grasp=None)
        out["q"] = _rod_rows(c, paths[:, 0], np.repeat(c["grasp"][:1], B, 0))   # (every row holds the rod as row 0 does: the dip is placed for it)
    else:
        raise KeyError(name)
    out.update(paths=np.ascontiguousarray(paths, np.float32), par=par)
    return out


@functools.lru_cache(maxsize=None)
def given_grasp():
    """(B, 7) float32: the grasp the float32 port takes from the start rows of "under" -- handed over, it must give what NULL gives"""
    c = carry_cases.case("under")
    pb = carry_cases.problem("under", np.float32)
    out = []
    for r in range(B):
        pb.grasp = None
        pb.set_row(c["q"][r])
        out.append(pb.grasp_used())
    return np.stack(out).astype(np.float32)


def self_on(name):
    return case(name)["mask"] is not None


def problem(name, dtype=np.float64):
    c = case(name)
    if c["carry"] is None:
        return self_ref.SelfProblem(c["spec"], c["probes"], c["links"], c["qadr"], c["n_extra"], c["mask"], c["skip"], c["max_distance"],
                                    c["self_margin"], c["self_max"], dtype)
    return carry_ref.CarryProblem(c["spec"], c["probes"], c["links"], c["qadr"], c["n_extra"], c["mask"], c["carry"][0], c["carry"][1], c["skip"],
                                  c["max_distance"], c["self_margin"], c["self_max"], dtype)


@functools.lru_cache(maxsize=None)
def _problem(name, dtname):
    return problem(name, np.dtype(dtname).type)


def row_problem(name, row, dtname="float64"):
    """the (shared) problem of a case with the row's grasp in place"""
    c, pb = case(name), _problem(name, dtname)
    if c["carry"] is not None:
        pb.grasp = None if c["grasp"] is None else c["grasp"][row]
    return pb


@functools.lru_cache(maxsize=None)
def reference(name, row, dtname="float64", bracket=None):
    """certrel_ref.certify of one row of a case (computed once, shared)"""
    c = case(name)
    par = dict(c["par"])
    if bracket is not None:
        par["bracket"] = bracket
    return certrel_ref.certify(row_problem(name, row, dtname), c["q"][row], c["paths"][row], self_on=self_on(name), **par)


@functools.lru_cache(maxsize=None)
def dense(name, row, n=2048):
    """the brute-force minima per segment of one row, (scene, self), float64; of the case it was made from (NaN waypoints and grasps)"""
    base = case(name)["base"]
    if base == "nan_grasp":
        base = "carry_given"
    c = case(base)
    return certrel_ref.dense_min(row_problem(base, row), c["q"][row], c["paths"][row], n)


def derive_carry_arm(depth=0.0015, seed=1):
    """how ARM_Q and ARM_U were found (float64, about a minute): -> (q, u, the lowest self clearance at the rule's samples, at the dip)"""
    c, pb = carry_cases.case("rod"), carry_cases.problem("rod")
    pb.set_row(c["q"][0])
    a, b = c["start"][0].astype(np.float64), c["goal"][0].astype(np.float64)
    both = lambda Q: certrel_ref.both_batch(pb, np.atleast_2d(Q))  # noqa: E731
    ts = np.linspace(0.55, 0.70, 3001)
    own = both(a[None] + ts[:, None] * (b - a)[None])[1]
    qs = a + ts[int(np.argmax(own >= -depth))] * (b - a)   # (where the rod leaves the arm, `depth` before it is out)
    g, h = np.zeros(9), 1e-6
    for j in range(7):
        e = np.zeros(9)
        e[j] = h
        g[j] = (both(qs + e)[1][0] - both(qs - e)[1][0]) / (2 * h)

    def value(u):
        u = u - (u @ g) / (g @ g) * g
        u = u / np.abs(u).max()
        s, o = both(np.stack([qs - 0.05 * u, qs + 0.05 * u, qs + 0.15 * u]))
        return min(o.min(), s.min()), u

    rng = np.random.default_rng(seed)
    best, bu = -1.0, None
    for _ in range(1500):
        u = np.zeros(9)
        u[:7] = rng.uniform(-1, 1, 7)
        v, cu = value(u)
        if v > best:
            best, bu = v, cu
    for sig in (0.3, 0.1, 0.03):
        for _ in range(800):
            cand = bu.copy()
            cand[:7] += rng.normal(0, sig, 7)
            v, cu = value(cand)
            if v > best:
                best, bu = v, cu
    return qs, bu, best, float(both(qs)[1][0])
