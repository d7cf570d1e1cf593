"""The scenes, start rows and paths of the certified-clearance tests, shared by tests/test_cert_cpu.py (which holds the conditions the GPU
tests lean on) and tests/test_gpu_cert.py.  A helper, no test.  B = 5 rows; the Franka cases use the scenes, start rows and the coarse
sphere model (N = 57) of tests/plan_cases.py; states are SET.

    clear       the straight edge start -> goal of plan_cases "clear", K = 2: CLEAR in a few evaluations.
    post_line   the straight edge of "post", K = 2: BLOCKED by a witness.
    detour      the float64 reference polyline of "post" per row, padded to a common K by repeating the last node: CLEAR at margin 0,
                BRACKET mode, zero-length segments.
    thin        row 0 of "clear" five times (rows 1 - 4 jittered by 0.4 mrad) plus one fixed sphere of radius 1 cm (THIN) that the arm
                sweeps through between two samples of the edge rule at resolution 0.1, in a gap whose midpoint is not t = 1/2: the
                sampled check passes, certification does not.
    deep_tree   tree_cases "deep" (15 joints in one chain, prismatic at every fourth) plus one world sphere; 8 probes on the last four
                links, all 15 joints planned, the ground skipped: S with prismatic joints mid-chain.
    budget, depth, nan   detour with max_evaluations = 8, with max_depth = 2 and tol = 1e-4, with a NaN in one waypoint.

THIN was found by derive_thin() below (float64): row 0 of "clear", the gap between samples 3 and 4 of 5 (t = 0.6 .. 0.8); over every
probe and 400 directions, the sphere pushed 4.5 mm into that probe at t = 0.7 from the direction that leaves the rule's own six samples
the most clearance.  tests/test_cert_cpu.py checks what it promises.
"""
from __future__ import annotations

import functools

import numpy as np

import cert_ref
import plan_cases as pc
import plan_ref
import tree_cases
from gym_genesis.backend import spec as S

B = pc.B
TOL, GUARD, MAX_DEPTH, MAX_EVAL = 0.002, 1e-5, 12, 4096
THIN_RADIUS, THIN_RESOLUTION, THIN_T = 0.01, 0.1, 0.7
THIN = (0.25410137, -0.46128893, 0.4837938)   # derive_thin(0.0045): the rule's samples keep +5.2 mm, t = 0.7 lies 4.5 mm inside
DEEP_SPHERE = dict(size=(0.05, 0.0, 0.0), pos=(0.9, 0.4, 0.3))
NAMES = ("clear", "post_line", "detour", "thin", "deep_tree", "budget", "depth", "nan")


def _franka(base, extra_sphere=None):
    c = pc.case(base)
    if extra_sphere is None:
        return dict(c)
    sb = pc.builder(base)
    sb.add_geom(0, S.GEOM_SPHERE, size=(THIN_RADIUS, 0.0, 0.0), pos=tuple(extra_sphere), rgb=(0.9, 0.2, 0.2))
    out = dict(c)
    out.update(sb=sb, spec=sb.build())
    return out


@functools.lru_cache(maxsize=None)
def detour_paths():
    """(B, K, D) float32: the float64 reference polylines of "post", padded by repeating the last node"""
    polys = [pc.reference("post", r)["poly"] for r in range(B)]
    assert all(pc.reference("post", r)["status"] == plan_ref.OK for r in range(B))
    K = max(len(p) for p in polys)
    out = np.stack([np.concatenate([p, np.repeat(p[-1:], K - len(p), 0)]) for p in polys]).astype(np.float32)
    assert 3 <= K <= 8, K
    return out


@functools.lru_cache(maxsize=None)
def _deep():
    sb, _ = tree_cases.build("deep")
    sb.add_geom(0, S.GEOM_SPHERE, **DEEP_SPHERE)
    spec = sb.build()
    model = plan_ref.kin_ref.Model(spec)
    rng = np.random.default_rng(211)
    links = np.repeat(np.arange(spec.nbody - 4, spec.nbody), 2).astype(np.int32)
    probes = np.concatenate([rng.uniform(-0.08, 0.08, (8, 3)), rng.uniform(0.02, 0.05, (8, 1))], 1).astype(np.float32)
    qadr = np.array([model.qadr[b] for b in range(1, spec.nbody) if model.jtype[b] in (plan_ref.kin_ref.REVOLUTE, plan_ref.kin_ref.PRISMATIC)], np.int32)
    lim = np.array([2.0 if model.jtype[b] == plan_ref.kin_ref.REVOLUTE else 0.15 for b in range(1, spec.nbody)])
    start = rng.uniform(-0.5, 0.5, (B, len(qadr))) * lim
    steps = rng.uniform(-0.06, 0.06, (B, 2, len(qadr))) * lim
    paths = np.stack([start, start + steps[:, 0], start + steps[:, 0] + steps[:, 1]], 1).astype(np.float32)
    q = np.zeros((B, model.nq), np.float32)
    q[:, qadr] = paths[:, 0]
    return dict(sb=sb, spec=spec, probes=probes, links=links, skip=1, qadr=qadr, q=q, paths=paths)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(spec, sb, probes, links, skip, qadr, q (B, nq), paths (B, K, D) float32, par: the keywords of the call, max_distance,
    base: the case whose scene and dense minima it shares)"""
    par = dict(margin=0.0, tol=TOL, guard=GUARD, max_depth=MAX_DEPTH, max_evaluations=MAX_EVAL, bracket=False)
    if name == "clear":
        c = _franka("clear")
        paths = np.stack([c["start"], c["goal"]], 1)
    elif name == "post_line":
        c = _franka("post")
        paths = np.stack([c["start"], c["goal"]], 1)
    elif name in ("detour", "budget", "depth", "nan"):
        c = _franka("post")
        paths = detour_paths().copy()
        if name == "budget":
            par.update(max_evaluations=8)
        elif name == "depth":
            par.update(max_depth=2, tol=1e-4)
        elif name == "nan":
            paths[1, 1, 3] = np.nan
    elif name == "thin":   # every row is row 0 of "clear" (THIN is placed for it) but for a jitter of 0.4 mrad in joints 1 - 6
        c = _franka("clear", THIN)
        jit = np.zeros((2, B, 9))
        jit[:, 1:, 1:7] = np.random.default_rng(77).uniform(-4e-4, 4e-4, (2, B - 1, 6))   # (joint 0 sets the rule's 5 samples: kept)
        start, goal = (c["start"][:1] + jit[0]).astype(np.float32), (c["goal"][:1] + jit[1]).astype(np.float32)
        q = np.repeat(c["q"][:1], B, 0)
        q[:, c["qadr"]] = start
        c.update(q=q, start=start, goal=goal)
        paths = np.stack([start, goal], 1)
    elif name == "deep_tree":
        c = dict(_deep())
        paths = c["paths"]
    else:
        raise KeyError(name)
    c = dict(c)
    c.update(paths=np.ascontiguousarray(paths, np.float32), par=par, max_distance=4.0 if name == "deep_tree" else 1.0,
             base="detour" if name in ("budget", "depth", "nan") else name, scene={"clear": "clear", "thin": "thin", "deep_tree": "deep_tree"}.get(name, "post"))
    return c


def problem(name, dtype=np.float64):
    c = case(name)
    return plan_ref.Problem(c["spec"], c["probes"], c["links"], c["qadr"], c["skip"], c["max_distance"], dtype)


@functools.lru_cache(maxsize=None)
def reference(name, row, dtname="float64", bracket=None):
    """cert_ref.certify of one row of a case (computed once, shared)"""
    c = case(name)
    par = dict(c["par"])
    if bracket is not None:
        par["bracket"] = bracket
    return cert_ref.certify(problem(name, np.dtype(dtname).type), c["q"][row], c["paths"][row], **par)


@functools.lru_cache(maxsize=None)
def dense(name, row, n=2048):
    """the brute-force minimum per segment of one row (float64; NaN waypoints: of the case it was made from)"""
    c = case(case(name)["base"])
    return cert_ref.dense_min(problem(c["base"]), c["q"][row], c["paths"][row], n)


def derive_thin(depth=0.0035, n_dir=400):
    """how THIN was found (float64, a second or two): -> (position, lowest clearance over the rule's samples, clearance at THIN_T)"""
    c = pc.case("clear")
    pb = pc.problem("clear")
    a, b = c["start"][0].astype(np.float64), c["goal"][0].astype(np.float64)
    pb.set_row(c["q"][0])
    samples = [a] + plan_ref.edge_samples(a, b, THIN_RESOLUTION, np.float64)
    assert len(samples) == 6
    at = np.stack([pb.centres(q).copy() for q in samples])           # (6, N, 3)
    mid = pb.centres(a + THIN_T * (b - a)).copy()                    # (N, 3)
    rad = np.asarray(pb.probes[:, 3], np.float64)
    k = np.arange(n_dir) + 0.5                                        # a Fibonacci lattice of directions
    z, phi = 1.0 - 2.0 * k / n_dir, np.pi * (1.0 + 5.0 ** 0.5) * k
    dirs = np.stack([np.sqrt(1.0 - z * z) * np.cos(phi), np.sqrt(1.0 - z * z) * np.sin(phi), z], 1)
    best = None
    for i in range(len(mid)):
        o = mid[i][None] + dirs * (rad[i] + THIN_RADIUS - depth)      # the sphere pushed `depth` into probe i at THIN_T
        gap = (np.linalg.norm(at[None] - o[:, None, None], axis=3) - rad[None, None]).min((1, 2)) - THIN_RADIUS
        hit = (np.linalg.norm(mid[None] - o[:, None], axis=2) - rad[None]).min(1) - THIN_RADIUS
        gap = np.where(o[:, 2] > 0.05, gap, -1.0)                     # (off the ground)
        w = int(gap.argmax())
        if best is None or gap[w] > best[1]:
            best = (o[w], float(gap[w]), float(hit[w]))
    return best
