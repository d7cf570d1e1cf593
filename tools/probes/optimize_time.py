"""Developer probe: what one optimize_path call (mir_optimize_path) costs and, measured in the same run, the two calls its cost should be
read against: get_path_clearance of the same paths (one sweep: an optimiser pass is of the order of a one-sample-per-segment sweep) and
plan_path for the same envs.  Device events around queued calls, for the Franka of the pick scene with a fixed box post between start
and goal (the scene of plan_time.py and blend_time.py), the gripper held at 0.02.  4096 envs by default, the entity's default sphere
model, K = 32 waypoints.

    python tools/probes/optimize_time.py [--envs 4096] [--waypoints 32] [--calls 3] [--rounds 5]

  (a) optimize_path, the defaults          (b) get_path_clearance of the seeds       (c) plan_path for the same envs
  (d) as (a) with max_iterations 10        (e) as (a) with the self test on          (f) as (a) with ignore_collision
Every variant is warmed up, then timed in `rounds` interleaved windows of `calls` back-to-back calls between two events; the median,
the minimum and the maximum over the rounds are printed, with the outcome of the calls.  The times include the Python wrapper and the
allocation of the outputs, as a caller pays them."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "gym-genesis_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gym_genesis.backend import models  # noqa: E402
from gym_genesis.backend import spec as S  # noqa: E402
from gym_genesis.backend.lib import MirScene  # noqa: E402
from gym_genesis.tasks.views import EntityView  # noqa: E402

START = (-0.9, -0.4, 0.0, -2.2, 0.0, 2.0, 0.8, 0.02, 0.02)
GOAL = (0.9, -0.35, 0.05, -2.1, 0.0, 1.9, 0.7, 0.02, 0.02)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--waypoints", type=int, default=32)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    B, W = a.envs, a.waypoints
    sb = models.franka_cube_pick_scene()
    sb.add_geom(0, S.GEOM_BOX, size=(0.04, 0.04, 0.25), pos=(0.45, 0.0, 0.25))
    sc = MirScene(sb.build(), B)
    robot = EntityView(sc, sb, "link0", models.FRANKA_JOINTS)
    rng = np.random.default_rng(0)
    jit = np.zeros((2, B, 9), np.float32)
    jit[:, :, :7] = rng.uniform(-0.04, 0.04, (2, B, 7))
    q = sc.get_state()[0].clone()
    q[:, robot._qcols] = torch.as_tensor(np.array(START, np.float32) + jit[0], device=sc.device)
    sc.set_state(qpos=q, qvel=torch.zeros((B, sc.nv), device=sc.device))
    goal = torch.as_tensor(np.array(GOAL, np.float32) + jit[1], device=sc.device)
    off = dict(self_collision=False)
    seeds = robot.plan_path(goal, num_waypoints=W, return_detail=True, **off)
    path = seeds["path"]

    def opt(**kw):
        return robot.optimize_path(path, return_detail=True, **{**off, **kw})

    variants = {
        "(a) optimize_path, the defaults": lambda: opt(),
        "(b) get_path_clearance of the seeds": lambda: robot.get_path_clearance(path, **off),
        "(c) plan_path for the same envs": lambda: robot.plan_path(goal, num_waypoints=W, **off),
        "(d) optimize_path, max_iterations 10": lambda: opt(max_iterations=10),
        "(e) optimize_path, self test on": lambda: opt(self_collision=True),
        "(f) optimize_path, ignore_collision": lambda: opt(ignore_collision=True),
    }
    stats = {}
    for name, fn in variants.items():
        r = fn()
        torch.cuda.synchronize()
        if isinstance(r, dict):
            st = r["stats"].float()
            stats[name] = {"statuses": sorted(set(r["status"].tolist())), "stops": sorted(set(r["stats"][:, 5].tolist())),
                           "S_in_out": [round(float(r["cost"][:, 0].median()), 4), round(float(r["cost"][:, 2].median()), 4)],
                           **{n: [float(st[:, i].median()), float(st[:, i].max())] for i, n in enumerate(("iterations", "accepted", "halvings", "evaluated", "swept"))}}
        elif r.dim() == 1:
            stats[name] = {"clearance_min": float(r.min()), "waypoints": W}
        else:
            stats[name] = {"waypoints": W}
    times = {name: [] for name in variants}
    for _ in range(a.rounds):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.calls)
    out = {"envs": B, "spheres": len(robot.collision_spheres()[1]), "waypoints": W, "plans_ok": int(seeds["valid"].sum()), "calls_per_window": a.calls,
           "rounds": a.rounds, "variants": {}}
    for name in variants:
        t = sorted(times[name])
        out["variants"][name] = {"ms_per_call_median": round(t[len(t) // 2], 3), "ms_per_call_min": round(t[0], 3), "ms_per_call_max": round(t[-1], 3),
                                 "outcome": stats[name]}
        print(f"{name:40s} median {t[len(t) // 2]:9.3f} ms   min {t[0]:9.3f} ms   max {t[-1]:9.3f} ms   {stats[name]}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
