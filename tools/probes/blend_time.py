"""Developer probe: what rounding the corners of a plan costs in one blend_path call (mir_blend_path) and, measured in the same run, one
get_path_clearance of the dense points it returns -- both are clear(q) calls on the same sphere model, so they should be of the same
order.  Device events around queued calls, for the Franka of the pick scene with a fixed box post between start and goal (the scene of
plan_time.py).  4096 envs by default, the entity's default sphere model.  The polylines are those robot.plan_path returns for the envs.

    python tools/probes/blend_time.py [--envs 4096] [--calls 5] [--rounds 5]

  (a) blend_path of the plans' polylines, dense points     (b) get_path_clearance of those dense points
  (c) as (a) with 32 waypoints resampled                   (d) as (a) with the self test on      (e) as (a) with ignore_collision
Starts and goals are jittered per env.  Every variant is warmed up, then timed in `rounds` interleaved windows of `calls` back-to-back
calls between two events; the median, the minimum and the maximum over the rounds are printed, with the outcome of the calls.  The times
include the Python wrapper and the allocation of the outputs, as a caller pays them."""
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

START = (-0.9, -0.4, 0.0, -2.2, 0.0, 2.0, 0.8, 0.04, 0.04)
GOAL = (0.9, -0.35, 0.05, -2.1, 0.0, 1.9, 0.7, 0.04, 0.04)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    B = a.envs
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
    plan = robot.plan_path(goal, num_waypoints=16, return_detail=True, **off)
    poly, n_poly = plan["poly"], plan["n_poly"]
    K = int(n_poly.max())
    poly = poly[:, :max(K, 2)].contiguous()   # (the nodes any env uses: the capacity of the dense points follows K)

    def blend(**kw):
        return robot.blend_path(poly, n_poly, return_detail=True, **{**off, **kw})

    dense = blend()["path"]
    variants = {
        "(a) blend_path, dense points": lambda: blend(),
        "(b) get_path_clearance of the dense points": lambda: robot.get_path_clearance(dense, **off),
        "(c) blend_path, 32 waypoints": lambda: blend(num_waypoints=32),
        "(d) blend_path, self test on": lambda: blend(self_collision=True),
        "(e) blend_path, ignore_collision": lambda: blend(ignore_collision=True),
    }
    stats = {}
    for name, fn in variants.items():
        r = fn()
        torch.cuda.synchronize()
        if isinstance(r, dict):
            st = r["stats"].float()
            stats[name] = {"statuses": sorted(set(r["status"].tolist())), "n_points_max": int(r["n_points"].max()),
                           **{n: [float(st[:, i].median()), float(st[:, i].max())] for i, n in enumerate(("nodes", "blended", "sharp", "checked"))}}
        else:
            stats[name] = {"clearance_min": float(r.min()), "points": int(dense.shape[0])}
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
    out = {"envs": B, "spheres": len(robot.collision_spheres()[1]), "plans_ok": int(plan["valid"].sum()), "nodes_max": K, "calls_per_window": a.calls,
           "rounds": a.rounds, "variants": {}}
    for name in variants:
        t = sorted(times[name])
        out["variants"][name] = {"ms_per_call_median": round(t[len(t) // 2], 3), "ms_per_call_min": round(t[0], 3), "ms_per_call_max": round(t[-1], 3),
                                 "outcome": stats[name]}
        print(f"{name:46s} median {t[len(t) // 2]:9.3f} ms   min {t[0]:9.3f} ms   max {t[-1]:9.3f} ms   {stats[name]}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
