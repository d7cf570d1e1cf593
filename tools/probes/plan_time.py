"""Developer probe: time of EntityView.plan_path (mir_plan_path) and get_path_clearance (mir_path_clearance) per call, with device events
around queued calls, for the Franka of the pick scene with a fixed box post in front of it.  4096 envs by default.

    python tools/probes/plan_time.py [--envs 4096] [--calls 5] [--rounds 5] [--waypoints 100]

  (a) direct edge: a goal whose straight segment is clear (start, goal and one edge are checked, no search)
  (b) detour: start and goal on either side of the post (RRT-Connect, 64 shortcut attempts, resampling)
  (c) the same without smoothing                        (d) get_path_clearance of the paths of (b)
Starts and goals are jittered per env.  Every variant is warmed up, then timed in `rounds` interleaved windows of `calls` back-to-back
calls between two events; the median and the minimum over the rounds are printed with the statistics of the plans: the share of rows
with a plan, iterations, nodes and configurations checked per row.  The times include the Python wrapper and the allocation of the
outputs, as a caller pays them."""
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
ACROSS = (0.9, -0.35, 0.05, -2.1, 0.0, 1.9, 0.7, 0.04, 0.04)
NEAR = (-1.4, -0.2, 0.1, -1.9, 0.1, 1.8, 0.6, 0.02, 0.02)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--waypoints", type=int, default=100)
    a = ap.parse_args()
    B = a.envs
    sb = models.franka_cube_pick_scene()
    sb.add_geom(0, S.GEOM_BOX, size=(0.04, 0.04, 0.25), pos=(0.45, 0.0, 0.25))
    sc = MirScene(sb.build(), B)
    robot = EntityView(sc, sb, "link0", models.FRANKA_JOINTS)
    rng = np.random.default_rng(0)
    jit = np.zeros((3, B, 9), np.float32)
    jit[:, :, :7] = rng.uniform(-0.04, 0.04, (3, B, 7))
    q = sc.get_state()[0].clone()
    q[:, robot._qcols] = torch.as_tensor(np.array(START, np.float32) + jit[0], device=sc.device)
    sc.set_state(qpos=q, qvel=torch.zeros((B, sc.nv), device=sc.device))
    across = torch.as_tensor(np.array(ACROSS, np.float32) + jit[1], device=sc.device)
    near = torch.as_tensor(np.array(NEAR, np.float32) + jit[2], device=sc.device)
    W = a.waypoints
    paths = robot.plan_path(across, num_waypoints=W)
    variants = {
        "(a) plan_path, direct edge": lambda: robot.plan_path(near, num_waypoints=W, return_detail=True),
        "(b) plan_path, detour round the post": lambda: robot.plan_path(across, num_waypoints=W, return_detail=True),
        "(c) the same, smooth_path=False": lambda: robot.plan_path(across, num_waypoints=W, smooth_path=False, return_detail=True),
        "(d) get_path_clearance of (b)'s paths": lambda: robot.get_path_clearance(paths),
    }
    stats = {}
    for k, fn in variants.items():
        r = fn()
        torch.cuda.synchronize()
        if isinstance(r, dict):
            st = r["stats"].float()
            stats[k] = {"valid": float(r["valid"].float().mean()), "n_poly_mean": float(r["n_poly"].float().mean()),
                        **{n: [float(st[:, i].median()), float(st[:, i].mean()), float(st[:, i].max())]
                           for i, n in enumerate(("iterations", "nodes_a", "nodes_b", "checked"))}}
    times = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / a.calls)
    out = {"envs": B, "spheres": len(robot.collision_spheres()[1]), "waypoints": W, "calls_per_window": a.calls, "rounds": a.rounds, "variants": {}}
    for k in variants:
        t = sorted(times[k])
        out["variants"][k] = {"ms_per_call_median": round(t[len(t) // 2], 3), "ms_per_call_min": round(t[0], 3), **({"plans": stats[k]} if k in stats else {})}
        print(f"{k:40s} median {t[len(t) // 2]:9.3f} ms   min {t[0]:9.3f} ms   {stats.get(k, '')}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
