"""Developer probe: what the self-collision test of the sphere model costs, with device events around queued calls, for the Franka of
the pick scene with a fixed box post in front of it (the scene of plan_time.py).  4096 envs by default, the entity's default models.

    python tools/probes/self_time.py [--envs 4096] [--calls 5] [--rounds 5] [--waypoints 100]

  (a) get_clearance (mir_signed_distance)               (b) get_self_clearance (mir_self_distance)
  (c) plan_path, detour round the post, self_collision off (mir_plan_path)      (d) the same, on (mir_plan_path_self)
  (e) get_path_clearance of (c)'s paths, off (mir_path_clearance)               (f) the same, on (mir_path_clearance_self)
Starts and goals are jittered per env.  Every variant is warmed up, then timed in `rounds` interleaved windows of `calls` back-to-back
calls between two events; the median and the minimum over the rounds are printed, with the statistics of the plans.  The times include
the Python wrapper and the allocation of the outputs, as a caller pays them."""
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
    jit = np.zeros((2, B, 9), np.float32)
    jit[:, :, :7] = rng.uniform(-0.04, 0.04, (2, B, 7))
    q = sc.get_state()[0].clone()
    q[:, robot._qcols] = torch.as_tensor(np.array(START, np.float32) + jit[0], device=sc.device)
    sc.set_state(qpos=q, qvel=torch.zeros((B, sc.nv), device=sc.device))
    across = torch.as_tensor(np.array(ACROSS, np.float32) + jit[1], device=sc.device)
    W = a.waypoints
    paths = robot.plan_path(across, num_waypoints=W)
    variants = {
        "(a) get_clearance": lambda: robot.get_clearance(),
        "(b) get_self_clearance": lambda: robot.get_self_clearance(),
        "(c) plan_path, detour, self_collision off": lambda: robot.plan_path(across, num_waypoints=W, self_collision=False, return_detail=True),
        "(d) plan_path, detour, self_collision on": lambda: robot.plan_path(across, num_waypoints=W, self_collision=True, return_detail=True),
        "(e) get_path_clearance, off": lambda: robot.get_path_clearance(paths, self_collision=False),
        "(f) get_path_clearance, on": lambda: robot.get_path_clearance(paths, self_collision=True),
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
    model = robot.self_collision_model()
    out = {"envs": B, "spheres": len(robot.collision_spheres()[1]), "extra_spheres": model[2], "pairs": len(robot.self_collision_pairs()), "waypoints": W,
           "calls_per_window": a.calls, "rounds": a.rounds, "variants": {}}
    for k in variants:
        t = sorted(times[k])
        out["variants"][k] = {"ms_per_call_median": round(t[len(t) // 2], 3), "ms_per_call_min": round(t[0], 3), "ms_per_call_max": round(t[-1], 3),
                              **({"plans": stats[k]} if k in stats else {})}
        print(f"{k:44s} median {t[len(t) // 2]:9.3f} ms   min {t[0]:9.3f} ms   max {t[-1]:9.3f} ms   {stats.get(k, '')}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
