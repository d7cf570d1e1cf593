"""Developer probe: time of pose-to-plan per call, with device events around queued calls, for the Franka of the pick scene with a fixed
box post in front of it (the scene, starts and goals of plan_time.py).  4096 envs by default.

    python tools/probes/goal_time.py [--envs 4096] [--calls 5] [--rounds 5] [--waypoints 100]

For two workloads -- "clear": the hand pose of a goal whose straight edge is clear; "post": the hand pose of a goal on the other side of
the post -- the same pose is planned to in four ways:
  (a) inverse_kinematics + plan_path, two calls       (b) plan_path_to_pose with max_samples=1, max_goals=1: the same, one launch
  (c) plan_path_to_pose with the defaults (16 samples, 4 goals)
  (d) plan_path_to_goals with the one goal configuration the pose was taken from, beside (e) plan_path to it: the same loop
and, on "post", (f) / (g) plan_path_to_goals with two / eight goal configurations: the forest.
Starts and goals are jittered per env.  Every variant is warmed up, then timed in `rounds` interleaved windows of `calls` back-to-back
calls between two events, all variants of both workloads in the same run; the median and the minimum over the rounds are printed with
the share of rows with a plan, iterations and nodes, and for (b), (c) the median and slowest goal_stats (samples tried, converged,
rejected, IK iterations) and goals kept.  The times include the Python wrapper and the allocation of the outputs, as a caller pays them."""
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
    jit = np.zeros((10, B, 9), np.float32)
    jit[:, :, :7] = rng.uniform(-0.04, 0.04, (10, B, 7))
    q = sc.get_state()[0].clone()
    q[:, robot._qcols] = torch.as_tensor(np.array(START, np.float32) + jit[0], device=sc.device)
    sc.set_state(qpos=q, qvel=torch.zeros((B, sc.nv), device=sc.device))
    across = torch.as_tensor(np.array(ACROSS, np.float32) + jit[1], device=sc.device)
    near = torch.as_tensor(np.array(NEAR, np.float32) + jit[2], device=sc.device)
    W = a.waypoints
    kw = dict(num_waypoints=W, return_detail=True)
    hand = robot.get_link("hand")
    q_start = sc.get_state()[0].clone()

    def hand_pose(cfg):   # the hand's pose at the configurations cfg, by the scene's own forward kinematics; the state is put back
        q2 = q_start.clone()
        q2[:, robot._qcols] = cfg
        sc.set_state(qpos=q2, qvel=torch.zeros((B, sc.nv), device=sc.device))
        pose = hand.get_pos().clone(), hand.get_quat().clone()
        sc.set_state(qpos=q_start, qvel=torch.zeros((B, sc.nv), device=sc.device))
        return pose

    def two_calls(pos, quat):
        q_goal = robot.inverse_kinematics(link=hand, pos=pos, quat=quat)
        q_goal[:, 7:] = q_start[:, robot._qcols][:, 7:]
        return robot.plan_path(q_goal, **kw)

    variants = {}
    for name, cfg in (("clear", near), ("post", across)):
        pos, quat = hand_pose(cfg)
        variants[f"{name} (a) inverse_kinematics + plan_path"] = lambda pos=pos, quat=quat: two_calls(pos, quat)
        variants[f"{name} (b) plan_path_to_pose, 1 sample, 1 goal"] = lambda pos=pos, quat=quat: robot.plan_path_to_pose(hand, pos, quat, max_goals=1, max_samples=1, **kw)
        variants[f"{name} (c) plan_path_to_pose, defaults"] = lambda pos=pos, quat=quat: robot.plan_path_to_pose(hand, pos, quat, **kw)
        variants[f"{name} (d) plan_path_to_goals, one goal"] = lambda cfg=cfg: robot.plan_path_to_goals(cfg[None], **kw)
        variants[f"{name} (e) plan_path to that goal"] = lambda cfg=cfg: robot.plan_path(cfg, **kw)
    # the forest itself: two and eight goal configurations across the post, jittered about one another
    eight = torch.stack([across] + [torch.as_tensor(np.array(ACROSS, np.float32) + jit[1] + jit[3 + k], device=sc.device) for k in range(7)])
    variants["post (f) plan_path_to_goals, two detours"] = lambda: robot.plan_path_to_goals(eight[:2], **kw)
    variants["post (g) plan_path_to_goals, eight detours"] = lambda: robot.plan_path_to_goals(eight, **kw)
    stats = {}
    for k, fn in variants.items():
        r = fn()
        torch.cuda.synchronize()
        if isinstance(r, dict):
            st = r["stats"].float()
            stats[k] = {"valid": float(r["valid"].float().mean()), "n_poly_mean": float(r["n_poly"].float().mean()),
                        **{n: [float(st[:, i].median()), float(st[:, i].mean()), float(st[:, i].max())]
                           for i, n in enumerate(("iterations", "nodes_a", "nodes_b", "checked"))}}
            if "goal_stats" in r:
                gs = r["goal_stats"].float()
                stats[k]["goal_stats_median"], stats[k]["goal_stats_max"] = gs.median(0).values.tolist(), gs.max(0).values.tolist()
                stats[k]["goals_kept_mean"] = float(r["n_goals"].float().mean())
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
        print(f"{k:50s} median {t[len(t) // 2]:9.3f} ms   min {t[0]:9.3f} ms   {stats.get(k, '')}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
