"""Plan to a pose: a hover pose above a cube that lies behind a post, as seen from where the arm starts -> robot.plan_path_to_pose ->
robot.retime_path -> the targets as PD targets.

    python examples/franka/plan_to_pose.py [--num-envs 8] [--waypoints 60] [--vmax 1.5] [--amax 4.0]

The pick scene with a fixed box post in front of the arm; the arm starts on one side of the post, the cube lies on the other.  Every env
solves the inverse kinematics of the hover pose from several seeds, keeps the solutions that are clear, takes the straight edge to the
nearest one that has one and otherwise plans round the post to whichever the trees meet through -- in ONE launch (include/mirigid.h:
mir_plan_path_pose); nothing is decided on the host between the pose and the plan.  Printed: the goals kept and the samples it took,
which rows needed the trees, the duration of the motion and, after following it, how far the hand is from the hover pose.  TOL is what
this script calls "arrived".
"""
import argparse
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

TOL = 0.02   # [m] the hand's distance from the hover pose after the motion has settled
START = (-0.9, -0.4, 0.0, -2.2, 0.0, 2.0, 0.8, 0.04, 0.04)
CUBE = (0.5, 0.3, 0.02)
DT = 0.01


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=8)
    ap.add_argument("--waypoints", type=int, default=60)
    ap.add_argument("--vmax", type=float, default=1.5)
    ap.add_argument("--amax", type=float, default=4.0)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    B = args.num_envs
    sb = models.franka_cube_pick_scene()
    sb.add_geom(0, S.GEOM_BOX, size=(0.04, 0.04, 0.25), pos=(0.45, 0.0, 0.25), rgb=(0.5, 0.5, 0.55))   # the post
    sc = MirScene(sb.build(), B)
    robot, cube = EntityView(sc, sb, "link0", models.FRANKA_JOINTS), EntityView(sc, sb, "cube", ())
    hand = robot.get_link("hand")
    rng = np.random.default_rng(args.seed)
    start = np.array(START, np.float32) + np.concatenate([rng.uniform(-0.04, 0.04, (B, 7)), np.zeros((B, 2))], 1).astype(np.float32)
    cube_xy = np.array(CUBE[:2], np.float32) + rng.uniform(-0.03, 0.03, (B, 2)).astype(np.float32)
    sc.reset(np.concatenate([cube_xy, np.full((B, 1), CUBE[2], np.float32)], 1), np.tile(np.array([0, 0, 0, 1], np.float32), (B, 1)), start)
    device = sc.device
    hover = torch.as_tensor(np.concatenate([cube_xy, np.full((B, 1), CUBE[2] + 0.115, np.float32)], 1), device=device)
    det = robot.plan_path_to_pose(hand, hover, (0.0, 1.0, 0.0, 0.0), max_goals=4, max_samples=16, num_waypoints=args.waypoints, margin=0.005,
                                  ignore_entities=[cube], seed=args.seed, return_detail=True)
    path, st = det["path"], det["goal_stats"]
    print(f"plans: {int(det['valid'].sum())} of {B} envs; goals kept per env {det['n_goals'].tolist()}, reached {det['goal_index'].tolist()}")
    print(f"samples tried {st[:, 0].tolist()}, converged {st[:, 1].tolist()}, rejected {st[:, 2].tolist()}; rows that needed the trees: "
          f"{int((det['stats'][:, 0] > 0).sum())} (iterations {det['stats'][:, 0].tolist()})")
    timed = robot.retime_path(path, args.vmax, args.amax, dt=DT, return_detail=True)
    targets, d = timed["samples"], timed["duration"]
    print(f"timed: {int(timed['valid'].sum())} of {B}; duration per env {float(d.min()):.3f} .. {float(d.max()):.3f} s, {targets.shape[0]} targets at {DT} s")
    bufs = (sc.empty(sc.agent_dim), sc.empty(sc.env_dim), sc.empty(), sc.empty(dtype=torch.uint8))
    for w in range(targets.shape[0] + 60):   # (60 more steps on the last target: the PD controller settles)
        sc.step_fused(targets[min(w, targets.shape[0] - 1)].contiguous(), *bufs)
    err = (hand.get_pos() - hover).norm(dim=1)
    joint = (robot.get_qpos() - path[-1]).abs().max(1).values
    print(f"hand to hover pose after settling: median {float(err.median()):.4f} m, worst {float(err.max()):.4f} m (TOL {TOL} m); joint error worst {float(joint.max()):.4f} rad")
    return det["valid"].cpu(), det["n_goals"].cpu(), err.cpu()


if __name__ == "__main__":
    main()
