"""Plan, time, then move: inverse kinematics to a hover pose above the cube, robot.plan_path to that goal, robot.retime_path to turn the
waypoints into position targets every control step within velocity, acceleration and torque limits, and the targets as PD targets.

    python examples/franka/plan_retime_follow.py [--num-envs 64] [--waypoints 60] [--vmax 1.5] [--amax 4.0]

Every env plans in one launch (include/mirigid.h: mir_plan_path) and is timed in one launch (mir_retime_path: the fastest traversal of
the polyline from rest to rest that keeps the limits, the torque limits being the dofs' force range).  The duration of every env's motion
is printed, and the tracking error DURING the motion beside that of examples/franka/plan_and_follow.py's way of following the same
path: one waypoint per control step, whatever the joints can do.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "gym-genesis_amd"))
import torch  # noqa: E402

from gym_genesis.env import GenesisEnv  # noqa: E402


def follow(task, robot, targets):
    """the targets (T, B, n) as PD targets, one per step -> the largest joint error of each env against the target of the step before
    (what the arm was asked to reach by now), over the motion"""
    worst = torch.zeros(targets.shape[1], device=targets.device)
    for w in range(targets.shape[0]):
        if w > 0:
            worst = torch.maximum(worst, (robot.get_qpos() - targets[w - 1]).abs().max(1).values)
        robot.control_dofs_position(targets[w])
        task.scene.step()
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=64)
    ap.add_argument("--waypoints", type=int, default=60)
    ap.add_argument("--vmax", type=float, default=1.5)
    ap.add_argument("--amax", type=float, default=4.0)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    errs = {}
    for mode in ("retimed", "one waypoint per step"):
        env = GenesisEnv(task="cube_pick", robot="franka", num_envs=args.num_envs, enable_pixels=False)
        obs, _ = env.reset(seed=args.seed)
        task = env._env
        robot, cube = env.get_robot(), task.cube
        B, device = args.num_envs, obs["agent_pos"].device
        down = torch.tensor([0, 1, 0, 0], dtype=torch.float32, device=device).expand(B, -1)
        hover = obs["environment_state"][:, :3] + torch.tensor([0.0, 0.0, 0.115], device=device)
        q_goal = robot.inverse_kinematics(link=robot.get_link("hand"), pos=hover, quat=down)
        q_goal[:, 7:] = 0.04   # fingers open
        path, valid = robot.plan_path(q_goal, num_waypoints=args.waypoints, margin=0.005, ignore_entities=[cube], return_valid_mask=True)
        if mode == "retimed":
            timed = robot.retime_path(path, args.vmax, args.amax, torque_limits=True, return_detail=True)
            targets, d = timed["samples"], timed["duration"]
            print(f"plans: {int(valid.sum())} of {B} envs; timed: {int(timed['valid'].sum())} of {B}; duration per env {float(d.min()):.3f} .. "
                  f"{float(d.max()):.3f} s (median {float(d.median()):.3f} s), {targets.shape[0]} targets at {task.scene.dt} s")
            print("duration per env [s]: " + " ".join(f"{float(v):.2f}" for v in d))
            speed = (targets[1:] - targets[:-1]).abs().amax((0, 1)) / task.scene.dt
            print("largest finite-difference joint speed of the targets [rad/s]: " + " ".join(f"{float(v):.3f}" for v in speed[:7]))
        else:
            targets = path
        errs[mode] = follow(task, robot, targets)
        for _ in range(40):   # let the PD controller settle on the last target
            task.scene.step()
        end = (robot.get_qpos() - path[-1]).abs().max(1).values
        print(f"[{mode}] tracking error during the motion: median {float(errs[mode].median()):.4f}, worst {float(errs[mode].max()):.4f} rad; "
              f"after settling: median {float(end.median()):.4f} rad")
    return float(errs["retimed"].median()), float(errs["one waypoint per step"].median())


if __name__ == "__main__":
    main()
