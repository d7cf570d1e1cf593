"""Plan before moving: inverse kinematics to a hover pose above the cube, robot.plan_path from the current joint positions to that goal,
then the waypoints as PD targets, one per control step, and the clearance of the path that was followed.

    python examples/franka/plan_and_follow.py [--num-envs 64] [--waypoints 60]

Every env plans in the same launch (RRT-Connect on the arm's sphere model, include/mirigid.h: mir_plan_path).  The cube is left out of
the obstacles while the hand reaches for it; the floor stays in.  A row without a plan keeps its start: its arm stays where it is.
The path's clearance is that of the sphere model against the scene; the arm touching itself is not checked.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "gym-genesis_amd"))
import torch  # noqa: E402

from gym_genesis.env import GenesisEnv  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=64)
    ap.add_argument("--waypoints", type=int, default=60)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    env = GenesisEnv(task="cube_pick", robot="franka", num_envs=args.num_envs, enable_pixels=False)
    obs, _ = env.reset(seed=args.seed)
    task = env._env
    robot, cube = env.get_robot(), task.cube
    B, device = args.num_envs, obs["agent_pos"].device
    cube_pos = obs["environment_state"][:, :3]
    down = torch.tensor([0, 1, 0, 0], dtype=torch.float32, device=device).expand(B, -1)
    hover = cube_pos + torch.tensor([0.0, 0.0, 0.115], device=device)
    q_goal = robot.inverse_kinematics(link=robot.get_link("hand"), pos=hover, quat=down)
    q_goal[:, 7:] = 0.04   # fingers open
    plan = robot.plan_path(q_goal, num_waypoints=args.waypoints, margin=0.005, ignore_entities=[cube], return_detail=True)
    path, valid = plan["path"], plan["valid"]
    print(f"plans: {int(valid.sum())} of {B} envs; polyline nodes {plan['n_poly'].min().item()} .. {plan['n_poly'].max().item()}, "
          f"iterations up to {plan['stats'][:, 0].max().item()}")
    clearance = robot.get_path_clearance(path, ignore_entities=[cube])
    print(f"clearance along the planned paths: lowest {float(clearance.min()):+.4f} m, median {float(clearance.median()):+.4f} m")
    for w in range(path.shape[0]):
        robot.control_dofs_position(path[w])
        task.scene.step()
    for _ in range(40):   # let the PD controller settle on the last waypoint
        task.scene.step()
    err = (robot.get_qpos() - path[-1]).abs().max(1).values
    print(f"joint error at the end of the path: median {float(err.median()):.4f}, worst {float(err.max()):.4f} rad")
    hand = robot.get_link("hand").get_pos()
    print(f"hand above the cube: {float((hand - hover)[valid].norm(dim=1).max()) if valid.any() else float('nan'):.4f} m at worst")
    return float(valid.float().mean())


if __name__ == "__main__":
    main()
