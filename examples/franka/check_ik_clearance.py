"""Vet the expert's IK goals before they are commanded: robot.in_collision(q_goal) on the joint positions that
robot.inverse_kinematics returns for the "hover" and "grasp" stages of the cube-pick expert (pick_cube_state.py), at the state of a
reset.  Prints the share of envs whose goal puts the arm's sphere model into the floor or the cube, and the lowest clearance.

    python examples/franka/check_ik_clearance.py [--num-envs 256]

The clearance is that of the goal configuration alone: nothing is said about the path to it, or about the arm touching itself
(signed distance and clearance).  The grasp goal is expected to be flagged: it closes the fingers around the cube.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "gym-genesis_amd"))
import torch  # noqa: E402

from gym_genesis.env import GenesisEnv  # noqa: E402

STAGE_DZ = {"hover": 0.115, "grasp": 0.03}  # hand target above the live cube position (the expert's constants)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=256)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    env = GenesisEnv(task="cube_pick", robot="franka", num_envs=args.num_envs, enable_pixels=False)
    obs, _ = env.reset(seed=args.seed)
    robot = env.get_robot()
    B, device = args.num_envs, obs["agent_pos"].device
    cube_pos = obs["environment_state"][:, :3]
    quat = torch.tensor([0, 1, 0, 0], dtype=torch.float32, device=device).expand(B, -1)
    out = {}
    for stage, dz in STAGE_DZ.items():
        q_goal = robot.inverse_kinematics(link=robot.get_link("hand"), pos=cube_pos + torch.tensor([0.0, 0.0, dz], device=device), quat=quat)
        flagged = robot.in_collision(q_goal)
        clearance = robot.get_clearance(qpos=q_goal)
        out[stage] = float(flagged.float().mean())
        print(f"{stage:6s}: {out[stage]:6.1%} of {B} envs flagged, lowest clearance {float(clearance.min()):+.4f} m, median {float(clearance.median()):+.4f} m")
    return out


if __name__ == "__main__":
    main()
