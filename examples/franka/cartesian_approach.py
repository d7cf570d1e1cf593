"""Approach, grasp and lift with the hand on straight lines: inverse kinematics to a hover pose above the cube and robot.plan_path there,
robot.plan_cartesian_path straight down onto the cube, the fingers close, robot.plan_cartesian_path straight up with the cube attached,
robot.retime_path on every leg, and the timed targets as PD targets.

    python examples/franka/cartesian_approach.py [--num-envs 64] [--hover 0.10] [--vmax 1.0] [--amax 3.0]

Every leg of every env is one launch (include/mirigid.h: mir_plan_path, mir_cartesian_path, mir_retime_path).  Printed: the share of
each line that was achieved, the duration of every leg, and the hand's largest lateral deviation from the vertical during the descent
-- of the planned motion (the timed targets played back kinematically, robot.get_links_pos at each) and of the motion the PD controller
made of it.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "gym-genesis_amd"))
import torch  # noqa: E402

from gym_genesis.env import GenesisEnv  # noqa: E402


def hand_xy(robot, hand_local):
    return robot.get_links_pos([hand_local])[:, 0, :2]


def planned_deviation(mir, robot, hand_local, targets):
    """the targets (T, B, n) played back kinematically: the hand's largest horizontal distance from where it started, over the envs"""
    state = [x.clone() for x in mir.get_state()]
    cols = torch.as_tensor(robot._qcols, dtype=torch.long, device=mir.device)
    worst, xy0 = 0.0, None
    for w in range(targets.shape[0]):
        q = state[0].clone()
        q[:, cols] = targets[w]
        mir.set_state(qpos=q)
        xy = hand_xy(robot, hand_local)
        xy0 = xy if xy0 is None else xy0
        worst = max(worst, float((xy - xy0).norm(dim=1).max()))
    mir.set_state(*state)
    return worst


def follow(task, robot, targets, hand_local=None):
    """the targets as PD targets, one per step -> the hand's largest horizontal distance from where it started (with hand_local)"""
    worst, xy0 = 0.0, None if hand_local is None else hand_xy(robot, hand_local)
    for w in range(targets.shape[0]):
        robot.control_dofs_position(targets[w])
        task.scene.step()
        if hand_local is not None:
            worst = max(worst, float((hand_xy(robot, hand_local) - xy0).norm(dim=1).max()))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=64)
    ap.add_argument("--hover", type=float, default=0.10, help="height of the hover pose above the grasp pose [m]")
    ap.add_argument("--vmax", type=float, default=1.0)
    ap.add_argument("--amax", type=float, default=3.0)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    env = GenesisEnv(task="cube_pick", robot="franka", num_envs=args.num_envs, enable_pixels=False)
    obs, _ = env.reset(seed=args.seed)
    task = env._env
    robot, cube, mir = env.get_robot(), task.cube, task._mir
    B, device = args.num_envs, obs["agent_pos"].device
    hand = robot.get_link("hand")
    hand_local = robot.link_idx.index(hand.idx)
    down = torch.tensor([0, 1, 0, 0], dtype=torch.float32, device=device).expand(B, -1)
    grasp = obs["environment_state"][:, :3] + torch.tensor([0.0, 0.0, 0.115], device=device)
    hover = grasp + torch.tensor([0.0, 0.0, args.hover], device=device)
    durations, fractions = {}, {}

    def timed(path, leg):
        t = robot.retime_path(path, args.vmax, args.amax, return_detail=True)
        durations[leg] = t["duration"]
        return t["samples"]

    # 1. to the hover pose: any collision-free joint path will do
    q_hover = robot.inverse_kinematics(link=hand, pos=hover, quat=down)
    q_hover[:, 7:] = 0.04   # fingers open
    path, valid = robot.plan_path(q_hover, num_waypoints=40, margin=0.005, ignore_entities=[cube], return_valid_mask=True)
    follow(task, robot, timed(path, "to hover"))
    for _ in range(40):   # let the PD controller settle on the hover pose
        task.scene.step()
    # 2. straight down onto the cube: the hand itself follows the vertical
    below = hand.get_pos().clone()   # (from where the hand is now, so that the line is the vertical through it)
    below[:, 2] = grasp[:, 2]
    det = robot.plan_cartesian_path(hand, below, hand.get_quat(), ignore_entities=[cube], return_detail=True)
    fractions["descent"] = [float(f) for f in det["fraction"]]
    n_max = int(det["n_points"].max())
    step = float((det["points"][:, 1:n_max] - det["points"][:, :n_max - 1]).abs().max()) if n_max > 1 else 0.0
    targets = timed(det["path"], "descent")
    planned = planned_deviation(mir, robot, hand_local, targets)
    followed = follow(task, robot, targets, hand_local)
    # 3. close the fingers on the cube
    closed = robot.get_qpos().clone()
    closed[:, :7] = targets[-1][:, :7]
    closed[:, 7:] = 0.0
    for _ in range(30):
        robot.control_dofs_position(closed)
        task.scene.step()
    # 4. straight up with the cube attached: its spheres are checked like the arm's.  The cube rests on the ground, which the sphere
    # that covers it would penetrate (the lift would start in collision), so for this move it is modelled by a sphere inside it.
    probes, links = cube.collision_spheres()
    probes = probes.copy()
    probes[:, 3] = 0.85 * 0.02   # (the cube's half edge is 0.02 m)
    cube.set_collision_spheres(probes, links)
    now = robot.get_qpos()
    up = hand.get_pos() + torch.tensor([0.0, 0.0, args.hover], device=device)
    lift = robot.plan_cartesian_path(hand, up, hand.get_quat(), attached_entity=cube, ee_link_name="hand", return_detail=True)
    fractions["lift"] = [float(f) for f in lift["fraction"]]
    targets = timed(lift["path"], "lift")
    targets[:, :, 7:] = 0.0   # (the fingers keep squeezing: the plan holds them where they are, on the cube)
    follow(task, robot, targets)
    height = float((task.cube.get_pos()[:, 2]).median()) if hasattr(task.cube, "get_pos") else float("nan")
    print(f"plans to the hover pose: {int(valid.sum())} of {B} envs")
    for leg, f in fractions.items():
        print(f"{leg}: fraction of the line achieved per env: min {min(f):.3f} median {sorted(f)[len(f) // 2]:.3f}; statuses "
              f"{sorted(set((det if leg == 'descent' else lift)['status'].tolist()))}")
    for leg, d in durations.items():
        print(f"{leg}: duration per env {float(d.min()):.3f} .. {float(d.max()):.3f} s (median {float(d.median()):.3f} s)")
    print(f"descent: the hand's largest lateral deviation from the vertical: planned {planned * 1e3:.3f} mm, followed {followed * 1e3:.3f} mm "
          f"(largest joint step between two samples {step:.4f} rad); joint travel {float((now - q_hover).abs().max()):.3f} rad; "
          f"cube height after the lift (median) {height:.3f} m")
    return dict(fractions=fractions, durations={k: [float(x) for x in v] for k, v in durations.items()}, planned_deviation=planned,
                followed_deviation=followed, largest_joint_step=step)


if __name__ == "__main__":
    main()
