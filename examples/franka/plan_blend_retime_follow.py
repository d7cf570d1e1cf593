"""Plan, blend, time, then move: robot.plan_path round a post, robot.blend_path to round the corners of the plan, retime_path to turn
the path into position targets every control step within velocity and acceleration limits, and the targets as PD targets.

    python examples/franka/plan_blend_retime_follow.py [--num-envs 64] [--waypoints 400] [--vmax 1.5] [--amax 4.0] [--deviation 0.05]

The scene is the pick scene with a fixed box post between start and goal, so the plan has corners.  Every env plans in one launch
(include/mirigid.h: mir_plan_path), is blended in one launch (mir_blend_path: each corner becomes a quadratic Bezier blend within
`deviation` of it, checked against the post like an edge of the planner, halved where it is blocked) and is timed in one launch
(mir_retime_path).  Both ways -- the planner's polyline as it is, and blended -- are resampled to the same number of waypoints, timed with
the same limits and followed; printed for each: the duration, the tracking error during the motion, and the largest second difference of
the targets over amax dt^2 (1 = the acceleration limit is kept sample by sample; a kink turned at a point exceeds it many times over).
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

START = (-0.9, -0.4, 0.0, -2.2, 0.0, 2.0, 0.8, 0.04, 0.04)
GOAL = (0.9, -0.35, 0.05, -2.1, 0.0, 1.9, 0.7, 0.04, 0.04)
POST = dict(size=(0.04, 0.04, 0.25), pos=(0.45, 0.0, 0.25))


def follow(sc, robot, targets):
    """the targets (T, B, n) as PD targets, one per step -> the largest joint error of each env against the target of the step before"""
    worst = torch.zeros(targets.shape[1], device=targets.device)
    for w in range(targets.shape[0]):
        if w > 0:
            worst = torch.maximum(worst, (robot.get_qpos() - targets[w - 1]).abs().max(1).values)
        robot.control_dofs_position(targets[w])
        sc.step()
    return worst


def retime(sc, path, vmax, amax, dt):
    """the path (W, B, n) as targets every dt -> (targets (T, B, n), duration (B,), status (B,)).  MirScene.retime_path itself, because the
    waypoints are dense: its max_path_speed is lifted from one waypoint per sample (the default of robot.retime_path) to no cap"""
    rows = path.permute(1, 0, 2).contiguous()
    T = int(sc.retime_path(rows, vmax, amax, dt, max_path_speed=1e5)["n_samples"].max())
    out = sc.retime_path(rows, vmax, amax, dt, num_samples=T, max_path_speed=1e5)
    return out["samples"].permute(1, 0, 2).contiguous(), out["duration"], out["status"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=64)
    ap.add_argument("--waypoints", type=int, default=400)
    ap.add_argument("--vmax", type=float, default=1.5)
    ap.add_argument("--amax", type=float, default=4.0)
    ap.add_argument("--deviation", type=float, default=0.05)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    B, W = args.num_envs, args.waypoints
    sb = models.franka_cube_pick_scene()
    sb.add_geom(0, S.GEOM_BOX, size=POST["size"], pos=POST["pos"], rgb=(0.5, 0.5, 0.55))
    sc = MirScene(sb.build(), B)
    robot = EntityView(sc, sb, "link0", models.FRANKA_JOINTS)
    dt = float(sc.spec.opt.dt)
    rng = np.random.default_rng(args.seed)
    jit = np.zeros((2, B, 9), np.float32)
    jit[:, :, :7] = rng.uniform(-0.04, 0.04, (2, B, 7))
    start = torch.as_tensor(np.array(START, np.float32) + jit[0], device=sc.device)
    goal = torch.as_tensor(np.array(GOAL, np.float32) + jit[1], device=sc.device)
    q0 = sc.get_state()[0].clone()
    q0[:, robot._qcols] = start
    off = dict(self_collision=False, margin=0.005)
    result = {}
    for mode in ("polyline", "blended"):
        sc.set_state(qpos=q0, qvel=torch.zeros((B, sc.nv), device=sc.device))
        robot.control_dofs_position(start)
        plan = robot.plan_path(goal, num_waypoints=W, return_detail=True, **off)
        path = plan["path"]
        if mode == "blended":
            K = max(int(plan["n_poly"].max()), 2)   # (the nodes any env uses: the capacity of the dense points follows K)
            smooth = robot.blend_path(plan["poly"][:, :K], plan["n_poly"], max_deviation=args.deviation, num_waypoints=W, return_detail=True, **off)
            path = smooth["path"]
            st = smooth["stats"]
            print(f"plans: {int(plan['valid'].sum())} of {B} envs; corners blended {int(st[:, 1].sum())}, left sharp {int(st[:, 2].sum())}, "
                  f"configurations checked per env {float(st[:, 3].float().mean()):.1f}; lowest clearance of the blended path "
                  f"{float(robot.get_path_clearance(path, self_collision=False).min()):.4f} m")
        targets, d, status = retime(sc, path, args.vmax, args.amax, dt)
        second = (targets[2:] - 2.0 * targets[1:-1] + targets[:-2]).abs().amax((0, 2)) / (args.amax * dt * dt)
        err = follow(sc, robot, targets)
        result[mode] = dict(duration=float(d.median()), tracking=float(err.median()), second=float(second.median()), second_worst=float(second.max()),
                            timed=int((status <= 1).sum()))   # (OK or NO_MOTION)
        print(f"[{mode}] timed {result[mode]['timed']} of {B}; duration median {result[mode]['duration']:.3f} s; tracking error during the motion "
              f"median {result[mode]['tracking']:.4f} rad; largest second difference of the targets over amax dt^2: median "
              f"{result[mode]['second']:.2f}, worst {result[mode]['second_worst']:.2f}")
    return result


if __name__ == "__main__":
    main()
