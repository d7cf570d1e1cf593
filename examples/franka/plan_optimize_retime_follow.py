"""Plan, optimise, time, then move: robot.plan_path round a post, robot.optimize_path to make the plan shorter, smoother and further
from the post, retime_path to turn the path into position targets every control step, and the targets as PD targets.

    python examples/franka/plan_optimize_retime_follow.py [--num-envs 64] [--waypoints 64] [--vmax 1.5] [--amax 4.0] [--margin 0.005]

The scene and the loop are those of plan_blend_retime_follow.py -- the pick scene with a fixed box post between start and goal -- with a
third way beside its two: plan -> optimise -> retime -> follow.  Every env plans in one launch (include/mirigid.h: mir_plan_path), is
optimised in one launch (mir_optimize_path: covariant gradient descent on smoothness plus an obstacle cost of the sphere model, the
result swept with the planner's edge rule; a row whose result does not pass comes back as its plan) and is timed in one launch
(mir_retime_path).  All three ways use the same number of waypoints (at most 128: the optimiser's capacity) and the same limits.
Printed for each: the duration, the lowest get_path_clearance, the second-difference ratio of the waypoints (the largest second
difference over the largest first difference: 0 for a straight line at equal spacing) and the tracking error during the motion.  The
optimised path goes through certify_path once, and the row statuses are printed.
The gripper is held half open (0.02): a joint that sits ON its limit with the obstacle gradient pointing outward is refused at every
step length (the rule rejects a candidate that leaves the limits, it does not project), and an open gripper at 0.04 is such a joint.
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

START = (-0.9, -0.4, 0.0, -2.2, 0.0, 2.0, 0.8, 0.02, 0.02)
GOAL = (0.9, -0.35, 0.05, -2.1, 0.0, 1.9, 0.7, 0.02, 0.02)
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
    """the path (W, B, n) as targets every dt -> (targets (T, B, n), duration (B,), status (B,))"""
    rows = path.permute(1, 0, 2).contiguous()
    T = int(sc.retime_path(rows, vmax, amax, dt, max_path_speed=1e5)["n_samples"].max())
    out = sc.retime_path(rows, vmax, amax, dt, num_samples=T, max_path_speed=1e5)
    return out["samples"].permute(1, 0, 2).contiguous(), out["duration"], out["status"]


def smoothness(path):
    """S per env of a path (W, B, n): (W - 1) / 2 times the sum of the squared steps"""
    d = path[1:] - path[:-1]
    return 0.5 * (path.shape[0] - 1) * (d * d).sum((0, 2))


def second_ratio(path):
    """per env: the largest second difference of the waypoints over the largest first difference"""
    return (path[2:] - 2.0 * path[1:-1] + path[:-2]).abs().amax((0, 2)) / (path[1:] - path[:-1]).abs().amax((0, 2)).clamp_min(1e-30)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=64)
    ap.add_argument("--waypoints", type=int, default=64)
    ap.add_argument("--vmax", type=float, default=1.5)
    ap.add_argument("--amax", type=float, default=4.0)
    ap.add_argument("--margin", type=float, default=0.005)
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
    off = dict(self_collision=False, margin=args.margin)
    result = {}
    for mode in ("polyline", "blended", "optimised"):
        sc.set_state(qpos=q0, qvel=torch.zeros((B, sc.nv), device=sc.device))
        robot.control_dofs_position(start)
        plan = robot.plan_path(goal, num_waypoints=W, return_detail=True, **off)
        path = plan["path"]
        if mode == "blended":
            K = max(int(plan["n_poly"].max()), 2)
            path = robot.blend_path(plan["poly"][:, :K], plan["n_poly"], max_deviation=args.deviation, num_waypoints=W, **off)
        elif mode == "optimised":
            opt = robot.optimize_path(plan["path"], return_detail=True, **off)
            path = opt["path"]
            st = opt["stats"]
            certified = robot.certify_path(path, margin=0.0)
            names = [S.OPT_STATUS[int(v)] for v in opt["status"].cpu()]
            print(f"plans: {int(plan['valid'].sum())} of {B} envs; optimiser statuses {dict((n, names.count(n)) for n in sorted(set(names)))}; iterations "
                  f"per env {float(st[:, 0].float().mean()):.1f}, accepted {float(st[:, 1].float().mean()):.1f}, halvings {float(st[:, 2].float().mean()):.1f}; "
                  f"certify_path row statuses {[S.CERT_STATUS[int(v)] for v in certified.cpu()][:16]}")
            result["rows"] = dict(ok=(opt["valid"] & plan["valid"]).cpu().numpy(), status=opt["status"].cpu().numpy(), S_in=smoothness(plan["path"]).cpu().numpy(),
                                  S_out=smoothness(path).cpu().numpy(), certified=certified.cpu().numpy())
        clearance = robot.get_path_clearance(path, self_collision=False)
        targets, d, status = retime(sc, path, args.vmax, args.amax, dt)
        err = follow(sc, robot, targets)
        result[mode] = dict(duration=float(d.median()), clearance=float(clearance.min()), ratio=float(second_ratio(path).median()), S=float(smoothness(path).median()),
                            tracking=float(err.median()), timed=int((status <= 1).sum()))   # (OK or NO_MOTION)
        v = result[mode]
        print(f"[{mode}] timed {v['timed']} of {B}; duration median {v['duration']:.3f} s; lowest get_path_clearance {v['clearance']:.4f} m; "
              f"second-difference ratio median {v['ratio']:.3f}; S median {v['S']:.4f}; tracking error during the motion median {v['tracking']:.4f} rad")
    return result


if __name__ == "__main__":
    main()
