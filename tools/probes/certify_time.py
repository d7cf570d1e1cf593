"""Developer probe: what certifying a path costs in one certify_path call (mir_certify_path), with and without `bracket`, beside -- measured
in the same run -- one get_path_clearance of the same paths: both evaluate clear(q) on the same sphere model, the first where the
Lipschitz bound asks for it, the second where the edge rule's resolution does.  Device events around queued calls, for the Franka of the
pick scene with a fixed box post between start and goal (the scene of plan_time.py).  4096 envs and 100 waypoints of the detour by
default, the entity's default sphere model.  The paths are those robot.plan_path returns for the envs.

    python tools/probes/certify_time.py [--envs 4096] [--waypoints 100] [--calls 5] [--rounds 5]

  (a) certify_path at margin 0      (b) certify_path with bracket=True      (c) get_path_clearance at resolution 0.05
Starts and goals are jittered per env.  Every variant is warmed up, then timed in `rounds` interleaved windows of `calls` back-to-back
calls between two events; the median, the minimum and the maximum over the rounds are printed, with the outcome of the calls.  The times
include the Python wrapper and the allocation of the outputs, as a caller pays them."""
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
GOAL = (0.9, -0.35, 0.05, -2.1, 0.0, 1.9, 0.7, 0.04, 0.04)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--waypoints", type=int, default=100)
    ap.add_argument("--margin", type=float, default=0.01)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
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
    goal = torch.as_tensor(np.array(GOAL, np.float32) + jit[1], device=sc.device)
    off = dict(self_collision=False)
    plan = robot.plan_path(goal, num_waypoints=a.waypoints, margin=a.margin, return_detail=True, **off)
    path = plan["path"]
    variants = {
        "(a) certify_path, margin 0": lambda: robot.certify_path(path, return_detail=True),
        "(b) certify_path, bracket": lambda: robot.certify_path(path, bracket=True, return_detail=True),
        "(c) get_path_clearance, resolution 0.05": lambda: robot.get_path_clearance(path, **off),
    }
    stats = {}
    for name, fn in variants.items():
        r = fn()
        torch.cuda.synchronize()
        if isinstance(r, dict):
            st, code = r["stats"].float(), r["status"].cpu().numpy()
            stats[name] = {"statuses": {S.CERT_STATUS[int(s)]: int((code == s).sum()) for s in np.unique(code)},
                           **{n: [float(st[:, i].median()), float(st[:, i].max())] for i, n in enumerate(("evaluations", "leaves", "deepest", "finished"))},
                           "lower_min": float(r["lower"].min()), "upper_min": float(r["upper"].min())}
        else:
            stats[name] = {"clearance_min": float(r.min())}
    times = {name: [] for name in variants}
    for _ in range(a.rounds):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.calls)
    out = {"envs": B, "spheres": len(robot.collision_spheres()[1]), "waypoints": int(path.shape[0]), "plans_ok": int(plan["valid"].sum()),
           "calls_per_window": a.calls, "rounds": a.rounds, "variants": {}}
    for name in variants:
        t = sorted(times[name])
        out["variants"][name] = {"ms_per_call_median": round(t[len(t) // 2], 3), "ms_per_call_min": round(t[0], 3), "ms_per_call_max": round(t[-1], 3),
                                 "outcome": stats[name]}
        print(f"{name:42s} median {t[len(t) // 2]:9.3f} ms   min {t[0]:9.3f} ms   max {t[-1]:9.3f} ms   {stats[name]}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
