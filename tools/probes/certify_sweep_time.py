"""Developer probe: what certifying a path with the self test and with a carried cube costs in one certify_sweep call
(mir_certify_path_self / mir_certify_path_carry), beside -- measured in the same run -- get_path_clearance(self_collision=True /
attached_entity=...) of the same paths, which judges samples of them, and beside certify_path and get_path_clearance of the scene test
alone.  Device events around queued calls, for the Franka of the pick scene with a fixed box post between start and goal (the scene of
certify_time.py).  4096 envs and 100 waypoints of the detour by default, the entity's default sphere and self models; the cube rides in
the hand by a fixed grasp.  The paths are those robot.plan_path(self_collision=True) returns for the envs.

    python tools/probes/certify_sweep_time.py [--envs 4096] [--waypoints 100] [--calls 5] [--rounds 5]

  (a) certify_sweep, self test            (b) get_path_clearance, self test, resolution 0.05
  (c) certify_sweep, cube attached        (d) get_path_clearance, cube attached
  (e) certify_path (scene only)           (f) get_path_clearance (scene only)
Starts and goals are jittered per env.  Every variant is warmed up, then timed in `rounds` interleaved windows of `calls` back-to-back
calls between two events; the median, the minimum and the maximum over the rounds are printed, with the outcome of the calls and the
ratios (a) / (b), (c) / (d), (e) / (f), (b) / (f) and (a) / (f).  The times include the Python wrapper and the allocation of the
outputs, as a caller pays them."""
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
GRASP = (0.0, 0.0, 0.119, 1.0, 0.0, 0.0, 0.0)   # the cube between the finger pads, in the hand's frame


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
    cube = EntityView(sc, sb, "cube", ())
    rng = np.random.default_rng(0)
    jit = np.zeros((2, B, 9), np.float32)
    jit[:, :, :7] = rng.uniform(-0.04, 0.04, (2, B, 7))
    q = sc.get_state()[0].clone()
    q[:, robot._qcols] = torch.as_tensor(np.array(START, np.float32) + jit[0], device=sc.device)
    sc.set_state(qpos=q, qvel=torch.zeros((B, sc.nv), device=sc.device))
    goal = torch.as_tensor(np.array(GOAL, np.float32) + jit[1], device=sc.device)
    own = dict(self_collision=True, ignore_entities=[cube])
    att = dict(attached_entity=cube, ee_link_name="hand", grasp_pose=torch.tensor(GRASP, device=sc.device), self_collision=False)
    off = dict(self_collision=False, ignore_entities=[cube])
    plan = robot.plan_path(goal, num_waypoints=a.waypoints, margin=a.margin, self_margin=a.margin, return_detail=True, **own)
    path = plan["path"]
    variants = {
        "(a) certify_sweep, self test": lambda: robot.certify_sweep(path, return_detail=True, **own),
        "(b) get_path_clearance, self test": lambda: robot.get_path_clearance(path, return_detail=True, **own),
        "(c) certify_sweep, cube attached": lambda: robot.certify_sweep(path, return_detail=True, **att),
        "(d) get_path_clearance, cube attached": lambda: robot.get_path_clearance(path, return_detail=True, **att),
        "(e) certify_path, scene only": lambda: robot.certify_path(path, ignore_entities=[cube], return_detail=True),
        "(f) get_path_clearance, scene only": lambda: robot.get_path_clearance(path, return_detail=True, **off),
    }
    stats = {}
    for name, fn in variants.items():
        r = fn()
        torch.cuda.synchronize()
        if "stats" in r:
            st, code = r["stats"].float(), r["status"].cpu().numpy()
            stats[name] = {"statuses": {S.CERT_STATUS[int(s)]: int((code == s).sum()) for s in np.unique(code)},
                           **{n: [float(st[:, i].median()), float(st[:, i].max())] for i, n in enumerate(("evaluations", "leaves", "deepest", "finished"))},
                           "lower_min": float(r["lower"].min()), "upper_min": float(r["upper"].min())}
            if "self_lower" in r:
                stats[name].update(self_lower_min=float(r["self_lower"].min()), self_upper_min=float(r["self_upper"].min()))
        else:
            stats[name] = {"clearance_min": float(r["clearance"].min())}
            if "self_clearance" in r:
                stats[name]["self_clearance_min"] = float(r["self_clearance"].min())
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
    out = {"envs": B, "spheres": len(robot.collision_spheres()[1]), "self_spheres": len(robot.self_collision_model()[1]), "waypoints": int(path.shape[0]),
           "plans_ok": int(plan["valid"].sum()), "calls_per_window": a.calls, "rounds": a.rounds, "variants": {}}
    med = {}
    for name in variants:
        t = sorted(times[name])
        med[name[:3]] = t[len(t) // 2]
        out["variants"][name] = {"ms_per_call_median": round(t[len(t) // 2], 3), "ms_per_call_min": round(t[0], 3), "ms_per_call_max": round(t[-1], 3),
                                 "outcome": stats[name]}
        print(f"{name:40s} median {t[len(t) // 2]:9.3f} ms   min {t[0]:9.3f} ms   max {t[-1]:9.3f} ms   {stats[name]}")
    out["ratios"] = {f"{x} / {y}": round(med[x] / med[y], 2) for x, y in (("(a)", "(b)"), ("(c)", "(d)"), ("(e)", "(f)"), ("(b)", "(f)"), ("(a)", "(f)"), ("(c)", "(f)"))}
    print(out["ratios"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
