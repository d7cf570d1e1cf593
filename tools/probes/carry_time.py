"""Developer probe: what planning and checking with a carried object costs, with device events around queued calls, for the Franka of
the pick scene with a fixed box post in front of it (the scene of plan_time.py and self_time.py) and the cube held between the finger
pads.  4096 envs by default, the entity's default models; arm against arm is off, so "with the cube" adds the cube's spheres to the
scene test and the cube-against-arm pairs of attached_links_default().

    python tools/probes/carry_time.py [--envs 4096] [--calls 5] [--rounds 5] [--waypoints 100]

  (a) plan_path, detour round the post, the cube ignored (mir_plan_path)        (b) the same, the cube attached (mir_plan_path_carry)
  (c) get_path_clearance of (a)'s 100 waypoints, ignored (mir_path_clearance)   (d) the same, attached (mir_path_clearance_carry)
  (e) plan_path, direct edge to a goal in the open, ignored                      (f) the same, attached
Starts and goals are jittered per env; the grasp is taken by the kernel from the start rows.  Every variant is warmed up, then timed in
`rounds` interleaved windows of `calls` back-to-back calls between two events; the median, the minimum and the maximum over the rounds
are printed, with the statistics of the plans.  The times include the Python wrapper and the allocation of the outputs, as a caller
pays them."""
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
OPEN = (-1.4, -0.2, 0.1, -1.9, 0.1, 1.8, 0.6, 0.04, 0.04)
GRASP_Z = 0.105   # the cube's centre on the hand's axis: between the finger pads


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
    robot, cube = EntityView(sc, sb, "link0", models.FRANKA_JOINTS), EntityView(sc, sb, "cube", ())
    rng = np.random.default_rng(0)
    jit = np.zeros((3, B, 9), np.float32)
    jit[:, :, :7] = rng.uniform(-0.04, 0.04, (3, B, 7))
    q = sc.get_state()[0].clone()
    q[:, robot._qcols] = torch.as_tensor(np.array(START, np.float32) + jit[0], device=sc.device)
    sc.set_state(qpos=q, qvel=torch.zeros((B, sc.nv), device=sc.device))
    # the cube into the hand: the hand's pose at the start rows, GRASP_Z along its axis, the hand's orientation
    hand = robot.links_kinematics([robot.link_idx.index(sb.body_index("hand"))], vel=False)
    hp, hq = hand["pos"][:, 0], hand["quat"][:, 0]
    u, w = hq[:, 1:], hq[:, :1]
    v = torch.tensor([0.0, 0.0, GRASP_Z], device=sc.device).expand(B, 3)
    t = 2.0 * torch.cross(u, v, dim=1)
    qa = sum({0: 0, 1: 1, 2: 1, 3: 7}[b["jtype"]] for b in sb.bodies[1:sb.body_index("cube")])   # (qpos follows the body order)
    q[:, qa:qa + 3] = hp + v + w * t + torch.cross(u, t, dim=1)
    q[:, qa + 3:qa + 7] = hq
    sc.set_state(qpos=q, qvel=torch.zeros((B, sc.nv), device=sc.device))
    across = torch.as_tensor(np.array(ACROSS, np.float32) + jit[1], device=sc.device)
    in_open = torch.as_tensor(np.array(OPEN, np.float32) + jit[2], device=sc.device)
    W = a.waypoints
    off, on = dict(ignore_entities=[cube], self_collision=False), dict(attached_entity=cube, ee_link_name="hand", self_collision=False)
    paths = robot.plan_path(across, num_waypoints=W, **off)
    variants = {
        "(a) plan_path, detour, cube ignored": lambda: robot.plan_path(across, num_waypoints=W, return_detail=True, **off),
        "(b) plan_path, detour, cube attached": lambda: robot.plan_path(across, num_waypoints=W, return_detail=True, **on),
        "(c) get_path_clearance, cube ignored": lambda: robot.get_path_clearance(paths, **off),
        "(d) get_path_clearance, cube attached": lambda: robot.get_path_clearance(paths, **on),
        "(e) plan_path, direct edge, cube ignored": lambda: robot.plan_path(in_open, num_waypoints=W, return_detail=True, **off),
        "(f) plan_path, direct edge, cube attached": lambda: robot.plan_path(in_open, num_waypoints=W, return_detail=True, **on),
    }
    stats = {}
    for k, fn in variants.items():
        r = fn()
        torch.cuda.synchronize()
        if isinstance(r, dict):
            st = r["stats"].float()
            stats[k] = {"valid": float(r["valid"].float().mean()), "n_poly_mean": float(r["n_poly"].float().mean()),
                        **{n: [float(st[:, i].median()), float(st[:, i].mean()), float(st[:, i].max())]
                           for i, n in enumerate(("iterations", "nodes_a", "nodes_b", "checked"))}}
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
    model = robot.carried_model(cube, "hand", self_collision=False)
    out = {"envs": B, "spheres": len(robot.collision_spheres()[1]), "carried_spheres": len(cube.collision_spheres()[1]), "extra_spheres": model[2],
           "links_against_the_cube": bin(int(model[3][model[4]])).count("1"), "waypoints": W, "calls_per_window": a.calls, "rounds": a.rounds, "variants": {}}
    for k in variants:
        t = sorted(times[k])
        out["variants"][k] = {"ms_per_call_median": round(t[len(t) // 2], 3), "ms_per_call_min": round(t[0], 3), "ms_per_call_max": round(t[-1], 3),
                              **({"plans": stats[k]} if k in stats else {})}
        print(f"{k:44s} median {t[len(t) // 2]:9.3f} ms   min {t[0]:9.3f} ms   max {t[-1]:9.3f} ms   {stats.get(k, '')}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
