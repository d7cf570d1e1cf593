"""Developer probe: what a straight-line descent of the hand costs in one plan_cartesian_path call (mir_cartesian_path) and, measured in
the same run, the way it is done without it: one inverse_kinematics call per Cartesian sample, each seeded with the answer before,
then one get_path_clearance of the joint path.  Device events around queued calls, for the Franka of the pick scene with a fixed box
post in front of it (the scene of plan_time.py) and the cube held between the finger pads.  4096 envs by default, the entity's default
sphere model.

    python tools/probes/cartesian_time.py [--envs 4096] [--calls 5] [--rounds 5]

  (a) plan_cartesian_path, 8 samples (0.075 m down at max_step 0.01)      (b) 8 chained inverse_kinematics + get_path_clearance
  (c) plan_cartesian_path, 25 samples (0.245 m down)                      (d) 25 chained inverse_kinematics + get_path_clearance
  (e) as (c) with the self test on    (f) as (c) with the cube attached    (g) as (c) with ignore_collision
Starts are jittered per env; the orientation is held.  Every variant is warmed up, then timed in `rounds` interleaved windows of `calls`
back-to-back calls between two events; the median, the minimum and the maximum over the rounds are printed, with the outcome of the
calls.  The times include the Python wrapper and the allocation of the outputs, as a caller pays them."""
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
GRASP_Z = 0.105   # the cube's centre on the hand's axis: between the finger pads
STEP = 0.01


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    B = a.envs
    sb = models.franka_cube_pick_scene()
    sb.add_geom(0, S.GEOM_BOX, size=(0.04, 0.04, 0.25), pos=(0.45, 0.0, 0.25))
    sc = MirScene(sb.build(), B)
    robot, cube = EntityView(sc, sb, "link0", models.FRANKA_JOINTS), EntityView(sc, sb, "cube", ())
    rng = np.random.default_rng(0)
    jit = np.zeros((B, 9), np.float32)
    jit[:, :7] = rng.uniform(-0.04, 0.04, (B, 7))
    q = sc.get_state()[0].clone()
    q[:, robot._qcols] = torch.as_tensor(np.array(START, np.float32) + jit, device=sc.device)
    sc.set_state(qpos=q, qvel=torch.zeros((B, sc.nv), device=sc.device))
    hand = robot.get_link("hand")
    k = robot.links_kinematics([robot.link_idx.index(hand.idx)], vel=False)
    hp, hq = k["pos"][:, 0].contiguous(), k["quat"][:, 0].contiguous()
    # the cube into the hand: GRASP_Z along the hand's axis, the hand's orientation
    u, w = hq[:, 1:], hq[:, :1]
    v = torch.tensor([0.0, 0.0, GRASP_Z], device=sc.device).expand(B, 3)
    t = 2.0 * torch.cross(u, v, dim=1)
    qa = sum({0: 0, 1: 1, 2: 1, 3: 7}[b["jtype"]] for b in sb.bodies[1:sb.body_index("cube")])   # (qpos follows the body order)
    q[:, qa:qa + 3] = hp + v + w * t + torch.cross(u, t, dim=1)
    q[:, qa + 3:qa + 7] = hq
    sc.set_state(qpos=q, qvel=torch.zeros((B, sc.nv), device=sc.device))
    q0 = robot.get_qpos().clone()
    off = dict(ignore_entities=[cube], self_collision=False)

    def target(n):
        return hp + torch.tensor([0.0, 0.0, -(n - 0.5) * STEP], device=sc.device)

    def cart(n, **kw):
        return robot.plan_cartesian_path(hand, target(n), hq, max_step=STEP, max_points=32, return_detail=True, **{**off, **kw})

    def chained(n):
        """what the experts do today: n Cartesian points, an IK call each from the answer before, then the swept check"""
        goal, qs, prev = target(n), [q0], q0
        for i in range(1, n + 1):
            p = hp + (i / n) * (goal - hp)
            prev = robot.inverse_kinematics(hand, pos=p, quat=hq, init_qpos=prev)
            qs.append(prev)
        path = torch.stack(qs)
        return path, robot.get_path_clearance(path, **off)

    variants = {
        "(a) plan_cartesian_path, 8 samples": lambda: cart(8),
        "(b) 8 x inverse_kinematics + get_path_clearance": lambda: chained(8),
        "(c) plan_cartesian_path, 25 samples": lambda: cart(25),
        "(d) 25 x inverse_kinematics + get_path_clearance": lambda: chained(25),
        "(e) 25 samples, self test on": lambda: cart(25, self_collision=True),
        "(f) 25 samples, cube attached": lambda: cart(25, attached_entity=cube, ee_link_name="hand", ignore_entities=()),
        "(g) 25 samples, ignore_collision": lambda: cart(25, ignore_collision=True),
    }
    stats = {}
    for name, fn in variants.items():
        r = fn()
        torch.cuda.synchronize()
        if isinstance(r, dict):
            st = r["stats"].float()
            stats[name] = {"fraction_mean": float(r["fraction"].mean()), "statuses": sorted(set(r["status"].tolist())),
                           **{n: [float(st[:, i].median()), float(st[:, i].max())] for i, n in enumerate(("ik_iterations", "checked", "samples"))}}
        else:
            stats[name] = {"clearance_min": float(r[1].min()), "joint_step_max": float((r[0][1:] - r[0][:-1]).abs().max())}
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
    out = {"envs": B, "spheres": len(robot.collision_spheres()[1]), "calls_per_window": a.calls, "rounds": a.rounds, "variants": {}}
    for name in variants:
        t = sorted(times[name])
        out["variants"][name] = {"ms_per_call_median": round(t[len(t) // 2], 3), "ms_per_call_min": round(t[0], 3), "ms_per_call_max": round(t[-1], 3),
                                 "outcome": stats[name]}
        print(f"{name:52s} median {t[len(t) // 2]:9.3f} ms   min {t[0]:9.3f} ms   max {t[-1]:9.3f} ms   {stats[name]}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
