"""Developer probe: time of MirScene.signed_distance (mir_signed_distance) per call, with device events, for the sphere model of the
Franka against the rest of the pick scene, next to MirScene.raycast at the same rows x items.  4096 envs by default.

    python tools/probes/distance_time.py [--envs 4096] [--calls 200] [--rounds 5]

  (a) the arm's collision_spheres() at the current state (pose cache), row_min only    (b) the same with every output
  (c) the same at candidate qpos rows (forward kinematics in the kernel), row_min only  (d) the same with every output
  (e) mir_raycast with as many rays as (a) has spheres from the hand, distances only    (f) the same with all four outputs
  (g) a robot.get_clearance(qpos=...) call as a user makes it (state read, scatter, launch)
Every variant is warmed up, then timed in `rounds` interleaved windows of `calls` back-to-back calls between two events; median and
minimum over the rounds are printed.  The times include the Python wrapper and the allocation of the outputs, as a caller pays them."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "gym-genesis_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gym_genesis.backend import models  # noqa: E402
from gym_genesis.backend.lib import MirScene  # noqa: E402
from gym_genesis.tasks.views import EntityView  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    B = a.envs
    sb = models.franka_cube_pick_scene()
    spec = sb.build()
    sc = MirScene(spec, B)
    rng = np.random.default_rng(0)
    pos = np.stack([rng.uniform(0.45, 0.8, B), rng.uniform(-0.25, 0.25, B), np.full(B, 0.02)], 1).astype(np.float32)
    sc.reset(pos, np.tile(np.array([1, 0, 0, 0], np.float32), (B, 1)), np.tile(np.array(models.FRANKA_HOME, np.float32), (B, 1)))
    sc.step(5)
    robot = EntityView(sc, sb, "link0", models.FRANKA_JOINTS)
    spheres, links = robot.collision_spheres()
    N = len(links)
    own = robot._own_geoms()
    probes = torch.as_tensor(spheres, device=sc.device)
    qfull = sc.get_state()[0].clone()
    qfull[:, robot._qcols] += 0.05 * torch.randn((B, len(robot._qcols)), device=sc.device, generator=torch.Generator(device=sc.device).manual_seed(0))
    qarm = qfull[:, robot._qcols].contiguous()
    dirs = rng.normal(size=(N, 3)).astype(np.float32)
    dirs_t = torch.as_tensor(dirs, device=sc.device)
    hand = sb.body_index("hand")
    every = dict(geom=True, closest=True, normal=True, row_min=True)
    variants = {
        f"(a) {N} spheres, pose cache, row_min": lambda: sc.signed_distance(probes, links=links, skip_geoms=own, row_min=True),
        f"(b) {N} spheres, pose cache, every output": lambda: sc.signed_distance(probes, links=links, skip_geoms=own, **every),
        f"(c) {N} spheres, qpos rows, row_min": lambda: sc.signed_distance(probes, links=links, skip_geoms=own, qpos=qfull, row_min=True),
        f"(d) {N} spheres, qpos rows, every output": lambda: sc.signed_distance(probes, links=links, skip_geoms=own, qpos=qfull, **every),
        f"(e) raycast, {N} rays from the hand, distances": lambda: sc.raycast(dirs_t, link=hand, skip_geoms=own, max_range=10.0, points=False),
        f"(f) raycast, {N} rays from the hand, four outputs": lambda: sc.raycast(dirs_t, link=hand, skip_geoms=own, max_range=10.0, geom=True, normal=True),
        "(g) robot.get_clearance(qpos=...)": lambda: robot.get_clearance(qpos=qarm),
    }
    for fn in variants.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / a.calls)
    out = {"envs": B, "spheres": N, "calls_per_window": a.calls, "rounds": a.rounds, "variants": {}}
    for k in variants:
        t = sorted(times[k])
        med = t[len(t) // 2]
        out["variants"][k] = {"us_per_call_median": round(med, 2), "us_per_call_min": round(t[0], 2)}
        print(f"{k:52s} median {med:9.2f} us   min {t[0]:9.2f} us")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
