"""Developer probe: time of EntityView.retime_path (mir_retime_path) per call, with device events around queued calls, for the Franka of
the pick scene on the detour paths of tools/probes/plan_time.py (start and goal on either side of a box post).  4096 envs by default.

    python tools/probes/retime_time.py [--envs 4096] [--calls 5] [--rounds 5] [--waypoints 100]

  (a) MirScene.retime_path, no samples: the two passes alone       (b) the same with T samples and velocities
  (c) EntityView.retime_path with num_samples given: one launch    (d) the same with torque_limits=True: three inverse_dynamics calls on
  envs x waypoints rows in front of the launch                      (e) num_samples=None: two launches and one host read
  (f) get_path_clearance of the same waypoints, the nearest existing call per path
Every variant is warmed up, then timed in `rounds` interleaved windows of `calls` back-to-back calls between two events; the median and
the minimum over the rounds are printed with the durations of the motions.  The times include the Python wrapper and the allocation of
the outputs, as a caller pays them."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--waypoints", type=int, default=100)
    ap.add_argument("--vmax", type=float, default=2.0)
    ap.add_argument("--amax", type=float, default=5.0)
    a = ap.parse_args()
    B, W = a.envs, a.waypoints
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
    paths = robot.plan_path(torch.as_tensor(np.array(ACROSS, np.float32) + jit[1], device=sc.device), num_waypoints=W)
    rows = paths.permute(1, 0, 2).contiguous()
    dt = float(sb.opt["dt"])
    first = robot.retime_path(paths, a.vmax, a.amax, torque_limits=True, return_detail=True)
    T = int(first["n_samples"].max())
    lim = dict(vmax=[a.vmax] * 9, amax=[a.amax] * 9, dt=dt)
    variants = {
        "(a) scene.retime_path, no samples": lambda: sc.retime_path(rows, **lim),
        "(b) the same, T samples and velocities": lambda: sc.retime_path(rows, num_samples=T, velocity=True, **lim),
        "(c) robot.retime_path, num_samples=T": lambda: robot.retime_path(paths, a.vmax, a.amax, num_samples=T),
        "(d) the same, torque_limits=True": lambda: robot.retime_path(paths, a.vmax, a.amax, num_samples=T, torque_limits=True),
        "(e) robot.retime_path, num_samples=None": lambda: robot.retime_path(paths, a.vmax, a.amax),
        "(f) get_path_clearance of the waypoints": lambda: robot.get_path_clearance(paths),
    }
    for fn in variants.values():
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
            times[k].append(e0.elapsed_time(e1) / a.calls)
    free = robot.retime_path(paths, a.vmax, a.amax, num_samples=T, return_detail=True)
    d0, d1 = free["duration"], first["duration"]
    out = {"envs": B, "waypoints": W, "samples": T, "dt": dt, "vmax": a.vmax, "amax": a.amax, "calls_per_window": a.calls, "rounds": a.rounds,
           "timed_rows": float(first["valid"].float().mean()), "duration_s_median": round(float(d0.median()), 4),
           "duration_s_median_with_torque_rows": round(float(d1.median()), 4), "variants": {}}
    for k in variants:
        t = sorted(times[k])
        out["variants"][k] = {"ms_per_call_median": round(t[len(t) // 2], 3), "ms_per_call_min": round(t[0], 3)}
        print(f"{k:42s} median {t[len(t) // 2]:9.3f} ms   min {t[0]:9.3f} ms")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
