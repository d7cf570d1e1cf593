"""Time the device-resident rollout that keeps every contact point (mir_rollout_exact) against its neighbours, 4096 envs, K = 16,
HIP events around whole calls after warm-up; the legs of a comparison alternate call by call in one process.

  random U(-1, 1) actions:  mir_rollout (switch off)  vs  rollout_exact (switch on)
  the scripted grasp (tests/golden/grasp_targets.json, 200 steps):  rollout_exact  vs  step_begin / step_end with exact contacts
                                                                    vs  the thinned mir_rollout

The host-closed leg is timed through MirScene.step_begin / step_end, not through GenesisEnv.step (bench.py's scripted-grasp leg times
that), so it leaves out the env wrapper's host work.  Prints one JSON line per comparison and the rollout_exact statistics.  python tools/rollout_exact_time.py [--envs 4096] [--reps 5]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-genesis_amd"))

from gym_genesis.backend import models  # noqa: E402
from gym_genesis.backend.lib import MirScene  # noqa: E402

K = 16


def scene(n, exact):
    sc = MirScene(models.franka_cube_pick_scene().build(), n)
    if exact:
        sc.set_exact_contacts(True)
    return sc


def reset(sc, pos):
    n = pos.shape[0]
    sc.reset(pos, np.tile(np.array([0, 0, 0, 1], np.float32), (n, 1)), np.tile(np.array(models.FRANKA_HOME, np.float32), (n, 1)))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    n = args.envs
    rng = np.random.default_rng(0)
    dev = torch.device("cuda")
    rows = torch.zeros((K, n, 22), device=dev)

    # random actions: the thinned rollout vs rollout_exact (no env above 16 points: nothing is handed off)
    off, on = scene(n, False), scene(n, True)
    pos = np.stack([rng.uniform(0.45, 0.8, n), rng.uniform(-0.25, 0.25, n), np.full(n, 0.02)], 1).astype(np.float32)
    reset(off, pos); reset(on, pos)
    acts = torch.as_tensor(rng.uniform(-1, 1, (K, n, 9)).astype(np.float32), device=dev)
    for _ in range(3):
        off.rollout(acts, rows); on.rollout_exact(acts, rows)
    t_off, t_on = [], []
    for _ in range(args.reps * 4):
        t_off.append(timed(lambda: off.rollout(acts, rows)))
        t_on.append(timed(lambda: on.rollout_exact(acts, rows)))
    print(json.dumps({"workload": "random", "envs": n, "K": K, "rollout_us": float(np.median(t_off)), "rollout_exact_us": float(np.median(t_on)),
                      "stats": on.rollout_exact_stats(reset=True)}))

    # the scripted grasp: 200 steps as calls of 16 (the last of 8), from the same reset each rep
    G_ = json.load(open(os.path.join(ROOT, "tests", "golden", "grasp_targets.json")))
    T = np.array(G_["targets"], np.float32)
    pos4 = np.array([[x, y, 0.02] for x, y in G_["cube_xy"]], np.float32)
    gp = np.tile(pos4, (n // 4, 1))
    gp[:, :2] += np.random.default_rng(5).uniform(-0.002, 0.002, (n, 2)).astype(np.float32)
    ga = torch.as_tensor(np.tile(np.repeat(T.transpose(1, 0, 2), G_["steps_per_stage"], axis=0), (1, n // 4, 1))[:200], device=dev)
    ex, host, thin = scene(n, True), scene(n, True), scene(n, False)
    bufs = (host.empty(host.agent_dim), host.empty(host.env_dim), host.empty(), host.empty(dtype=torch.uint8))
    calls = [(t, min(K, 200 - t)) for t in range(0, 200, K)]

    def run_exact():
        for t, k in calls:
            ex.rollout_exact(ga[t:t + k].contiguous(), rows[:k])

    def run_thin():
        for t, k in calls:
            thin.rollout(ga[t:t + k].contiguous(), rows[:k])

    def run_host():
        for t in range(200):
            host.step_begin(ga[t], *bufs)
            host.step_end()

    res = {"exact": [], "host": [], "thin": []}
    for rep in range(args.reps + 1):
        for name, sc, fn in (("exact", ex, run_exact), ("host", host, run_host), ("thin", thin, run_thin)):
            reset(sc, gp)
            torch.cuda.synchronize()
            us = timed(fn)
            if rep > 0:
                res[name].append(us)
    med = {k: float(np.median(v)) for k, v in res.items()}
    print(json.dumps({"workload": "scripted_grasp", "envs": n, "steps": 200, "K": K,
                      **{f"{k}_us": v for k, v in med.items()},
                      **{f"{k}_Menv_steps_per_s": 200 * n / v for k, v in med.items()},
                      "stats": ex.rollout_exact_stats(reset=True)}))


if __name__ == "__main__":
    main()
