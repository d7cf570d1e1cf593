"""Developer probe: time of MirScene.link_accelerations (mir_link_accelerations) per call, with device events, next to
mir_link_kinematics for the same links and rows and to mir_forward (where the default qacc comes from).  Franka pick scene, 4096 envs by
default.

    python tools/probes/acc_time.py [--envs 4096] [--calls 2000] [--rounds 5]

Every variant is warmed up, then timed in `rounds` interleaved windows of `calls` back-to-back calls between two events; median and
minimum over the rounds are printed, with the bytes a call writes."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    B = a.envs
    sb = models.franka_cube_pick_scene()
    sc = MirScene(sb.build(), B)
    rng = np.random.default_rng(0)
    pos = np.stack([rng.uniform(0.45, 0.8, B), rng.uniform(-0.25, 0.25, B), np.full(B, 0.02)], 1).astype(np.float32)
    sc.reset(pos, np.tile(np.array([1, 0, 0, 0], np.float32), (B, 1)), np.tile(np.array(models.FRANKA_HOME, np.float32), (B, 1)))
    sc.step(5)
    hand, every = sb.body_index("hand"), list(range(1, sc.nbody))
    qacc = sc.forward()[3].clone()
    L = len(every)
    variants = {
        "hand: acc + bias_acc + imu (caller's qacc)": (lambda: sc.link_accelerations([hand], qacc=qacc, bias_acc=True, imu=True), B * 18 * 4),
        "hand: link_kinematics vel": (lambda: sc.link_kinematics([hand], pos=False, quat=False, jac=False), B * 6 * 4),
        "all links: acc (caller's qacc)": (lambda: sc.link_accelerations(every, qacc=qacc), B * L * 6 * 4),
        "all links: acc + bias_acc + imu (caller's qacc)": (lambda: sc.link_accelerations(every, qacc=qacc, bias_acc=True, imu=True), B * L * 18 * 4),
        "all links: link_kinematics vel": (lambda: sc.link_kinematics(every, pos=False, quat=False, jac=False), B * L * 6 * 4),
        "all links: link_kinematics pos + quat + vel": (lambda: sc.link_kinematics(every, jac=False), B * L * 13 * 4),
        "hand: imu (qacc=None: mir_forward first)": (lambda: sc.link_accelerations([hand], acc=False, imu=True), B * 6 * 4),
        "mir_forward alone": (sc.forward, B * (sc.nv * sc.nv + 3 * sc.nv) * 4),
    }
    for fn, _ in variants.values():
        for _ in range(50):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, (fn, _) in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / a.calls)
    floor = sc.null_roundtrip_us(2000)
    out = {"envs": B, "calls_per_window": a.calls, "rounds": a.rounds, "null_roundtrip_us": round(floor, 3), "variants": {}}
    for k, (_, nbytes) in variants.items():
        t = sorted(times[k])
        out["variants"][k] = {"us_per_call_median": round(t[len(t) // 2], 3), "us_per_call_min": round(t[0], 3), "bytes_written": nbytes}
        print(f"{k:52s} median {t[len(t) // 2]:8.2f} us   min {t[0]:8.2f} us   {nbytes / 1e6:8.3f} MB written")
    print(f"launch + host-visible completion floor (mir_debug_null_roundtrip): {floor:.2f} us")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
