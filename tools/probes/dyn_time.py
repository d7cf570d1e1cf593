"""Developer probe: time of MirScene.dynamics (mir_dynamics) per call, with device events, next to mir_forward (the step kernel in
forward mode: the other way to M and qfrc_bias) and the launch floor of mir_debug_null_roundtrip.  Franka pick scene, 4096 envs by default.

    python tools/probes/dyn_time.py [--envs 4096] [--calls 1000] [--rounds 5]

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
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    B = a.envs
    sb = models.franka_cube_pick_scene()
    sc = MirScene(sb.build(), B)
    rng = np.random.default_rng(0)
    pos = np.stack([rng.uniform(0.45, 0.8, B), rng.uniform(-0.25, 0.25, B), np.full(B, 0.02)], 1).astype(np.float32)
    sc.reset(pos, np.tile(np.array([1, 0, 0, 0], np.float32), (B, 1)), np.tile(np.array(models.FRANKA_HOME, np.float32), (B, 1)))
    sc.step(5)
    nv = sc.nv
    qacc = torch.as_tensor(rng.uniform(-1, 1, (B, nv)).astype(np.float32), device=sc.device)
    variants = {
        "arm (9 dofs): M + bias": (lambda: sc.dynamics(dof0=0, n_dofs=9), B * (81 + 9) * 4),
        "all 15 dofs: M, bias, gravity, tau, ctrl_force": (lambda: sc.dynamics(qacc=qacc, gravity=True, tau=True, ctrl_force=True), B * (nv * nv + 4 * nv) * 4),
        "mir_forward (step kernel, mode 1)": (sc.forward, B * (nv * nv + 3 * nv) * 4),
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
        out["variants"][k] = {"us_per_call_median": round(t[len(t) // 2], 3), "us_per_call_min": round(t[0], 3), "bytes_written": nbytes,
                              "GB_per_s_at_median": round(nbytes / t[len(t) // 2] * 1e-3, 2)}
        print(f"{k:52s} median {t[len(t) // 2]:8.2f} us   min {t[0]:8.2f} us   {nbytes / 1e6:8.3f} MB written")
    print(f"launch + host-visible completion floor (mir_debug_null_roundtrip): {floor:.2f} us")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
