"""Developer probe: time of MirScene.raycast (mir_raycast) per call, with device events, next to the depth image of the rasteriser.
Franka pick scene, 4096 envs by default.

    python tools/probes/ray_time.py [--envs 4096] [--calls 200] [--rounds 5]

  (a) the hand lidar 64 x 16 (skip_own_entity), distances only      (b) the same with all four outputs
  (c) a world-fixed 64 x 48 depth pattern, distances only           (d) render_outputs(rgb=False, depth=True) at 64 x 48, per env
Every variant is warmed up, then timed in `rounds` interleaved windows of `calls` back-to-back calls between two events; median and
minimum over the rounds are printed, with the bytes a call writes and the share of --hbm-write-gbs those stores reach."""
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
from gym_genesis.backend.spec import make_camera  # noqa: E402
from gym_genesis.tasks import sensors  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--hbm-write-gbs", type=float, default=0.0, help="write rate to relate the stores to (0: measured here with a device fill)")
    a = ap.parse_args()
    B = a.envs
    sb = models.franka_cube_pick_scene()
    spec = sb.build()
    sc = MirScene(spec, B)
    rng = np.random.default_rng(0)
    pos = np.stack([rng.uniform(0.45, 0.8, B), rng.uniform(-0.25, 0.25, B), np.full(B, 0.02)], 1).astype(np.float32)
    sc.reset(pos, np.tile(np.array([1, 0, 0, 0], np.float32), (B, 1)), np.tile(np.array(models.FRANKA_HOME, np.float32), (B, 1)))
    sc.step(5)
    hand = sb.body_index("hand")
    top = lambda b: b if spec.body[b].parent == 0 else top(spec.body[b].parent)  # noqa: E731
    own = sum(1 << g for g in range(spec.ngeom) if spec.geom[g].body and top(spec.geom[g].body) == top(hand))
    lidar = torch.as_tensor(sensors.SphericalPattern((360.0, 30.0), (64, 16)).directions(), device=sc.device)
    depth = torch.as_tensor(sensors.DepthCameraPattern((64, 48), 50.0).directions(), device=sc.device)
    cpos, look = (1.2, 0.0, 0.9), (0.3, 0.0, 0.2)
    cq = sensors.lookat_quat(cpos, look)
    cam, vis = make_camera(64, 48, cpos, look, 50.0), sb.visual(round_geoms=True)
    variants = {
        "(a) hand lidar 64x16, distances": (lambda: sc.raycast(lidar, link=hand, skip_geoms=own, max_range=10.0, points=False), B * 1024 * 4),
        "(b) hand lidar 64x16, all four outputs": (lambda: sc.raycast(lidar, link=hand, skip_geoms=own, max_range=10.0, geom=True, normal=True), B * 1024 * 32),
        "(c) world depth pattern 64x48, distances": (lambda: sc.raycast(depth, pos_offset=cpos, quat_offset=cq, max_range=10.0, points=False), B * 3072 * 4),
        "(d) rasteriser depth image 64x48": (lambda: sc.render_outputs(cam, vis, mode=0, rgb=False, depth=True), B * 3072 * 4),
    }
    for fn, _ in variants.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    # the write rate a plain device fill reaches on a buffer of 256 MB (the reference point of the stores)
    rate = a.hbm_write_gbs
    if rate <= 0.0:
        buf = torch.empty(64 << 20, dtype=torch.float32, device=sc.device)
        for _ in range(3):
            buf.fill_(1.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            buf.fill_(2.0)
        e1.record()
        e1.synchronize()
        rate = buf.numel() * 4 * 20 / (e0.elapsed_time(e1) * 1e-3) * 1e-9
        del buf
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
    out = {"envs": B, "calls_per_window": a.calls, "rounds": a.rounds, "fill_write_GB_per_s": round(rate, 1), "variants": {}}
    print(f"device fill of 256 MB: {rate:.0f} GB/s written")
    for k, (_, nbytes) in variants.items():
        t = sorted(times[k])
        med = t[len(t) // 2]
        gbs = nbytes / med * 1e-3
        out["variants"][k] = {"us_per_call_median": round(med, 2), "us_per_call_min": round(t[0], 2), "bytes_written": nbytes, "GB_per_s_at_median": round(gbs, 1),
                              "share_of_fill_rate": round(gbs / rate, 3)}
        print(f"{k:44s} median {med:9.2f} us   min {t[0]:9.2f} us   {nbytes / 1e6:8.2f} MB written   {gbs:7.1f} GB/s = {gbs / rate:.3f} of the fill rate")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
