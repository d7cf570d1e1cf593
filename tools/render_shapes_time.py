"""HIP-event A/B of MIR_VIS_ROUND_GEOMS (spheres and capsules drawn as themselves) against the bounding boxes, in one process, the two
alternated so that drift hits both alike.  The Franka pick scene (capsule links) in the manner of tools/render_outputs_time.py.

    python tools/render_shapes_time.py     # per-env 1024 x 480 x 640 RGB and depth-only, the global view at 4096 envs
"""
import os
import sys

import numpy as np
import torch

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_R, "gym-genesis_amd"))
from gym_genesis.backend import models  # noqa: E402
from gym_genesis.backend.lib import MirScene  # noqa: E402
from gym_genesis.backend.spec import make_camera  # noqa: E402

N = 20
ROUNDS = 3


def scene(B):
    b = models.franka_cube_pick_scene()
    sc = MirScene(b.build(), B)
    rng = np.random.RandomState(0)
    pos = np.stack([rng.uniform(0.45, 0.80, B), rng.uniform(-0.25, 0.25, B), np.full(B, 0.02)], 1).astype(np.float32)
    sc.reset(pos, np.tile(np.array([0, 0, 0, 1], np.float32), (B, 1)), np.tile(np.array(models.FRANKA_HOME, np.float32), (B, 1)))
    sc.step(5)
    return b, sc


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(N):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / N * 1e3  # us


def ab(label, fn_of_vis, b):
    vis = {"boxes": b.visual(), "round": b.visual(round_geoms=True)}
    res = {k: [] for k in vis}
    for _ in range(ROUNDS):
        for k, v in vis.items():
            res[k].append(timed(lambda: fn_of_vis(v)))
    print(f"{label}: " + "  ".join(f"{k} {' / '.join(f'{u:.1f}' for u in us)} us (min {min(us):.1f})" for k, us in res.items())
          + f"  round/boxes {min(res['round']) / min(res['boxes']):.3f}", flush=True)


def per_env(B, W, H):
    b, sc = scene(B)
    cam = make_camera(W, H, (3.5, 0, 2.5), (0, 0, 0.5), 30)
    rgb = torch.empty((B, H, W, 3), dtype=torch.uint8, device=sc.device)
    d = torch.empty((B, H, W), dtype=torch.float32, device=sc.device)
    ab(f"per-env B={B} {W}x{H} rgb (mir_render)", lambda v: sc.render(cam, v, out=rgb), b)
    ab(f"per-env B={B} {W}x{H} depth", lambda v: sc.render_outputs(cam, v, rgb=False, depth=True, out=(None, d, None, None)), b)
    del sc, rgb, d
    torch.cuda.empty_cache()


def global_view(B, W=640, H=480):
    b, sc = scene(B)
    side = int(np.ceil(np.sqrt(B)))
    idx = np.arange(B)
    off = torch.as_tensor(np.stack([(idx % side - (side - 1) / 2) * 1.0, (idx // side - (side - 1) / 2) * 1.0, np.zeros(B)], 1)
                          .astype(np.float32), device=sc.device)
    cam = make_camera(W, H, (3.5, 0, 2.5), (0, 0, 0.5), 30)
    ab(f"global B={B} {W}x{H} rgb", lambda v: sc.render(cam, v, mode=1, env_offset=off), b)
    ab(f"global B={B} {W}x{H} depth+seg+normal",
       lambda v: sc.render_outputs(cam, v, mode=1, env_offset=off, rgb=False, depth=True, segmentation=True, normal=True), b)


if __name__ == "__main__":
    per_env(1024, 640, 480)
    global_view(4096)
