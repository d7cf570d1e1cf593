"""HIP-event times of mir_render_outputs' aux pass (depth / segmentation / normal), in the manner of tools/render_time.py.

    python tools/render_outputs_time.py            # per-env 1024 x 480 x 640, 4096 x 84 x 84, the global view at 4096 envs
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


def per_env(B, W, H):
    b, sc = scene(B)
    cam, vis = make_camera(W, H, (3.5, 0, 2.5), (0, 0, 0.5), 30), b.visual()
    base = (B, H, W)
    d = torch.empty(base, dtype=torch.float32, device=sc.device)
    s = torch.empty(base, dtype=torch.int32, device=sc.device)
    n = torch.empty(base + (3,), dtype=torch.uint8, device=sc.device)
    rgb = torch.empty(base + (3,), dtype=torch.uint8, device=sc.device)
    px = B * H * W
    for name, kw, nbytes in (("rgb (mir_render)", None, 3 * px), ("depth", dict(depth=True), 4 * px),
                             ("depth+seg+normal", dict(depth=True, segmentation=True, normal=True), 11 * px)):
        if kw is None:
            us = timed(lambda: sc.render(cam, vis, out=rgb))
        else:
            us = timed(lambda: sc.render_outputs(cam, vis, rgb=False, out=(None, d, s, n), **kw))
        print(f"per-env B={B} {W}x{H} {name}: {us:.1f} us/render  {nbytes / 1e9:.3f} GB  {nbytes / us / 1e6:.2f} TB/s written  "
              f"({nbytes / us / 1e6 / 8.0:.2f} of 8 TB/s)")
    flat = d.view(-1)
    us = timed(lambda: flat.fill_(1.0))
    print(f"    torch fill_ of the depth buffer ({4 * px / 1e9:.3f} GB): {us:.1f} us  {4 * px / us / 1e6:.2f} TB/s")
    del sc, d, s, n, rgb
    torch.cuda.empty_cache()


def global_view(B, W=640, H=480):
    b, sc = scene(B)
    side = int(np.ceil(np.sqrt(B)))
    idx = np.arange(B)
    off = torch.as_tensor(np.stack([(idx % side - (side - 1) / 2) * 1.0, (idx // side - (side - 1) / 2) * 1.0, np.zeros(B)], 1)
                          .astype(np.float32), device=sc.device)
    cam, vis = make_camera(W, H, (3.5, 0, 2.5), (0, 0, 0.5), 30), b.visual()
    us_rgb = timed(lambda: sc.render(cam, vis, mode=1, env_offset=off))
    us_aux = timed(lambda: sc.render_outputs(cam, vis, mode=1, env_offset=off, rgb=False, depth=True, segmentation=True, normal=True))
    print(f"global B={B} {W}x{H}: rgb {us_rgb:.1f} us, depth+seg+normal {us_aux:.1f} us")


if __name__ == "__main__":
    per_env(1024, 640, 480)
    per_env(4096, 84, 84)
    global_view(4096)
