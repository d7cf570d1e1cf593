"""Developer probe: time per call of the multi-link IK kernel (MirScene.inverse_kinematics_multilink / mir_inverse_kinematics_multilink)
next to the single-link kernel (mir_inverse_kinematics_rows) on the same job, with device events.  Franka pick scene, 4096 envs by
default; targets are the scene's own link poses at home +- 0.5 rad on the arm (joint 4 clipped to [-2.9, -0.3]), the seed is the home pose.

    python tools/probes/ikm_time.py [--envs 4096] [--calls 100] [--out FILE]

Variants: the hand's full pose through the old kernel; the same through the new kernel (one link, full masks); both fingertips, full
pose, all nine dofs, finger targets uniform in [0, 0.04] (the limit rule at work); the hand's pose with eight samples on targets drawn
over the whole joint ranges.  Every variant calls the C entry point on buffers made once (the calls queue up behind one another: the events see the kernel, not a
wrapper), is warmed up, then every call is timed between two events of its own; median and minimum over the calls are printed, with
the iteration counts of the new kernel's rows."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "gym-genesis_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gym_genesis.backend import models  # noqa: E402
from gym_genesis.backend.lib import MirScene  # noqa: E402
from gym_genesis.backend.spec import IK_DEFAULTS, IK_INIT_BY_ENV, IK_POS_BY_ENV, IK_QUAT_BY_ENV, MirIkOptions, MirIkRows, make_ik_multi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B = a.envs
    sb = models.franka_cube_pick_scene()
    spec = sb.build()
    sc = MirScene(spec, B)
    hand, lf, rf = (sb.body_index(n) for n in ("hand", "left_finger", "right_finger"))
    rng = np.random.default_rng(0)
    home = np.tile(np.asarray(models.FRANKA_HOME, np.float32), (B, 1))
    lo = np.array([spec.dof[i].range[0] for i in range(7)])
    hi = np.array([spec.dof[i].range[1] for i in range(7)])

    def poses_at(q9):
        q = sc.get_state()[0].clone()
        q[:, :9] = torch.as_tensor(q9, dtype=torch.float32, device=sc.device)
        sc.set_state(qpos=q)
        pos, quat = sc.get_links()
        return pos.clone(), quat.clone()

    near = home.copy()
    near[:, :7] += rng.uniform(-0.5, 0.5, (B, 7)).astype(np.float32)
    near[:, 3] = np.clip(near[:, 3], -2.9, -0.3)
    near[:, 7:9] = rng.uniform(0.0, 0.04, (B, 2))
    far = home.copy()
    far[:, :7] = rng.uniform(lo, hi, (B, 7))
    p_near, q_near = poses_at(near)
    p_far, q_far = poses_at(far)
    seed = torch.as_tensor(home, device=sc.device)
    poses_at(home)
    hp, hq = p_near[:, hand].contiguous(), q_near[:, hand].contiguous()
    fp, fq = p_near[:, [lf, rf]].contiguous(), q_near[:, [lf, rf]].contiguous()
    gp, gq = p_far[:, hand].contiguous(), q_far[:, hand].contiguous()
    by_env = IK_POS_BY_ENV | IK_QUAT_BY_ENV | IK_INIT_BY_ENV
    # the C entry points themselves, on buffers made once: the host enqueues a call in a few microseconds, so the calls of a variant
    # queue up behind one another and the events around each see the kernel, not the wrapper
    qout = torch.empty((B, sc.n_arm), device=sc.device)
    err = torch.empty((B, 2, 2), device=sc.device)
    iters = torch.zeros((B,), dtype=torch.int32, device=sc.device)
    sample = torch.zeros((B,), dtype=torch.int32, device=sc.device)
    opt = MirIkOptions(**IK_DEFAULTS)
    rows = MirIkRows(None, B, by_env, 0, 0)
    stream = sc._stream()

    def old(p, q):
        return lambda: sc.lib.mir_inverse_kinematics_rows(sc.h, hand, C.byref(rows), p.data_ptr(), q.data_ptr(), seed.data_ptr(), C.byref(opt),
                                                          qout.data_ptr(), err.data_ptr(), stream)

    def new(links, p, q, **kw):
        mq = make_ik_multi(links, n_arm=sc.n_arm, **kw)
        mq.rows = MirIkRows(None, B, 0, 0, 0)
        return lambda: sc.lib.mir_inverse_kinematics_multilink(sc.h, C.byref(mq), p.data_ptr(), q.data_ptr(), seed.data_ptr(), C.byref(opt),
                                                               qout.data_ptr(), err.data_ptr(), iters.data_ptr(), sample.data_ptr(), stream)

    variants = {
        "mir_inverse_kinematics_rows: hand pose": (old(hp, hq), 0),
        "mir_inverse_kinematics_multilink: hand pose, one link, full masks": (new([hand], hp, hq), 1),
        "mir_inverse_kinematics_multilink: both fingers, full pose, nine dofs": (new([lf, rf], fp, fq), 2),
        "mir_inverse_kinematics_rows: hand pose, whole-range targets": (old(gp, gq), 0),
        "mir_inverse_kinematics_multilink: the same, 1 sample": (new([hand], gp, gq), 1),
        "mir_inverse_kinematics_multilink: the same, 8 samples": (new([hand], gp, gq, max_samples=8, seed=5), 1),
    }
    out = {"envs": B, "calls": a.calls, "variants": {}}
    lines = [f"ikm_time.py --envs {B} --calls {a.calls}: Franka pick scene, seed = home pose"]
    for k, (fn, L) in variants.items():   # (L: links of the new kernel's call, 0: the old kernel)
        for _ in range(10):
            assert fn() == 0
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.calls)]
        for e0, e1 in ev:
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize()
        t = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)
        rec = {"us_per_call_median": round(t[len(t) // 2], 2), "us_per_call_min": round(t[0], 2)}
        if L:
            e = err.reshape(-1)[:B * L * 2].reshape(B, L, 2)
            rec["mean_iters"] = round(float(iters.float().mean()), 2)
            rec["max_iters"] = int(iters.max())
            rec["converged"] = round(float(((e[:, :, 0] < 5e-4) & (e[:, :, 1] < 5e-3)).all(1).float().mean()), 4)
        out["variants"][k] = rec
        lines.append(f"{k:72s} median {rec['us_per_call_median']:9.2f} us   min {rec['us_per_call_min']:9.2f} us" +
                     (f"   iterations mean {rec['mean_iters']} max {rec['max_iters']}, converged {rec['converged']}" if "mean_iters" in rec else ""))
    lines.append(json.dumps(out))
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
