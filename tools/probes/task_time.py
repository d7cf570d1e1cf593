"""Developer probe: time of MirScene.task_dynamics (mir_task_dynamics) per call, with device events, next to what the library offered for
the same answer before it: mir_dynamics (M) + mir_link_kinematics (J) + torch.linalg on the device (cholesky, cholesky_solve, bmm, inv).
Franka pick scene, 4096 envs by default, the hand link, damping 0.05.

    python tools/probes/task_time.py [--envs 4096] [--calls 200] [--rounds 5] [--out FILE]

Every variant is warmed up, then timed in `rounds` interleaved windows of `calls` back-to-back calls between two events; median and
minimum over the rounds are printed.  The two ways are compared on the same state first (largest difference per output, printed)."""
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
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, d = a.envs, 0.05
    sb = models.franka_cube_pick_scene()
    sc = MirScene(sb.build(), B)
    rng = np.random.default_rng(0)
    pos = np.stack([rng.uniform(0.45, 0.8, B), rng.uniform(-0.25, 0.25, B), np.full(B, 0.02)], 1).astype(np.float32)
    sc.reset(pos, np.tile(np.array([1, 0, 0, 0], np.float32), (B, 1)), np.tile(np.array(models.FRANKA_HOME, np.float32), (B, 1)))
    sc.step(5)
    hand = sb.body_index("hand")
    eye6 = d * d * torch.eye(6, device=sc.device)

    def one_launch():
        return sc.task_dynamics(links=[hand], dof0=0, n_dofs=9, damping=d)

    def composed():
        M = sc.dynamics(dof0=0, n_dofs=9, bias=False)["mass"]
        J = sc.link_kinematics([hand], dof0=0, n_dofs=9, pos=False, quat=False, vel=False)["jac"][:, 0]
        Lm = torch.linalg.cholesky(M)
        mjt = torch.cholesky_solve(J.transpose(1, 2), Lm)          # M^-1 J^T
        lam_inv = torch.bmm(J, mjt)
        lam = torch.linalg.inv(lam_inv + eye6)
        return {"lambda_inv": lam_inv, "lambda": lam, "jbar": torch.bmm(mjt, lam)}

    def one_launch_minv():
        return sc.task_dynamics(dof0=0, n_dofs=9, minv=True)

    def composed_minv():
        return torch.linalg.inv(sc.dynamics(dof0=0, n_dofs=9, bias=False)["mass"])

    x, y = one_launch(), composed()
    diff = {k: float((x[k][:, 0] - y[k]).abs().max()) for k in ("lambda_inv", "lambda", "jbar")}
    diff["minv"] = float((one_launch_minv()["minv"] - composed_minv()).abs().max())
    variants = {
        "mir_task_dynamics: hand, lambda_inv + lambda + jbar (1 launch)": one_launch,
        "mir_dynamics + mir_link_kinematics + torch.linalg, the same outputs": composed,
        "mir_task_dynamics: minv of the arm (1 launch)": one_launch_minv,
        "mir_dynamics + torch.linalg.inv": composed_minv,
    }
    for fn in variants.values():
        for _ in range(20):
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
    floor = sc.null_roundtrip_us(2000)
    out = {"envs": B, "calls_per_window": a.calls, "rounds": a.rounds, "null_roundtrip_us": round(floor, 3), "max_abs_difference": diff, "variants": {}}
    lines = [f"task_time.py --envs {B} --calls {a.calls} --rounds {a.rounds}: Franka pick scene, hand link, arm window (9 dofs), damping {d}",
             "largest difference between the two ways on the same state: " + ", ".join(f"{k} {v:.3e}" for k, v in diff.items())]
    for k in variants:
        t = sorted(times[k])
        out["variants"][k] = {"us_per_call_median": round(t[len(t) // 2], 3), "us_per_call_min": round(t[0], 3)}
        lines.append(f"{k:70s} median {t[len(t) // 2]:9.2f} us   min {t[0]:9.2f} us")
    lines.append(f"launch + host-visible completion floor (mir_debug_null_roundtrip): {floor:.2f} us")
    lines.append(json.dumps(out))
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
