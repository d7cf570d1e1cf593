"""Developer probe: sha256 of every output of the four link / tree query kernels (link_kinematics, link_accelerations, dynamics,
task_dynamics) at a seeded state, to compare two builds of the library bit for bit.

    python tools/probes/query_bits.py [--out digests.json]

Franka pick scene (16-lane model) and five-cube stack scene (wave model), 5 envs, state set with set_state from a fixed seed.  Each call
asks for every output of three links (the hand, an arm link, the last body) at non-zero local points, once for a 7-row env_idx with
repeats (21 (row, link) pairs: five whole waves and a ragged one) and once for the full batch.  Prints one JSON object
{scene: {rows: {call.output: sha256}}}; run it on both builds and compare the two objects."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "gym-genesis_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gym_genesis.backend import models  # noqa: E402
from gym_genesis.backend.lib import MirScene  # noqa: E402

B = 5


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def scene_digests(builder, seed):
    spec = builder.build()
    sc = MirScene(spec, B)
    rng = np.random.default_rng(seed)
    q, v, _, _ = (t.cpu().numpy() for t in sc.get_state())
    sc.set_state(qpos=(q + rng.uniform(-0.3, 0.3, q.shape)).astype(np.float32), qvel=rng.uniform(-1, 1, v.shape).astype(np.float32))
    links = [int(spec.task.eef_body), 4, sc.nbody - 1]
    pts = rng.uniform(-0.1, 0.1, (3, 3)).astype(np.float32)
    offs = rng.uniform(-1, 1, (3, 4)).astype(np.float32)
    out = {}
    for name, idx in (("rows", [3, 0, 4, 1, 3, 2, 0]), ("batch", None)):
        R = B if idx is None else len(idx)
        env_idx = None if idx is None else torch.as_tensor(idx, device=sc.device)
        qacc = torch.as_tensor(rng.uniform(-2, 2, (R, sc.nv)).astype(np.float32), device=sc.device)
        calls = {
            "link_kinematics": sc.link_kinematics(links, pts, env_idx=env_idx),
            "link_accelerations": sc.link_accelerations(links, pts, offs, env_idx=env_idx, qacc=qacc, acc=True, bias_acc=True, imu=True),
            "dynamics": sc.dynamics(env_idx=env_idx, qacc=qacc, mass=True, bias=True, gravity=True, tau=True, ctrl_force=True),
            "task_dynamics": sc.task_dynamics(links, pts, env_idx=env_idx, x=qacc, damping=0.05, minv=True, solve=True, lambda_inv=True,
                                              lambda_=True, jbar=True),
        }
        torch.cuda.synchronize()
        out[name] = {f"{c}.{k}": digest(t) for c, r in calls.items() for k, t in sorted(r.items())}
    return {"kernel": sc.kernel, **out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    a = ap.parse_args()
    res = {"franka_cube_pick": scene_digests(models.franka_cube_pick_scene(), 1), "franka_cube_stack": scene_digests(models.franka_cube_stack_scene(), 2)}
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
