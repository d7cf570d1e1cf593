"""Developer probe: sha256 of every output of the two inverse-kinematics kernels (mir_inverse_kinematics_rows,
mir_inverse_kinematics_multilink), to compare two builds of the library bit for bit -- the companion of query_bits.py.

    python tools/probes/ik_bits.py [--out digests.json]

Franka pick scene (16-lane model) and five-cube stack scene (wave model), 5 envs, seed = the home pose, targets from the float64 oracle
(tests/ikm_ref.py: build_case).  Single-link calls: the hand (eight chain elements), link4 (four) and link1 (one, behind the folded
base), each with and without a target quaternion, max_iters 100.  Multi-link calls: the seven cases of ikm_ref.GPU_CASES and the hand's
pose over the whole joint ranges with max_samples = 4.  Every call once for a 7-row env_idx with repeats (one whole wave and a ragged
one) and once for the full batch.  Prints one JSON object {scene: {rows: {call.output: sha256}}}; run it on both builds and compare."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in ("gym-genesis_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ikm_ref  # noqa: E402
import orc  # noqa: E402
from gym_genesis.backend import models  # noqa: E402
from gym_genesis.backend.lib import MirScene  # noqa: E402
from gym_genesis.backend.spec import IK_INIT_BY_ENV, IK_POS_BY_ENV, IK_QUAT_BY_ENV  # noqa: E402

B = 5
BY_ENV = IK_POS_BY_ENV | IK_QUAT_BY_ENV | IK_INIT_BY_ENV
HOME = models.FRANKA_HOME


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def scene_digests(builder):
    spec = builder.build()
    sc = MirScene(spec, B)
    o64, arm = orc.Oracle(spec, 1), ikm_ref.Arm(spec)
    dev = sc.device
    f32 = lambda a: None if a is None else torch.as_tensor(a, dtype=torch.float32, device=dev).contiguous()  # noqa: E731
    single = [ikm_ref.build_case(builder, spec, o64, arm, dict(name=n, links=(n,)), HOME, B, 200 + i) for i, n in enumerate(("hand", "link4", "link1"))]
    multi = [ikm_ref.build_case(builder, spec, o64, arm, c, HOME, B, 100 + i) for i, c in enumerate(ikm_ref.GPU_CASES)]
    restart = ikm_ref.restart_case(builder, spec, o64, arm, HOME, n=B)
    out = {}
    for name, idx in (("rows", [3, 0, 4, 1, 3, 2, 0]), ("batch", None)):
        env_idx = None if idx is None else torch.as_tensor(idx, device=dev)
        flags = 0 if idx is None else BY_ENV
        d = {}
        for c in single:
            for quat in (True, False):
                q, err = sc.inverse_kinematics_rows(c["links"][0], f32(c["poss"][:, 0]), f32(c["quats"][:, 0]) if quat else None, f32(c["seed_q"]),
                                                    env_idx, flags, return_error=True, max_iters=100)
                k = f"rows {c['name']} {'pose' if quat else 'position'}"
                d[k + ".qpos"], d[k + ".err"] = digest(q), digest(err)
        for c, kw in [(c, ikm_ref.kwargs(c)) for c in multi] + [(dict(restart, name="hand whole range, 4 samples"), dict(max_samples=4, seed=5))]:
            q, err, info = sc.inverse_kinematics_multilink(c["links"], c["poss"], c["quats"], c["seed_q"], env_idx=env_idx, flags=flags,
                                                           return_error=True, return_info=True, **kw)
            k = f"multilink {c['name']}"
            d[k + ".qpos"], d[k + ".err"], d[k + ".iters"], d[k + ".sample"] = digest(q), digest(err), digest(info["iters"]), digest(info["sample"])
        torch.cuda.synchronize()
        out[name] = d
    return {"kernel": sc.kernel, **out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    a = ap.parse_args()
    res = {"franka_cube_pick": scene_digests(models.franka_cube_pick_scene()), "franka_cube_stack": scene_digests(models.franka_cube_stack_scene())}
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
