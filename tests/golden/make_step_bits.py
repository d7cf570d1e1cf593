"""Generator of tests/golden/step_bits.json: sha256 digests of what the 16-lane step kernel computes on gfx950, instantiation by
instantiation, for tests/test_gpu_step_bits.py.

    python tests/golden/make_step_bits.py            # on an MI355X, from the repository root, with the library built

The fixture pins the BITS of this kernel on gfx950: it is written on the commit whose arithmetic is to be kept, and a change that is
meant to leave every result as it was (compiler flags, scheduling, instruction selection, register moves) must reproduce it.  A later
change that alters the arithmetic ON PURPOSE (another operation order, another fma formation, another solver) regenerates the file with
the command above on its own commit and says so in its description; nothing else may.

What is digested (digests(), shared with the test): for every scene x batch x route the bytes of qpos, qvel, qacc_ws (the solver's warm
start), the observation tensors, reward and terminated after every 8th of 88 steps:

  * 48 steps of seeded U(-1, 1) targets from the task's reset;
  * then, Franka scenes: the scene put back to the home pose with the cubes of tests/golden/grasp_targets.json, and the first 8 steps of
    each of its 5 stages (hover, stabilize, descend, close, lift: the pads meet the cube); SO-101 (six dofs, no such script): 40 more
    U(-1, 1) steps.

Scenes: the Franka pick scene with capsule links (mir_step_convex.hip), with box links (mir_step.hip, built with -fno-signed-zeros) and
the SO-101 pick scene (the non-specialised instantiation).  Batches: 5 (a partly filled wave) and 8.  Routes: `step_raw` (the fused
launch), `GenesisEnv.step` (the rotated launch), K = 4 rollouts (the device-side loop, exact contacts kept) and -- Franka -- every env
on the three-contacts-per-lane list instantiation (set_exact_contacts("all"))."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "step_bits.json")
SCENES = {"franka_capsule": dict(robot="franka", link_shape="capsule"), "franka_box": dict(robot="franka", link_shape="box"),
          "so101": dict(robot="so101")}
BATCHES = (5, 8)
ROUTES = ("fused", "rotated", "rollout", "list")
RANDOM_STEPS, STAGE_STEPS, EVERY, K = 48, 8, 8, 4


def _sha(*tensors) -> str:
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t).tobytes())
    return h.hexdigest()


def routes_of(scene: str):
    return ROUTES if scene.startswith("franka") else ROUTES[:3]


def actions(scene: str, B: int, nu: int):
    """(88, B, nu) float32 targets and the step at which the scripted part starts (None: all of them random)."""
    rng = np.random.RandomState(1)
    if not scene.startswith("franka"):
        return rng.uniform(-1.0, 1.0, (RANDOM_STEPS + 5 * STAGE_STEPS, B, nu)).astype(np.float32), None
    G = json.load(open(os.path.join(HERE, "grasp_targets.json")))
    T = np.array(G["targets"], np.float32)                                    # (4 cubes, 5 stages, 9)
    rand = rng.uniform(-1.0, 1.0, (RANDOM_STEPS, B, nu)).astype(np.float32)
    grasp = np.repeat(T.transpose(1, 0, 2), STAGE_STEPS, axis=0)              # (40, 4, 9)
    grasp = np.tile(grasp, (1, (B + 3) // 4, 1))[:, :B]
    return np.concatenate([rand, grasp]), RANDOM_STEPS


def digests(scene: str, B: int, route: str) -> list:
    """One record per 8th step: {"step", "qpos", "qvel", "qacc_ws", "agent_pos", "environment_state", "reward", "terminated"}."""
    import torch

    from gym_genesis.backend import models
    from gym_genesis.env import GenesisEnv

    kw = dict(SCENES[scene])
    env = GenesisEnv(task="cube_pick", robot=kw.pop("robot"), num_envs=B, enable_pixels=False, **kw)
    env.reset(seed=0)
    task = env._env
    mir = task._mir
    if route == "list":
        mir.set_exact_contacts("all")
    acts_np, scripted = actions(scene, B, mir.nu)
    acts = torch.as_tensor(acts_np, device=mir.device)
    rows = torch.zeros((K, B, mir.agent_dim + mir.env_dim + 2), device=mir.device)
    out, t = [], 0
    while t < acts.shape[0]:
        if scripted is not None and t == scripted:
            G = json.load(open(os.path.join(HERE, "grasp_targets.json")))
            pos = np.tile(np.array([[x, y, 0.02] for x, y in G["cube_xy"]], np.float32), ((B + 3) // 4, 1))[:B]
            mir.reset(pos, np.tile(np.array([0, 0, 0, 1], np.float32), (B, 1)), np.tile(np.array(models.FRANKA_HOME, np.float32), (B, 1)))
        if route == "rollout":
            mir.rollout_exact(acts[t:t + K].contiguous(), rows)
            a, e = mir.agent_dim, mir.env_dim
            last = rows[K - 1]
            outs = (last[:, :a], last[:, a:a + e], last[:, a + e], last[:, a + e + 1])
            t += K
        elif route == "fused":
            task.step_raw(acts[t])
            outs = (task._agent, task._envst, task._reward, task._term)
            t += 1
        else:
            obs, reward, terminated, _, _ = env.step(acts[t])
            outs = (obs["agent_pos"], obs["environment_state"], reward, terminated)
            t += 1
        if t % EVERY == 0:
            q, v, _, w = mir.get_state()
            out.append({"step": t, "qpos": _sha(q), "qvel": _sha(v), "qacc_ws": _sha(w), "agent_pos": _sha(outs[0]),
                        "environment_state": _sha(outs[1]), "reward": _sha(outs[2]), "terminated": _sha(outs[3])})
    return out


def main():
    sys.path[:0] = [os.path.join(os.path.dirname(os.path.dirname(HERE)), "gym-genesis_amd")]
    import torch

    assert torch.cuda.is_available(), "the fixture is written on an MI355X"
    dst = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    doc = {"device": torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], "every": EVERY, "digests": {}}
    for scene in SCENES:
        for B in BATCHES:
            for route in routes_of(scene):
                doc["digests"][f"{scene}/B{B}/{route}"] = digests(scene, B, route)
    with open(dst, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", dst, len(doc["digests"]), "runs")


if __name__ == "__main__":
    main()
