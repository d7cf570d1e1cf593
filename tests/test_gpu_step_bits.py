"""GPU: the 16-lane step kernel computes, bit for bit, what tests/golden/step_bits.json recorded on gfx950 -- sha256 digests of qpos,
qvel, qacc_ws, the observation tensors, reward and terminated after every 8th of 88 steps (48 of seeded U(-1, 1) targets, then the
5 x 8-step prefix of the scripted grasp of tests/golden/grasp_targets.json), for the capsule-link scene (mir_step_convex.hip), the
box-link scene (mir_step.hip) and the SO-101 pick scene (the non-specialised instantiation), at B = 5 and B = 8, through `step_raw`
(fused), `GenesisEnv.step` (rotated), a K = 4 rollout and the three-contacts-per-lane list instantiation.

The fixture pins this kernel's bits on gfx950: build flags, scheduling and instruction selection must reproduce it.  A later change
that alters the arithmetic ON PURPOSE regenerates it on its own commit with `python tests/golden/make_step_bits.py` (on an MI355X,
library built) and says so; see that file's docstring for what is digested and how."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_step_bits", os.path.join(GOLDEN, "make_step_bits.py"))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)


@pytest.mark.parametrize("B", bits.BATCHES)
@pytest.mark.parametrize("scene", list(bits.SCENES))
def test_step_kernel_reproduces_the_recorded_bits(scene, B):
    import torch

    doc = json.load(open(bits.FIXTURE))
    assert torch.cuda.get_device_properties(0).gcnArchName.split(":")[0] == doc["device"], "the fixture holds the bits of " + doc["device"]
    state = {}
    for route in bits.routes_of(scene):
        want = doc["digests"][f"{scene}/B{B}/{route}"]
        got = bits.digests(scene, B, route)
        assert len(want) == (bits.RANDOM_STEPS + 5 * bits.STAGE_STEPS) // bits.EVERY
        for w, g in zip(want, got):
            diff = [k for k in w if w[k] != g[k]]
            assert not diff, f"{scene} B={B} {route}: step {w['step']}: {diff} differ from the recorded bits"
        assert len(got) == len(want)
        state[route] = [(g["qpos"], g["qvel"], g["qacc_ws"]) for g in got]
    # (the routes that thin nothing differently agree among themselves as well: fused == rotated == rollout while no env exceeds 16
    #  contact points -- the random part)
    n = bits.RANDOM_STEPS // bits.EVERY
    assert state["fused"][:n] == state["rotated"][:n] == state["rollout"][:n]
