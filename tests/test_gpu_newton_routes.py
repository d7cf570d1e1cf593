"""GPU: the instantiations that share the 16-lane kernel's Newton loop (mir_step_body.inc) agree bit for bit on the headline workload
(CubePick-v0, Franka, 4096 envs, U(-1, 1) actions) over a few hundred steps, in the steps that hold envs with three or more Newton
iterations as well: the rotated launch of step_begin / step_end (<5>), the fused launch (<0>), the K-step rollout (<1>), and every env
on the three-contacts-per-lane list instantiation (set_exact_contacts("all"), <6> / <7>: at most 16 points here, so the helper wave's
shares are exact zeros)."""
import numpy as np
import pytest
import torch

from gym_genesis.backend import models

pytestmark = pytest.mark.gpu
HOME = np.array(models.FRANKA_HOME, dtype=np.float32)
B, STEPS, K = 4096, 320, 16


def _reset(sc):
    rng = np.random.RandomState(0)
    pos = np.stack([rng.uniform(0.45, 0.80, B), rng.uniform(-0.25, 0.25, B), np.full(B, 0.02)], 1).astype(np.float32)
    sc.reset(pos, np.tile(np.array([0, 0, 0, 1], np.float32), (B, 1)), np.tile(HOME, (B, 1)))


def _same_state(a, b):
    return all(torch.equal(x, y) for x, y in zip(a.get_state(), b.get_state()))


def test_rotated_fused_rollout_and_list_routes_agree_through_three_iteration_steps(franka_spec, monkeypatch):
    from gym_genesis.backend.lib import MirScene

    monkeypatch.setenv("MIR_SPLIT_STEP", "1")
    rot, fused, roll, lst = (MirScene(franka_spec, B) for _ in range(4))
    assert rot.split_step == 1
    lst.set_exact_contacts("all")
    for s in (rot, fused, roll, lst):
        _reset(s)
    fused.set_diag(True)
    g = torch.Generator(device=rot.device).manual_seed(1)
    acts = torch.empty((STEPS, B, 9), device=rot.device).uniform_(-1.0, 1.0, generator=g)
    bufs = {id(s): (s.empty(9), s.empty(11), s.empty(), s.empty(dtype=torch.uint8)) for s in (rot, fused, lst)}
    rows = torch.zeros((K, B, roll.agent_dim + roll.env_dim + 2), device=roll.device)
    most, steps3 = 0, 0
    for t0 in range(0, STEPS, K):
        roll.rollout(acts[t0:t0 + K].contiguous(), rows)
        for t in range(t0, t0 + K):
            rot.step_begin(acts[t], *bufs[id(rot)])
            host = rot.step_end()
            lst.step_begin(acts[t], *bufs[id(lst)])
            lst.step_end()
            fused.step_fused(acts[t], *bufs[id(fused)])
            ni = fused.get_diag()[2]
            most = max(most, int(ni.max()))
            steps3 += int(ni.max()) >= 3
            for x, y, z in zip(bufs[id(rot)], bufs[id(fused)], bufs[id(lst)]):
                assert torch.equal(x, y) and torch.equal(x, z), t
            assert np.array_equal(host, bufs[id(fused)][3].cpu().numpy().astype(bool)), t
        assert _same_state(rot, fused) and _same_state(roll, fused) and _same_state(lst, fused), t0
    assert most >= 3 and steps3 >= STEPS // 4, (most, steps3)
