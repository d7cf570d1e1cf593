"""GPU tier: the kernels of the sphere model that share a phase (gym-genesis_amd/csrc/mir_sphere_front.h) agree on it bit for bit.
mir_signed_distance, mir_self_distance and mir_path_clearance reach a row's clearance through the same forward kinematics, probe
centres and distance functions, so on the same rows they must return the same floats; and all three clamp a row's env index the same
way.  Inputs: the B = 5 rows of plan_cases "post" and the sphere models of self_cases / carry_cases; states are SET."""
import numpy as np
import pytest
import torch

import carry_cases as cc
import plan_cases as pc
import self_cases as sfc

pytestmark = pytest.mark.gpu

B = pc.B
_scenes = {}


def _scene(key, c):
    if key not in _scenes:
        from gym_genesis.backend.lib import MirScene

        sc = MirScene(c["spec"], B)
        sc.set_state(qpos=c["q"], qvel=np.zeros((B, sc.nv), np.float32))
        _scenes[key] = sc
    return _scenes[key]


def _self_case():
    """a self model with N < 64 < N + E and N + E no multiple of 64 (the list then spans a whole and a ragged chunk, the extra probes
    start inside the first) if a case offers one, else self_cases' own"""
    cands = [("self fold", sfc.case("fold"))] + [("carry " + n, cc.case(n)) for n in cc.NAMES]
    for key, c in cands:
        ns, n = len(c["links"]), len(c["links"]) - c["n_extra"]
        if n < 64 < ns and ns % 64:
            return key, c
    return cands[0]


def _still(c, rows=slice(None)):
    """(R, 2, D): every row's start twice -- a path of one segment that stays where it is"""
    return np.repeat(c["start"][rows][:, None], 2, axis=1)


def test_distance_and_path_clearance_agree_on_a_row():
    c = pc.case("post")
    sc = _scene("post", c)
    q = torch.as_tensor(c["q"], device=sc.device)
    dist = sc.signed_distance(c["probes"], links=c["links"], qpos=q, max_distance=1.0, skip_geoms=c["skip"], row_min=True)["row_min"]
    path = sc.path_clearance(c["probes"], c["links"], c["qadr"], _still(c), qpos_start=q, max_distance=1.0, skip_geoms=c["skip"])["row_min"]
    print(f"\n[sphere front] scene clearance of the post rows: signed_distance {dist.cpu().numpy()} path_clearance {path.cpu().numpy()}")
    assert torch.isfinite(dist).all() and (dist < 1.0).all(), "the rows are near the post: the comparison is of distances, not of the cap"
    assert torch.equal(dist, path)


def test_self_distance_and_path_clearance_agree_on_a_row():
    key, c = _self_case()
    sc = _scene(key, c)
    q = torch.as_tensor(c["q"], device=sc.device)
    own = sc.self_distance(c["probes"], c["links"], c["mask"], qpos=q, max_distance=1.0, n_extra=c["n_extra"], row_min=True)["row_min"]
    path = sc.path_clearance(c["probes"], c["links"], c["qadr"], _still(c), qpos_start=q, max_distance=1.0, skip_geoms=c["skip"],
                             self_model=dict(link_mask=c["mask"], n_extra=c["n_extra"], self_margin=0.0, max_distance=1.0))["row_self_min"]
    print(f"\n[sphere front] self clearance ({key}: N = {len(c['links']) - c['n_extra']}, E = {c['n_extra']}): self_distance {own.cpu().numpy()} "
          f"path_clearance {path.cpu().numpy()}")
    assert torch.isfinite(own).all() and (own < 1.0).all()
    assert torch.equal(own, path)


def test_every_family_clamps_the_env_index_alike():
    """a row list with a repeat and indices on either side of the batch gives the rows of the clamped list (the rows' own state is
    evaluated, so the env decides the result; the planner's random numbers are keyed by it, too)"""
    given, clamped = [3, 0, 3, B + 2, -1], [3, 0, 3, B - 1, 0]
    c = pc.case("post")
    sc = _scene("post", c)
    key, s = _self_case()
    ss = _scene(key, s)
    sm = dict(link_mask=s["mask"], n_extra=s["n_extra"], self_margin=0.0, max_distance=1.0)
    budget = dict(num_waypoints=pc.BUDGET["W"], max_nodes=pc.BUDGET["max_nodes"], max_iterations=pc.BUDGET["max_iterations"], resolution=pc.RESOLUTION,
                  step=pc.STEP, margin=pc.MARGIN, skip_geoms=c["skip"])
    calls = {
        "signed_distance": lambda idx: sc.signed_distance(c["probes"], links=c["links"], env_idx=idx, skip_geoms=c["skip"], geom=True, closest=True,
                                                          normal=True, row_min=True),
        "self_distance": lambda idx: ss.self_distance(s["probes"], s["links"], s["mask"], env_idx=idx, n_extra=s["n_extra"], other=True, row_min=True),
        "path_clearance": lambda idx: sc.path_clearance(c["probes"], c["links"], c["qadr"], np.stack([c["start"][clamped], c["goal"][clamped]], 1),
                                                        env_idx=idx, skip_geoms=c["skip"]),
        "path_clearance, self": lambda idx: ss.path_clearance(s["probes"], s["links"], s["qadr"], np.stack([s["start"][clamped], s["goal"][clamped]], 1),
                                                              env_idx=idx, skip_geoms=s["skip"], self_model=sm),
        "plan_path": lambda idx: sc.plan_path(c["probes"], c["links"], c["qadr"], c["goal"][clamped], env_idx=idx, **budget),
    }
    for name, call in calls.items():
        got, want = call(torch.tensor(given, device=sc.device)), call(torch.tensor(clamped, device=sc.device))
        assert sorted(got) == sorted(want)
        for k in want:
            assert torch.equal(got[k], want[k]), (name, k)
        assert all(torch.equal(t[0], t[2]) for t in want.values()), (name, "a repeated row repeats")
        assert any(not torch.equal(t[0], t[1]) for t in want.values()), (name, "another env differs in some output: the env decides the result")
