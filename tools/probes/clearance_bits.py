"""Developer probe: sha256 of every output of the sphere-model kernels (mir_signed_distance, mir_self_distance, mir_plan_path,
mir_path_clearance and their _self / _carry forms), to compare two builds of the library bit for bit -- the companion of query_bits.py
and ik_bits.py.

    python tools/probes/clearance_bits.py [--out digests.json]

Inputs are the cases of the tests (tests/dist_cases.py: zoo, pick = 16-lane model, stack = wave model; plan_cases "post", self_cases
"fold", carry_cases "under" and "rod": the pick scene), 5 envs, states SET.  signed_distance with every optional output at the state
and at the case's candidate rows; self_distance at the state and at the start rows; plan_path and path_clearance plain, with the self
model and with the carried object.  Every call once for the full batch and once for a 7-row env_idx with repeats.  Prints one JSON
object {case: {rows: {call.output: sha256}}}; run it on both builds and compare."""
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

import carry_cases  # noqa: E402
import dist_cases  # noqa: E402
import plan_cases  # noqa: E402
import self_cases  # noqa: E402
from gym_genesis.backend.lib import MirScene  # noqa: E402

B = 5
ROWS = [3, 0, 4, 1, 3, 2, 0]
BUDGET = dict(num_waypoints=plan_cases.BUDGET["W"], max_nodes=plan_cases.BUDGET["max_nodes"], max_iterations=plan_cases.BUDGET["max_iterations"],
              resolution=plan_cases.RESOLUTION, step=plan_cases.STEP, margin=0.0)


def digests(prefix, out, d):
    for k, t in out.items():
        d[f"{prefix}.{k}"] = hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def scene(c):
    sc = MirScene(c["spec"], B)
    sc.set_state(qpos=c["q"], qvel=np.zeros((B, sc.nv), np.float32))
    return sc


def both_row_lists(sc, fill):
    """fill(d, idx, take): idx the env_idx argument, take(a) the rows of a per-env array that go with it"""
    out = {}
    for name, rows in (("rows", ROWS), ("batch", None)):
        idx = None if rows is None else torch.as_tensor(rows, device=sc.device)
        d = {}
        fill(d, idx, (lambda a: a) if rows is None else (lambda a: a[rows]))
        torch.cuda.synchronize()
        out[name] = d
    return {"kernel": sc.kernel, **out}


def distance_digests(name):
    c, sc = dist_cases.case(name), scene(dist_cases.case(name))
    cand = dist_cases.candidate(name)["q"].astype(np.float32)

    def fill(d, idx, take):
        kw = dict(links=c["links"], env_idx=idx, max_distance=c["max_distance"], skip_geoms=c["skip"], geom=True, closest=True, normal=True, row_min=True)
        digests("signed_distance state", sc.signed_distance(c["probes"], **kw), d)
        digests("signed_distance qpos", sc.signed_distance(c["probes"], qpos=take(cand), **kw), d)
    return both_row_lists(sc, fill)


def planner_digests(c, sc, d, idx, take, label, **model):
    paths = np.stack([take(c["start"]), 0.5 * (take(c["start"]) + take(c["goal"])), take(c["goal"])], 1).astype(np.float32)
    digests(f"plan_path {label}", sc.plan_path(c["probes"], c["links"], c["qadr"], take(c["goal"]), env_idx=idx, skip_geoms=c["skip"], **BUDGET, **model), d)
    digests(f"path_clearance {label}", sc.path_clearance(c["probes"], c["links"], c["qadr"], paths, env_idx=idx, skip_geoms=c["skip"],
                                                         resolution=plan_cases.RESOLUTION, **model), d)
    digests(f"path_clearance {label} start rows", sc.path_clearance(c["probes"], c["links"], c["qadr"], paths, env_idx=idx, qpos_start=take(c["q"]),
                                                                    skip_geoms=c["skip"], resolution=plan_cases.RESOLUTION, **model), d)


def plain_digests():
    c = plan_cases.case("post")
    sc = scene(c)
    return both_row_lists(sc, lambda d, idx, take: planner_digests(c, sc, d, idx, take, "plain"))


def self_digests():
    c = self_cases.case("fold")
    sc = scene(c)
    sm = dict(link_mask=c["mask"], n_extra=c["n_extra"], self_margin=0.0, max_distance=1.0)

    def fill(d, idx, take):
        kw = dict(env_idx=idx, n_extra=c["n_extra"], other=True, row_min=True)
        digests("self_distance state", sc.self_distance(c["probes"], c["links"], c["mask"], **kw), d)
        digests("self_distance qpos", sc.self_distance(c["probes"], c["links"], c["mask"], qpos=take(c["q"])[::-1].copy(), **kw), d)
        planner_digests(c, sc, d, idx, take, "self", self_model=sm)
    return both_row_lists(sc, fill)


def carry_digests(name):
    c = carry_cases.case(name)
    sc = scene(c)
    sm = dict(link_mask=c["mask"], n_extra=c["n_extra"], self_margin=0.0, max_distance=1.0)

    def fill(d, idx, take):
        planner_digests(c, sc, d, idx, take, "carry", self_model=sm, carry=dict(body=c["body"], link=c["link"], grasp=None))
        given = torch.as_tensor(take(c["grasp"]).astype(np.float32), device=sc.device)
        planner_digests(c, sc, d, idx, take, "carry, grasp given", self_model=sm, carry=dict(body=c["body"], link=c["link"], grasp=given))
        n = len(c["links"]) - c["n_extra"]   # (the scene-test probes: the arm's and the carried body's)
        cn = dict(c, probes=c["probes"][:n], links=c["links"][:n])
        planner_digests(cn, sc, d, idx, take, "carry, no self", carry=dict(body=c["body"], link=c["link"], grasp=None))
    return both_row_lists(sc, fill)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    a = ap.parse_args()
    res = {f"dist {n}": distance_digests(n) for n in ("zoo", "pick", "stack")}
    res.update({"plan post": plain_digests(), "self fold": self_digests()})
    res.update({f"carry {n}": carry_digests(n) for n in carry_cases.NAMES})
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    print("digests:", sum(len(v) for s in res.values() for k, v in s.items() if k != "kernel"), file=sys.stderr)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
