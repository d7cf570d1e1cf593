"""Developer probe: sha256 of every output of the certified-clearance kernel (mir_certify_path, mir_certify_path_self,
mir_certify_path_carry through MirScene.certify_path), to compare two builds of the library bit for bit -- the companion of
clearance_bits.py, query_bits.py and ik_bits.py.

    python tools/probes/certify_bits.py [--out digests.json]

Inputs are the cases of the tests: every name of tests/cert_cases.py through mir_certify_path, every name of tests/certrel_cases.py
through the entry point that case uses (a self model: _self; a carried body, with or without one: _carry), 5 envs, states SET.  Every
case with and without `bracket`, max_leaves = 512 as the tests set it, once for the full batch and once for a 7-row env_idx with
repeats.  Every output tensor is hashed: the seg_* and row_* bounds and statuses, stats and leaves, and for the relative entry points
the self bounds and grasp.  Prints one JSON object {case: {rows: {bracket.output: sha256}}}; run it on both builds and compare."""
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

import cert_cases  # noqa: E402
import certrel_cases  # noqa: E402
from gym_genesis.backend.lib import MirScene  # noqa: E402

B = 5
ROWS = [3, 0, 4, 1, 3, 2, 0]
MAX_LEAVES = 512


def case_digests(c):
    sc = MirScene(c["spec"], B)
    sc.set_state(qpos=c["q"], qvel=np.zeros((B, sc.nv), np.float32))
    kw = dict(probes=c["probes"], links=c["links"], dof_qadr=c["qadr"], skip_geoms=c["skip"], max_distance=c["max_distance"], max_leaves=MAX_LEAVES)
    if c.get("mask") is not None:
        kw["self_model"] = dict(link_mask=c["mask"], n_extra=c["n_extra"], self_margin=c["self_margin"], max_distance=c["self_max"])
    out = {}
    for name, rows in (("rows", ROWS), ("batch", None)):
        idx = None if rows is None else torch.as_tensor(rows, device=sc.device)
        take = (lambda a: a) if rows is None else (lambda a: a[rows])
        if c.get("carry") is not None:
            g = None if c["grasp"] is None else torch.as_tensor(take(c["grasp"]), device=sc.device)
            kw["carry"] = dict(body=c["carry"][0], link=c["carry"][1], grasp=g)
        d = {}
        for bracket in (False, True):
            got = sc.certify_path(paths=take(c["paths"]), env_idx=idx, **{**c["par"], "bracket": bracket}, **kw)
            for k, t in got.items():
                d[f"{'bracket' if bracket else 'margin'}.{k}"] = hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
        torch.cuda.synchronize()
        out[name] = d
    return {"kernel": sc.kernel, **out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    a = ap.parse_args()
    res = {f"scene {n}": case_digests(cert_cases.case(n)) for n in cert_cases.NAMES}
    res.update({f"relative {n}": case_digests(certrel_cases.case(n)) for n in certrel_cases.NAMES})
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    print("digests:", sum(len(v) for s in res.values() for k, v in s.items() if k != "kernel"), file=sys.stderr)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
