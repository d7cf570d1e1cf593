"""examples/franka/plan_optimize_retime_follow.py on the GPU at 8 envs with a short path: it completes, at least one row is OK, and the
OK rows' optimised paths have lower S (the discrete integral of |q'|^2) than their seeds -- what tests/test_opt_cpu.py asserts of the
float64 reference, here through the planner, the optimiser and the retimer."""
import importlib.util
import os
import sys

import pytest

pytestmark = pytest.mark.gpu


def test_the_example_runs(monkeypatch):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("plan_optimize_retime_follow", os.path.join(root, "examples", "franka", "plan_optimize_retime_follow.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(sys, "argv", ["plan_optimize_retime_follow.py", "--num-envs", "8", "--waypoints", "24"])
    res = mod.main()
    print(f"\n[opt, example] { {k: v for k, v in res.items() if k != 'rows'} }")
    rows = res["rows"]
    assert all(res[m]["timed"] == 8 for m in ("polyline", "blended", "optimised"))
    assert rows["ok"].sum() >= 1, rows["status"]
    assert (rows["S_out"][rows["ok"]] < rows["S_in"][rows["ok"]]).all(), (rows["S_in"], rows["S_out"])
    assert len(rows["certified"]) == 8
