"""examples/franka/plan_to_pose.py end to end on 8 envs: every env keeps a goal, plans to it and ends within the example's own tolerance
of the hover pose."""
import importlib.util
import os
import sys

import pytest

pytestmark = pytest.mark.gpu


def test_example_plan_to_pose(monkeypatch):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("plan_to_pose", os.path.join(root, "examples", "franka", "plan_to_pose.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(sys, "argv", ["plan_to_pose.py", "--num-envs", "8", "--waypoints", "30"])
    valid, n_goals, err = mod.main()
    assert valid.all() and (n_goals >= 1).all(), (valid, n_goals)
    assert (err <= mod.TOL).all(), err
