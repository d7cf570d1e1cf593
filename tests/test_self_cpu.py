"""Self-collision of the sphere model, CPU tier: the host-side self model (EntityView.self_collision_model /
set_self_collision_pairs), the struct mirror, the wrappers' argument handling and refusals, and the conditions that make the GPU tier
(tests/test_gpu_self.py) fair -- in float64, with the reference of tests/self_ref.py on the cases of tests/self_cases.py.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import plan_cases as pc
import plan_ref
import self_cases as sc
import self_ref
from gym_genesis.backend import models
from gym_genesis.backend import spec as S
from gym_genesis.backend.lib import LIB_PATH
from gym_genesis.tasks.views import EntityView

CASES = ("fold", "swing")


def _robot():
    sb = models.franka_cube_pick_scene()
    return sb, pc.arm(sb)


def test_self_model_of_the_franka():
    sb, robot = _robot()
    probes, links = robot.collision_spheres()
    allp, alll, n_extra, mask = robot.self_collision_model(spacing=pc.SPACING)
    N = len(links)
    assert allp.dtype == np.float32 and alll.dtype == np.int32 and mask.dtype == np.uint32 and mask.shape == (32,)
    assert len(allp) == N + n_extra and n_extra > 0
    assert np.array_equal(allp[:N], probes) and np.array_equal(alll[:N], links), "the first N spheres are collision_spheres() unchanged"
    covered = set(robot._covered_links())
    assert all(int(b) not in covered and int(b) in robot.link_idx for b in alll[N:]), "extras ride on the links collision_spheres() leaves out"
    assert set(int(b) for b in alll[N:]) == {sb.body_index("link0")}
    bits = np.array([[(int(mask[a]) >> b) & 1 for b in range(32)] for a in range(32)])
    assert np.array_equal(bits, bits.T) and not bits.diagonal().any()
    for b in robot.link_idx:
        assert not bits[b, sb.bodies[b]["parent"]], "no parent / child pair"
    assert not bits[[i for i in range(32) if i not in robot.link_idx]].any()
    # no enabled pair overlaps at the neutral configuration, every disabled pair that is neither the same link nor parent / child does
    poses, qrot = robot._neutral_poses()
    centre = np.stack([poses[int(b)][0] + qrot(poses[int(b)][1], p[:3].astype(float)) for p, b in zip(allp, alll)])
    gap = np.linalg.norm(centre[:, None] - centre[None], axis=2) - allp[:, 3][:, None] - allp[:, 3][None]
    names = [b["name"] for b in sb.bodies]
    off = []
    for i, a in enumerate(robot.link_idx):
        for b in robot.link_idx[i + 1:]:
            lowest = gap[np.ix_(alll == a, alll == b)].min()
            related = sb.bodies[b]["parent"] == a or sb.bodies[a]["parent"] == b
            assert bits[a, b] == (not related and lowest >= 0.0), (names[a], names[b], lowest)
            if not bits[a, b] and not related:
                off.append((names[a], names[b]))
    pairs = robot.self_collision_pairs()
    assert all(bits[robot.link_idx[i], robot.link_idx[j]] and i < j for i, j in pairs)
    n_links = len(robot.link_idx)
    print(f"\n[self model] N = {N}, E = {n_extra}; {len(pairs)} of {n_links * (n_links - 1) // 2} link pairs enabled; overlapping at neutral: {off}")
    assert len(pairs) == bits.sum() // 2
    assert sorted(off) == sorted([("link5", "link7"), ("link5", "hand"), ("left_finger", "right_finger")])
    # another neutral configuration is another mask; the cache holds the arguments given last; set_collision_spheres drops it
    bent = robot.self_collision_model(neutral_qpos=sc.deepest("fold", 0).astype(float), spacing=pc.SPACING)[3]
    assert not np.array_equal(bent, mask) and np.array_equal(robot.self_collision_model()[3], bent)
    robot.set_collision_spheres(probes, links)
    assert "_self_model" not in robot.__dict__
    fine = robot.self_collision_model()
    assert fine[2] > 0 and fine[2] != n_extra and len(fine[0]) == N + fine[2], "without a spacing the base gets the default model of its geoms"


def test_set_self_collision_pairs_round_trip():
    sb, robot = _robot()
    robot.self_collision_model(spacing=pc.SPACING)
    before = robot.self_collision_pairs()
    hand, link0, link2 = (robot.link_idx.index(sb.body_index(n)) for n in ("hand", "link0", "link2"))   # (local link indices)
    assert (link0, hand) in before and link0 == 0
    robot.set_self_collision_pairs(disable=[("hand", "link0"), (robot.get_link("link2"), 0)])   # names, a LinkView, a local index
    after = robot.self_collision_pairs()
    assert sorted(set(before) - set(after)) == sorted([(link0, hand), (link0, link2)])
    robot.set_self_collision_pairs(pairs=[("link0", "hand")])
    assert robot.self_collision_pairs() == [(link0, hand)]
    mask = robot.self_collision_model()[3]
    b0, bh = sb.body_index("link0"), sb.body_index("hand")
    assert int(mask[b0]) == 1 << bh and int(mask[bh]) == 1 << b0 and int(mask.astype(np.uint64).sum()) == (1 << bh) + (1 << b0)
    robot.set_self_collision_pairs(pairs=before)
    assert robot.self_collision_pairs() == before
    robot.set_self_collision_pairs(pairs=[])
    assert not robot.self_collision_model()[3].any()
    with pytest.raises(ValueError):
        robot.set_self_collision_pairs(pairs=[("hand", "hand")])
    with pytest.raises(ValueError):
        robot.set_self_collision_pairs(pairs=[("hand", "cube")])


def test_struct_mirror():
    q = S.make_self_query([0] * 32)
    assert C.sizeof(S.MirSelfQuery) == 20 + 4 * 32 == q.struct_size and S.MirSelfQuery.link_mask.offset == 20
    assert S.PLAN_STATUS[7:] == ("START_IN_SELF_COLLISION", "GOAL_IN_SELF_COLLISION") and S.PLAN_STATUS[:7] == (
        "OK", "GOAL_OUT_OF_LIMITS", "START_IN_COLLISION", "GOAL_IN_COLLISION", "NODE_LIMIT", "ITERATION_LIMIT", "PATH_TOO_LONG")
    assert (S.PLAN_START_IN_SELF_COLLISION, S.PLAN_GOAL_IN_SELF_COLLISION) == (7, 8)
    q = S.make_self_query(np.arange(32, dtype=np.uint32), n_extra=3, self_margin=0.01, max_distance=0.5)
    assert list(q.link_mask) == list(range(32)) and q.n_extra == 3 and q.flags == 0 and abs(q.self_margin - 0.01) < 1e-9
    with pytest.raises(ValueError):
        S.make_self_query([0] * 31)
    if os.path.exists(LIB_PATH):
        lib = C.CDLL(LIB_PATH)
        lib.mir_self_query_sizeof.restype = C.c_int
        assert lib.mir_self_query_sizeof() == C.sizeof(S.MirSelfQuery)


class _StubScene:
    """what EntityView asks of a scene for the self-collision calls (argument handling only)"""
    num_envs, device, nq = sc.B, torch.device("cpu"), 16

    def __init__(self):
        self.calls = []
        self.q = torch.zeros((sc.B, 16))

    def get_state(self):
        return (self.q, None, None, None)

    def self_distance(self, probes, **kw):
        self.calls.append(("self", dict(kw, probes=probes)))
        R = self.num_envs if kw["env_idx"] is None else len(kw["env_idx"])
        pair = torch.tensor([[3, 60]] * (R - 1) + [[-1, -1]], dtype=torch.int32)
        return {"distance": torch.zeros((R, len(probes))), "row_min": torch.tensor([-0.02] * (R - 1) + [1.0]), "row_pair": pair}

    def plan_path(self, **kw):
        self.calls.append(("plan", kw))
        R, W, D = kw["qpos_goal"].shape[0], kw["num_waypoints"], len(kw["dof_qadr"])
        return {"path": torch.zeros((R, W, D)), "status": torch.tensor([0] * (R - 1) + [7], dtype=torch.int32), "poly": torch.zeros((R, 128, D)),
                "n_poly": torch.ones(R, dtype=torch.int32), "stats": torch.zeros((R, 4), dtype=torch.int32)}

    def path_clearance(self, **kw):
        self.calls.append(("clearance", kw))
        R, K = kw["paths"].shape[:2]
        out = {"seg_min": torch.zeros((R, K - 1)), "row_min": torch.tensor([0.05] * R), "row_first_blocked": torch.full((R,), -1, dtype=torch.int32)}
        if "self_model" in kw:
            out.update(seg_self_min=torch.zeros((R, K - 1)), row_self_min=torch.tensor([0.03] * (R - 1) + [0.004]))
        return out


def test_entity_view_argument_handling_and_refusals():
    c = sc.case("fold")
    st = _StubScene()
    robot = sc.arm(c, st)
    N, E = len(c["links"]) - c["n_extra"], c["n_extra"]
    clear = robot.get_self_clearance()
    kind, kw = st.calls[-1]
    assert kind == "self" and clear.tolist() == pytest.approx([-0.02] * (sc.B - 1) + [1.0])
    assert kw["probes"].shape == (N + E, 4) and len(kw["links"]) == N + E and kw["n_extra"] == E and np.array_equal(kw["link_mask"], c["mask"])
    assert kw["env_idx"] is None and kw["max_distance"] == 1.0 and kw["row_min"] and "qpos" not in kw
    det = robot.get_self_clearance(qpos=torch.as_tensor(c["start"][:2]), envs_idx=[4, 0], return_detail=True)
    kind, kw = st.calls[-1]
    assert kw["qpos"].shape == (2, 16) and kw["env_idx"].tolist() == [4, 0]
    assert sorted(det) == ["clearance", "links", "spheres"] and det["spheres"].tolist() == [[3, 60], [-1, -1]]
    assert det["links"].tolist() == [[int(c["links"][3]), int(c["links"][60])], [-1, -1]]
    assert robot.in_self_collision().tolist() == [True] * (sc.B - 1) + [False]
    assert robot.in_self_collision(margin=0.6).tolist() == [True] * (sc.B - 1) + [False] and st.calls[-1][1]["max_distance"] == 1.2
    # plan_path / get_path_clearance: off by default (the scene's option is 0), on by argument or by the option
    goal = torch.as_tensor(c["goal"])
    robot.plan_path(goal)
    assert "self_model" not in st.calls[-1][1] and len(st.calls[-1][1]["links"]) == N
    det = robot.plan_path(goal, self_collision=True, self_margin=0.6, return_detail=True)
    kw = st.calls[-1][1]
    assert len(kw["links"]) == N + E and kw["probes"].shape == (N + E, 4) and det["status"].tolist()[-1] == 7 and not det["valid"][-1]
    assert kw["self_model"]["n_extra"] == E and kw["self_model"]["self_margin"] == 0.6 and kw["self_model"]["max_distance"] == 1.2
    assert np.array_equal(kw["self_model"]["link_mask"], c["mask"])
    path = torch.zeros((4, sc.B, 9))
    plain = robot.get_path_clearance(path)
    assert "self_model" not in st.calls[-1][1] and plain.tolist() == pytest.approx([0.05] * sc.B)
    both = robot.get_path_clearance(path, margin=0.01, self_collision=True, self_margin=0.005)
    assert both.tolist() == pytest.approx([0.035] * (sc.B - 1) + [0.009]), "min(clearance - margin, self_clearance - self_margin) + margin"
    assert robot.path_in_collision(path, margin=0.01, self_collision=True, self_margin=0.005).tolist() == [False] * (sc.B - 1) + [True]
    det = robot.get_path_clearance(path, self_collision=True, return_detail=True)
    assert sorted(det) == ["clearance", "first_blocked", "seg_min", "self_clearance", "self_seg_min"]
    c["sb"].opt["enable_self_collision"] = 1
    try:
        robot.plan_path(goal)
        assert "self_model" in st.calls[-1][1]
        robot.plan_path(goal, self_collision=False)
        assert "self_model" not in st.calls[-1][1]
    finally:
        c["sb"].opt["enable_self_collision"] = 0
    with pytest.raises(ValueError):
        robot.plan_path(goal, self_collision=True, self_margin=-0.1)
    with pytest.raises(ValueError):
        robot.self_collision_model(neutral_qpos=np.zeros(7))

    # a scene without the entry point
    class Old:
        num_envs, device, nq = sc.B, torch.device("cpu"), 16
        plan_path, path_clearance, get_state = _StubScene.plan_path, _StubScene.path_clearance, _StubScene.get_state

        def __init__(self):
            self.calls, self.q = [], torch.zeros((sc.B, 16))

    old = sc.arm(c, Old())
    for call in (lambda: old.get_self_clearance(), lambda: old.in_self_collision(), lambda: old.plan_path(goal, self_collision=True),
                 lambda: old.get_path_clearance(path, self_collision=True)):
        with pytest.raises(NotImplementedError, match="no self-collision queries"):
            call()
    assert old.plan_path(goal).shape == (100, sc.B, 9)
    # an entity without spheres on moving links
    cube = EntityView(st, c["sb"], "cube", ())
    assert cube.self_collision_model()[2] == 0 and not cube.self_collision_model()[3].any()


@pytest.mark.parametrize("name", CASES)
def test_the_cases_are_fair(name):
    """what tests/test_gpu_self.py leans on, for every row, in float64"""
    c = sc.case(name)
    pb = sc.problem(name)
    print()
    for r in range(sc.B):
        pb.set_row(c["q"][r])
        v = np.array([pb.both(q) for q in sc.straight(name, r)], np.float64)
        print(f"[self, {name}] row {r}: ends scene {v[0, 0]:.4f} / {v[-1, 0]:.4f} self {v[0, 1]:.4f} / {v[-1, 1]:.4f}; straight edge scene {v[:, 0].min():.4f} "
              f"self {v[:, 1].min():.4f}")
        assert min(v[0].min(), v[-1].min()) >= 0.02, "both ends keep 2 cm from the scene and from the arm"
        assert v[:, 0].min() >= 0.02 and v[:, 1].min() <= -0.01, "the straight edge is clear of the scene and 1 cm into the arm"
        assert pb.both(sc.deepest(name, r).astype(np.float64))[1] <= -0.01
    for seed in range(3):
        for r in range(sc.B):
            for dtname in ("float64", "float32"):
                ref = sc.reference(name, r, seed, dtname)
                assert ref["status"] == plan_ref.OK and len(ref["poly"]) >= 3, (name, seed, r, dtname, ref["status"])
                assert ref["iterations"] <= sc.BUDGET["max_iterations"] // 4 and max(ref["nodes"]) <= sc.BUDGET["max_nodes"] // 2, (ref["iterations"], ref["nodes"])
                seg, seg_self, _ = self_ref.polyline_clearances(pb, c["q"][r], np.asarray(ref["poly"], np.float64), sc.RESOLUTION)
                assert seg.min() >= sc.MARGIN - (1e-5 if dtname == "float32" else 0.0), "the scene test of the float64 validator"
                assert seg_self.min() >= sc.SELF_MARGIN - (1e-5 if dtname == "float32" else 0.0), "the self test of the float64 validator"
            ref = sc.reference(name, r, seed)
            print(f"[self, {name}] seed {seed} row {r}: iterations {ref['iterations']} nodes {ref['nodes']} polyline {len(ref['poly'])} checked {ref['checked']}")


def test_status_precedence():
    """for one configuration the scene test decides first: 2 before 7, 3 before 8"""
    c = sc.case("fold")
    kw = dict(W=4, max_nodes=8, max_iterations=0, smooth_passes=0, resolution=sc.RESOLUTION, step=sc.STEP)
    deep = sc.deepest("fold", 0)
    q_self = c["q"][0].copy()
    q_self[c["qadr"]] = deep
    floor, both = np.array(sc.IN_GROUND, np.float32), np.array(sc.IN_BOTH, np.float32)
    q_floor, q_both = c["q"][0].copy(), c["q"][0].copy()
    q_floor[c["qadr"]], q_both[c["qadr"]] = floor, both
    pb = sc.problem("fold")
    pb.set_row(c["q"][0])
    values = {k: pb.both(q.astype(np.float64)) for k, q in (("deep", deep), ("floor", floor), ("both", both))}
    print(f"\n[self, statuses] (scene, self) of the three configurations: {values}")
    assert values["deep"][0] >= 0.02 and values["deep"][1] <= -0.01
    assert values["floor"][0] <= -0.01 and values["floor"][1] >= 0.02
    assert values["both"][0] <= -0.01 and values["both"][1] <= -0.01
    plan = lambda q, g: self_ref.plan(sc.problem("fold"), q, g, 0, **kw)["status"]  # noqa: E731
    assert plan(q_self, c["goal"][0]) == self_ref.START_IN_SELF_COLLISION == 7
    assert plan(c["q"][0], deep) == self_ref.GOAL_IN_SELF_COLLISION == 8
    assert plan(q_floor, c["goal"][0]) == plan_ref.START_IN_COLLISION and plan(c["q"][0], floor) == plan_ref.GOAL_IN_COLLISION
    assert plan(q_both, c["goal"][0]) == plan_ref.START_IN_COLLISION == 2, "2 before 7"
    assert plan(c["q"][0], both) == plan_ref.GOAL_IN_COLLISION == 3, "3 before 8"
    assert plan(q_self, floor) == 7 and plan(q_floor, deep) == 2, "the start is judged before the goal"


def test_self_distance_reference_is_rarely_ambiguous():
    """the GPU tier compares `other` wherever the runner-up partner is more than 1e-4 m behind: at most 5 % of the probes may be left out"""
    for name in CASES:
        c = sc.case(name)
        pb = sc.problem(name)
        for r in range(sc.B):
            for qp in (None, sc.deepest(name, r).astype(np.float64)):
                dist, other, row_min, pair, runner, _ = self_ref.self_distance(pb, c["q"][r], qp)
                share = float(((runner <= 1e-4) & (other >= 0)).mean())
                assert share <= 0.05, (name, r, share)
                assert (other >= 0).all() and pair[0] < pair[1] and dist[pair[0]] == row_min == dist.min()
                assert (row_min < -0.01) == (qp is not None)
