"""The carried object on the CPU: the conditions the GPU tests of tests/test_gpu_carry.py lean on (tests/carry_cases.py), in the float64
reference of tests/carry_ref.py and its float32 port; the host-side composition of EntityView (carried_model, the default link filter,
the ValueErrors) and the layout of MirCarryQuery.  No GPU, no library call.
"""
import ctypes as C

import numpy as np
import pytest

import carry_cases as cc
import plan_ref
from gym_genesis.backend import spec as S
from gym_genesis.tasks.views import EntityView


@pytest.mark.parametrize("name", cc.NAMES)
def test_case_conditions(name):
    c = cc.case(name)
    pb, plain = cc.problem(name), cc.plain_problem(name)
    default = set(cc.views(name, c["sb"])[0].attached_links_default("hand"))
    print()
    for r in range(cc.B):
        pb.grasp = None
        pb.set_row(c["q"][r])
        plain.set_row(c["q"][r])
        assert np.abs(pb.grasp_used() - c["grasp"][r]).max() < 1e-6, "the start row holds the nominal grasp (to float32)"
        qs = cc.straight(name, r)
        both = np.array([pb.both(q) for q in qs])
        arm = np.array([plain.clearance(q) for q in qs])
        print(f"[{name}] row {r}: ends scene {both[0, 0]:.4f} {both[-1, 0]:.4f} carried-arm {both[0, 1]:.4f} {both[-1, 1]:.4f}; straight edge: scene "
              f"{both[:, 0].min():.4f} carried-arm {both[:, 1].min():.4f} arm alone {arm.min():.4f}")
        assert both[[0, -1]].min() >= 0.02, "start and goal are clear by 2 cm with the carried spheres"
        if name == "under":
            assert arm.min() >= 0.01 and both[:, 0].min() <= -0.01 and both[:, 1].min() >= 0.02
            ref = plan_ref.plan(plain, c["q"][r], c["goal"][r], r, W=cc.BUDGET["W"], resolution=cc.RESOLUTION, step=cc.STEP)
            assert ref["status"] == plan_ref.OK and len(ref["poly"]) == 2, "the plain planner returns the straight line"
        else:
            assert arm.min() >= 0.02 and both[:, 0].min() >= 0.02 and both[:, 1].min() <= -0.01
            deep = qs[int(both[:, 1].argmin())]
            best, other = pb.self_distances(pb.centres(deep))
            i = int(best.argmin())
            pair = {int(pb.links[i]), int(pb.links[other[i]])}
            assert c["body"] in pair and (pair - {c["body"]}) <= default, pair


@pytest.mark.parametrize("dtname", ("float64", "float32"))
@pytest.mark.parametrize("name", cc.NAMES)
def test_every_row_finds_a_plan(name, dtname):
    c = cc.case(name)
    for r in range(cc.B):
        out = cc.reference(name, r, 0, dtname)
        assert out["status"] == plan_ref.OK and len(out["poly"]) >= 3, (name, dtname, r, out["status"], out["iterations"], out["nodes"])
        assert out["iterations"] <= cc.BUDGET["max_iterations"] and max(out["nodes"]) <= cc.BUDGET["max_nodes"]
        ok, scene, own, _ = cc.valid_polyline(name, r, out["poly"], tol=1e-5 if dtname == "float32" else 0.0)
        assert ok, (name, dtname, r, scene, own)
        # the straight line the plain planner returns fails the same validator
        assert not cc.valid_polyline(name, r, np.stack([c["start"][r], c["goal"][r]]))[0]


def test_grasp_given_and_blocked_rows():
    name = "under"
    c = cc.case(name)
    for dt in (np.float64, np.float32):
        pb = cc.problem(name, dt)
        pb.grasp = None
        pb.set_row(c["q"][1])
        from_row, v0 = pb.grasp_used(), pb.both(c["start"][1].astype(dt))
        pb.grasp = np.concatenate([c["grasp"][1, :3], 3.0 * c["grasp"][1, 3:]])   # (the quaternion is normalised)
        pb.set_row(c["q"][1])
        assert np.abs(pb.grasp_used() - c["grasp"][1]).max() < 1e-6 and np.abs(pb.grasp_used() - from_row).max() < 1e-6
        assert abs(float(pb.both(c["start"][1].astype(dt))[0]) - float(v0[0])) < 1e-6
        for bad in (np.array([0, 0, 0.1, 0, 0, 0, 0.0]), np.array([np.nan, 0, 0.1, 1, 0, 0, 0.0]), np.array([0, 0, 0.1, 1, np.inf, 0, 0.0])):
            pb.grasp = bad
            pb.set_row(c["q"][1])
            assert pb.blocked and np.isneginf(pb.both(c["start"][1].astype(dt))).all()
            out = cc.carry_ref.self_ref.plan(pb, c["q"][1], c["goal"][1], 1, W=4, max_nodes=8, max_iterations=4, resolution=cc.RESOLUTION, step=cc.STEP)
            assert out["status"] == plan_ref.START_IN_COLLISION


def test_default_link_filter_and_composition():
    name = "under"
    c = cc.case(name)
    sb = c["sb"]
    robot, cube, _ = cc.views(name, sb)
    body = sb.body_index
    carrying = sorted(set(int(b) for b in robot.self_collision_model()[1]))
    out = {body("hand"), body("left_finger"), body("right_finger"), body("link7")}
    assert out <= set(carrying), "the excluded links do carry spheres"
    assert robot.attached_links_default("hand") == [b for b in carrying if b not in out]
    assert body("link0") in robot.attached_links_default("hand"), "the bolted base is tested through its extra spheres"
    probes, links, n_extra, mask, Cb, Lk = robot.carried_model(cube, "hand", self_collision=False)
    arm_p, arm_l, arm_e, arm_mask = robot.self_collision_model()
    N, n_c = len(arm_l) - arm_e, len(cube.collision_spheres()[1])
    assert (Cb, Lk, n_extra) == (body("cube"), body("hand"), arm_e) and len(links) == len(arm_l) + n_c
    assert np.array_equal(probes[:N], arm_p[:N]) and np.array_equal(probes[N + n_c:], arm_p[N:]) and (links[N:N + n_c] == Cb).all()
    assert np.array_equal(probes[N:N + n_c], cube.collision_spheres()[0])
    want = sum(1 << b for b in carrying if b not in out)
    assert int(mask[Cb]) == want and all(int(mask[b]) == ((1 << Cb) if (want >> b) & 1 else 0) for b in range(32) if b != Cb), "only the C rows and columns"
    # arm against arm on: the arm's filter plus the same C rows and columns
    both = robot.carried_model(cube, "hand", self_collision=True)[3]
    assert int(both[Cb]) == want and all(int(both[b]) == int(arm_mask[b]) | ((1 << Cb) if (want >> b) & 1 else 0) for b in range(32) if b != Cb)
    # attached_links=[]: an empty C row (and no C column)
    none = robot.carried_model(cube, "hand", attached_links=[], self_collision=False)[3]
    assert not none.any()
    some = robot.carried_model(cube, "hand", attached_links=["link5", robot.get_link("link2")], self_collision=False)[3]
    assert int(some[Cb]) == (1 << body("link5")) | (1 << body("link2"))
    # what set_collision_spheres() put in place of the cube's own model
    fine = EntityView(None, sb, "cube", ())
    fine.set_collision_spheres(*fine.collision_spheres(spacing=0.02))
    assert len(fine.collision_spheres()[1]) == 8 and len(robot.carried_model(fine, "hand")[1]) == len(arm_l) + 8


def test_value_errors():
    name = "rod"
    sb = cc.case(name)["sb"]
    robot, rod, cube = cc.views(name, sb)
    with pytest.raises(ValueError, match="ee_link_name"):
        robot.carried_model(rod, None)
    with pytest.raises(ValueError, match="free body"):
        robot.carried_model(robot, "hand")                                   # articulated
    with pytest.raises(ValueError, match="free body"):
        robot.carried_model(EntityView(None, sb, "hand", ()), "link7")       # a fixed link with children
    with pytest.raises(ValueError, match="free body"):
        robot.carried_model("cube", "hand")
    with pytest.raises(ValueError, match="not a link of this entity"):
        robot.carried_model(rod, "cube")
    with pytest.raises(ValueError, match="does not belong"):
        robot.carried_model(rod, "hand", attached_links=[cube.get_link("cube")])

    class FakeScene:   # (enough of MirScene for the argument checks, which come before any launch)
        device, num_envs, plan_path, self_distance = "cpu", cc.B, True, True

    robot, rod, cube = cc.views(name, sb, FakeScene())
    for shape in ((7, 1), (cc.B, 6), (cc.B + 1, 7), (8,)):
        with pytest.raises(ValueError, match="grasp_pose"):
            robot._plan_args(None, None, None, (), "plan_path", False, 0.0, rod, "hand", np.zeros(shape), None)
    with pytest.raises(ValueError, match="ee_link_name"):
        robot._plan_args(None, None, None, (), "plan_path", False, 0.0, rod, None, None, None)
    with pytest.raises(ValueError, match="attached_entity"):
        robot._plan_args(None, None, None, (), "plan_path", False, 0.0, None, "hand", None, None)
    args, R = robot._plan_args(None, None, None, (cube,), "plan_path", False, 0.0, rod, "hand", np.array([0, 0, 0.1, 1, 0, 0, 0.0]), None)
    assert R == cc.B and tuple(args["carry"]["grasp"].shape) == (cc.B, 7) and args["carry"]["body"] == sb.body_index("rod")
    assert args["skip_geoms"] == cc.case(name)["skip"] and args["self_model"]["n_extra"] == cc.case(name)["n_extra"]


def test_carry_query_layout():
    q = S.make_carry_query(12, 9)
    assert C.sizeof(S.MirCarryQuery) == 16 and q.struct_size == 16 and (q.body, q.link, q.flags) == (12, 9, 0)
    assert [(n, getattr(S.MirCarryQuery, n).offset) for n, _ in S.MirCarryQuery._fields_] == [("struct_size", 0), ("body", 4), ("link", 8), ("flags", 12)]
    assert bytes(q) == np.array([16, 12, 9, 0], np.int32).tobytes()
