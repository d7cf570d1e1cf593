"""Certified swept clearance with the self test and a carried object on the GPU (include/mirigid.h: mir_certify_path_self,
mir_certify_path_carry; backend/lib.py: MirScene.certify_path(self_model=, carry=, grasp=); tasks/views.py: EntityView.certify_sweep,
sweep_is_certified_clear).

The cases -- scenes, start rows, models, paths -- are those of tests/certrel_cases.py; tests/test_certrel_cpu.py holds the conditions that
make the comparisons below fair.  States are SET.  R = 5, K <= 3, 57 + 8 spheres (+ 1 thin, + the carried body's), and all five rows are
judged in every case.

The GPU is judged on its OWN leaves, as tests/test_gpu_cert.py does: which leaves a float32 run accepts may differ from the float64
reference's wherever a test is decided within rounding, and every such tree is a valid run of the rule.
a. With max_leaves large enough: the leaves of every finished segment tile [0, 1]; replayed in float64 on those leaves
   (certrel_ref.replay), seg_lower / seg_self_lower are the minima of lo / lo_s over the leaves, seg_upper / seg_self_upper the minima of
   u / u_s over every node the rule evaluates for that tree and the endpoints, and every leaf's acceptance test holds -- within tol32.
b. lower <= the dense float64 minimum (2048 samples per segment) + tol32, for both brackets, on every segment of every case.
c. Statuses: self_clear, carry_clear, carry_given all CLEAR; self_thin and carry_arm BLOCKED through self_upper while the scene bracket
   stays clear; carry_under BLOCKED through upper; common in three evaluations; budget, depth, nan and a NaN grasp as the rule says.
   common's "self_lower == self_upper - guard to the bit" is asserted on common_capped (self_max = 2^-5, below every pair distance, so
   the three evaluations return one number); uncapped, the three float32 evaluations of a distance that does not change differ by their
   own rounding (1.5e-8 m measured on an MI355X) and the difference is asserted within tol32.  Both calls take three evaluations, which a
   wrong LCA or the naive v_i + v_j cannot.
d. self_thin and carry_arm through the entity view: the sampled check at resolution 0.1 passes with >= 1 mm, certify_sweep is BLOCKED --
   what the feature buys.
e. Identities with mir_certify_path, byte for byte; a given grasp against the one taken from the start row.
f. Invisibility and addressing: env_idx with repeats; one launch of R rows against R launches of one; state, state version and a
   following step bit-identical with a call in between; a refusal writes no output byte and is refused inside an open step.
g. BRACKET on self_clear: both brackets <= tol + tol32.
Yardstick, the project's rule: tol32 = 4 x max(float32 port against float64 on the same leaves, 2^-23 x L), printed before it is used.
L: the largest magnitude entering a bound -- the largest |coordinate| of a sphere centre plus the largest hw v_i or hw v_ij.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import carry_cases
import cert_ref
import certrel_cases as rc
import certrel_ref
import plan_cases as pc
import self_cases
from gym_genesis.backend import spec as S

pytestmark = pytest.mark.gpu

B = rc.B
MAX_LEAVES = 512
_scenes, _at = {}, {}
SCENE_KEYS = ("seg_lower", "seg_upper", "row_lower", "row_upper", "stats", "leaves")


def _scene(name):
    """one scene per kind of case ("self", "under", "rod"), at the start rows of the case asked for"""
    from gym_genesis.backend.lib import MirScene

    c = rc.case(name)
    kind = c["kind"]
    if kind not in _scenes:
        _scenes[kind] = MirScene(c["spec"], B)
    sc = _scenes[kind]
    if _at.get(kind) != c["q"].tobytes():
        sc.set_state(qpos=c["q"], qvel=np.zeros((B, sc.nv), np.float32))
        _at[kind] = c["q"].tobytes()
    return sc


def _models(c, sc=None):
    kw = {}
    if c["mask"] is not None:
        kw["self_model"] = dict(link_mask=c["mask"], n_extra=c["n_extra"], self_margin=c["self_margin"], max_distance=c["self_max"])
    if c["carry"] is not None:
        g = None if c["grasp"] is None or sc is None else torch.as_tensor(c["grasp"], device=sc.device)
        kw["carry"] = dict(body=c["carry"][0], link=c["carry"][1], grasp=g)
    return kw


def _args(name, sc=None):
    c = rc.case(name)
    return c, dict(probes=c["probes"], links=c["links"], dof_qadr=c["qadr"], skip_geoms=c["skip"], max_distance=c["max_distance"],
                   max_leaves=MAX_LEAVES, **c["par"], **_models(c, sc))


def _call(name, rows=None, **over):
    """the case through MirScene.certify_path (rows: env indices, the paths and grasps of those rows) -> numpy arrays"""
    sc = _scene(name)
    c, kw = _args(name, sc)
    kw.update(over)
    paths = c["paths"]
    if rows is not None:
        rows = np.asarray(rows)
        paths = paths[rows]
        kw["env_idx"] = torch.as_tensor(rows, device=sc.device)
        if "carry" in kw and kw["carry"]["grasp"] is not None:
            kw["carry"] = {**kw["carry"], "grasp": kw["carry"]["grasp"][torch.as_tensor(rows, device=sc.device)]}
    return {k: v.cpu().numpy() for k, v in sc.certify_path(paths=paths, **kw).items()}


def _leaves(got, r, s):
    n = int(got["stats"][r, 1])
    assert n <= MAX_LEAVES, "the capacity of the test holds every leaf"
    lv = got["leaves"][r, :n]
    assert (got["leaves"][r, n:] == -1).all(), "entries behind the count are not written"
    return [(int(l), int(k)) for (ss, l, k) in lv if ss == s]


def _judge(name, got, bracket=False):
    """a. and b. on every row and segment of a result -> the largest tol32 used"""
    c = rc.case(name)
    par, on = c["par"], rc.self_on(name)
    margin, smargin, tol, guard = float(np.float32(par["margin"])), float(np.float32(c["self_margin"])), float(np.float32(par["tol"])), par["guard"]
    worst_tol, worst = 0.0, dict(lower=0.0, upper=0.0, self_lower=0.0, self_upper=0.0)
    for r in range(B):
        finite_row = not (name == "nan_grasp" and r == 2)
        dense = rc.dense(name, r)
        finished = 0
        assert int(got["row_status"][r]) == int(got["seg_status"][r].max())
        notclear = np.flatnonzero(got["seg_status"][r] != 0)
        assert int(got["row_first"][r]) == (int(notclear[0]) if len(notclear) else -1)
        for a, b in (("row_lower", "seg_lower"), ("row_upper", "seg_upper"), ("row_self_lower", "seg_self_lower"), ("row_self_upper", "seg_self_upper")):
            assert float(got[a][r]) == float(got[b][r].min()), (name, r, a)
        p64, p32 = rc.row_problem(name, r), rc.row_problem(name, r, "float32")
        for s in range(c["paths"].shape[1] - 1):
            st = int(got["seg_status"][r, s])
            lo, up = float(got["seg_lower"][r, s]), float(got["seg_upper"][r, s])
            lo_s, up_s = float(got["seg_self_lower"][r, s]), float(got["seg_self_upper"][r, s])
            lv = _leaves(got, r, s)
            tol32 = 4.0 * 2.0 ** -23 * 2.0
            if st in (S.CERT_CLEAR, S.CERT_UNDECIDED, S.CERT_DEPTH) or (st == S.CERT_BLOCKED and bracket):
                finished += 1
                assert cert_ref.tiles(lv), (name, r, s, lv)
                n64 = certrel_ref.replay(p64, c["q"][r], c["paths"][r], s, lv, guard, on)
                n32 = certrel_ref.replay(p32, c["q"][r], c["paths"][r], s, lv, guard, on)
                keys = ("lo", "u", "lo_s", "us") if on else ("lo", "u")
                err = max(abs(float(x[k]) - float(y[k])) for x, y in zip(n64, n32) for k in keys)
                L = max(x["L"] + x["reach"] for x in n64)
                tol32 = 4.0 * max(err, 2.0 ** -23 * L)
                lo64, up64 = min(float(x["lo"]) for x in n64 if x["leaf"]), float(n64[-1]["upper"])
                worst["lower"], worst["upper"] = max(worst["lower"], abs(lo - lo64)), max(worst["upper"], abs(up - up64))
                assert abs(lo - lo64) <= tol32 and abs(up - up64) <= tol32, (name, r, s, lo, lo64, up, up64, tol32)
                if on:
                    los64, ups64 = min(float(x["lo_s"]) for x in n64 if x["leaf"]), float(n64[-1]["upper_s"])
                    worst["self_lower"], worst["self_upper"] = max(worst["self_lower"], abs(lo_s - los64)), max(worst["self_upper"], abs(up_s - ups64))
                    assert abs(lo_s - los64) <= tol32 and abs(up_s - ups64) <= tol32, (name, r, s, lo_s, los64, up_s, ups64, tol32)
                for x in n64:
                    if x["leaf"]:
                        held = (not bracket and x["lo"] >= margin - tol32) or x["lo"] >= x["upper"] - tol - tol32
                        if on:
                            held = held and ((not bracket and x["lo_s"] >= smargin - tol32) or x["lo_s"] >= x["upper_s"] - tol - tol32)
                        assert held or x["l"] == par["max_depth"], (name, r, s, x)
                    assert x["l"] <= par["max_depth"]
                if st == S.CERT_CLEAR:
                    assert lo >= margin and (not on or lo_s >= smargin)
                if st in (S.CERT_CLEAR, S.CERT_UNDECIDED):
                    assert lo >= margin or up - lo <= tol + tol32
                    assert not on or lo_s >= smargin or up_s - lo_s <= tol + tol32
            worst_tol = max(worst_tol, tol32)
            if finite_row:
                assert lo <= dense[0][s] + tol32, (name, r, s, lo, dense[0][s])   # b.
                assert not on or lo_s <= dense[1][s] + tol32, (name, r, s, lo_s, dense[1][s])
        assert int(got["stats"][r, 3]) == finished, (name, r, got["stats"][r], finished)
    print(f"\n[certify sweep, {name}{' bracket' if bracket else ''}] against float64 on the GPU's own leaves: lower {worst['lower']:.3e} upper "
          f"{worst['upper']:.3e} self_lower {worst['self_lower']:.3e} self_upper {worst['self_upper']:.3e}, largest tol32 {worst_tol:.3e}; "
          f"evaluations {got['stats'][:, 0]}, leaves {got['stats'][:, 1]}, deepest {got['stats'][:, 2]}")
    return worst_tol


@pytest.mark.parametrize("name", rc.NAMES)
def test_bounds_on_the_gpus_own_leaves(name):
    """a., b. and c."""
    got = _call(name)
    tol32 = _judge(name, got)
    st = got["seg_status"]
    guard = np.float32(rc.GUARD)
    if name in ("self_clear", "carry_clear", "carry_given"):
        assert (st == S.CERT_CLEAR).all() and (got["row_first"] == -1).all() and (got["seg_lower"] >= 0.0).all() and (got["seg_self_lower"] >= 0.0).all(), st
    elif name in ("self_thin", "carry_arm"):
        assert (st == S.CERT_BLOCKED).all() and (got["seg_self_upper"] < 0.0).all() and (got["row_first"] == 0).all(), (st, got["seg_self_upper"])
        assert (got["seg_upper"] >= 0.1).all(), "the scene bracket stays clear: the self test is what blocks"
        assert (got["row_self_upper"] <= -1e-3 + tol32).all(), got["row_self_upper"]
    elif name == "carry_under":
        assert (st == S.CERT_BLOCKED).all() and (got["seg_upper"] < 0.0).all() and (got["seg_self_upper"] > 0.1).all(), (st, got["seg_upper"])
    elif name in ("common", "common_capped"):
        assert (got["stats"][:, 0] == 3).all() and (got["stats"][:, 1] == 1).all() and (st == S.CERT_CLEAR).all(), got["stats"]
        want = (got["row_self_upper"].astype(np.float32) - guard).astype(np.float32)
        print(f"[certify sweep, {name}] self_lower - (self_upper - guard): {np.abs(got['row_self_lower'] - want).max():.3e}")
        if name == "common_capped":
            assert np.array_equal(got["row_self_lower"], want) and (got["row_self_upper"] == np.float32(rc.COMMON_CAP)).all(), "to the bit"
        else:   # (uncapped, the three evaluations of a distance that does not change differ by their own rounding)
            assert (np.abs(got["row_self_lower"] - want) <= tol32).all()
    elif name == "budget":
        assert (got["stats"][:, 0] == 8).all() and (st[:, 1] == S.CERT_BUDGET).all() and (st[:, 0] == S.CERT_CLEAR).all(), (st, got["stats"])
        assert np.isneginf(got["seg_lower"][:, 1]).all() and np.isneginf(got["seg_self_lower"][:, 1]).all()
        none = _call(name, max_evaluations=1)
        assert (none["seg_status"] == S.CERT_BUDGET).all() and np.isposinf(none["seg_self_upper"][:, 1]).all(), "upper keeps what was sampled"
        assert np.isfinite(none["seg_self_upper"][:, 0]).all() and np.isfinite(none["seg_upper"][:, 0]).all()
    elif name == "depth":
        assert (got["row_status"] == S.CERT_DEPTH).all() and (got["stats"][:, 2] == 2).all()
        assert ((st == S.CERT_DEPTH) | (st == S.CERT_CLEAR)).all()
    elif name == "nan":
        want = np.zeros_like(st)
        want[1, :] = S.CERT_NOT_FINITE
        assert np.array_equal(st, want), st
        for k in ("seg_lower", "seg_self_lower"):
            assert np.isneginf(got[k][1]).all()
        assert np.isposinf(got["seg_upper"][1]).all() and np.isposinf(got["seg_self_upper"][1]).all() and got["row_first"][1] == 0
        clean = _call("self_clear")
        keep = np.arange(B) != 1
        for k in ("seg_lower", "seg_self_lower", "seg_upper", "seg_self_upper"):
            assert np.array_equal(got[k][keep], clean[k][keep]), "the other rows are what they were"
    elif name == "nan_grasp":
        want = np.zeros_like(st)
        want[2, :] = S.CERT_NOT_FINITE
        assert np.array_equal(st, want), st
        assert np.isneginf(got["seg_lower"][2]).all() and np.isneginf(got["seg_self_lower"][2]).all() and (got["stats"][2] == 0).all()
        clean = _call("carry_given")
        keep = np.arange(B) != 2
        for k in ("seg_lower", "seg_self_lower", "seg_upper", "seg_self_upper", "grasp"):
            assert np.array_equal(got[k][keep], clean[k][keep]), "the other rows are what they were"


def test_bracket_mode_closes_both_brackets():
    """g."""
    got = _call("self_clear", bracket=True)
    tol32 = _judge("self_clear", got, bracket=True)
    assert (got["seg_status"] == S.CERT_CLEAR).all()
    assert (got["seg_upper"] - got["seg_lower"] <= np.float32(rc.TOL) + tol32).all(), got["seg_upper"] - got["seg_lower"]
    assert (got["seg_self_upper"] - got["seg_self_lower"] <= np.float32(rc.TOL) + tol32).all(), got["seg_self_upper"] - got["seg_self_lower"]
    plain = _call("self_clear")
    assert (got["stats"][:, 0] >= plain["stats"][:, 0]).all(), "closing every bracket costs at least what deciding the margin costs"


def _thin_robot(c, sc):
    robot = self_cases.arm(c, sc)
    robot._self_model = (c["probes"].copy(), c["links"].copy(), c["n_extra"], c["mask"].copy())   # (the thin sphere behind the derived model)
    robot.__dict__.pop("_self_dev", None)
    return robot


def test_self_thin_the_sampled_check_passes_and_the_certified_one_does_not():
    """d."""
    c, sc = rc.case("self_thin"), _scene("self_thin")
    robot = _thin_robot(c, sc)
    cube = carry_cases.EntityView(sc, c["sb"], "cube", ())
    path = torch.as_tensor(c["paths"], device=sc.device).permute(1, 0, 2)
    kw = dict(self_collision=True, ignore_entities=[cube])
    sampled = robot.path_in_collision(path, resolution=rc.THIN_RESOLUTION, **kw)
    assert sampled.shape == (B,) and not bool(sampled.any()), sampled
    low = robot.get_path_clearance(path, resolution=rc.THIN_RESOLUTION, return_detail=True, **kw)
    certified = robot.sweep_is_certified_clear(path, **kw)
    assert certified.shape == (B,) and not bool(certified.any()), certified
    det = robot.certify_sweep(path, return_detail=True, **kw)
    print(f"\n[certify sweep, self_thin] sampled self clearance at 0.1 {low['self_clearance'].cpu().numpy().round(5)}, certified self_upper "
          f"{det['self_upper'].cpu().numpy().round(5)}, scene upper {det['upper'].cpu().numpy().round(4)}")
    assert (low["self_clearance"] >= 1e-3).all() and (low["clearance"] >= 1e-3).all()
    assert (det["status"] == S.CERT_BLOCKED).all() and (det["self_upper"] < 0.0).all() and (det["upper"] > 0.0).all() and (det["first"] == 0).all()
    raw = _call("self_thin", max_leaves=0)
    assert np.array_equal(det["self_upper"].cpu().numpy(), raw["row_self_upper"]) and np.array_equal(det["status"].cpu().numpy(), raw["row_status"])


def test_carry_arm_the_sampled_check_passes_and_the_certified_one_does_not():
    """d."""
    c, sc = rc.case("carry_arm"), _scene("carry_arm")
    robot, rod, cube = carry_cases.views("rod", c["sb"], sc)
    path = torch.as_tensor(c["paths"], device=sc.device).permute(1, 0, 2)
    kw = dict(attached_entity=rod, ee_link_name="hand", self_collision=False, ignore_entities=[cube])
    sampled = robot.path_in_collision(path, resolution=rc.ARM_RESOLUTION, **kw)
    assert sampled.shape == (B,) and not bool(sampled.any()), sampled
    low = robot.get_path_clearance(path, resolution=rc.ARM_RESOLUTION, return_detail=True, **kw)
    det = robot.certify_sweep(path, return_detail=True, **kw)
    print(f"\n[certify sweep, carry_arm] sampled self clearance at 0.1 {low['self_clearance'].cpu().numpy().round(5)}, certified self_upper "
          f"{det['self_upper'].cpu().numpy().round(5)}, evaluations {det['stats'][:, 0].cpu().numpy()}")
    assert (low["self_clearance"] >= 1e-3).all() and (low["clearance"] >= 1e-3).all()
    assert (det["status"] == S.CERT_BLOCKED).all() and (det["self_upper"] < 0.0).all() and (det["upper"] > 0.0).all()
    assert not bool(robot.sweep_is_certified_clear(path, **kw).any())
    raw = _call("carry_arm", max_leaves=0)
    assert np.array_equal(det["self_upper"].cpu().numpy(), raw["row_self_upper"]) and np.array_equal(det["grasp"].cpu().numpy(), raw["grasp"])


def test_a_given_grasp_against_the_one_from_the_start_row():
    """e. grasp_used is what each row used; handed back as (R, 7) it gives the same bits when it comes out equal"""
    taken, given = _call("carry_clear"), _call("carry_given")
    c = rc.case("carry_clear")
    p64 = rc.row_problem("carry_clear", 0)
    for r in range(B):
        p64.grasp = None
        p64.set_row(c["q"][r])
        assert np.abs(taken["grasp"][r] - p64.grasp_used()).max() <= 4 * 2.0 ** -23 * 2.0, (r, taken["grasp"][r], p64.grasp_used())
    again = _call("carry_clear", carry=dict(body=c["carry"][0], link=c["carry"][1], grasp=torch.as_tensor(taken["grasp"], device=_scene("carry_clear").device)))
    same = np.array_equal(again["grasp"], taken["grasp"])
    print(f"\n[certify sweep, grasp] handed back, grasp_used differs by {np.abs(again['grasp'] - taken['grasp']).max():.3e}; the port's by "
          f"{np.abs(given['grasp'] - taken['grasp']).max():.3e}")
    assert np.array_equal(again["grasp"][:, :3], taken["grasp"][:, :3]), "a given position is used as it is"
    assert np.abs(again["grasp"] - taken["grasp"]).max() <= 2.0 ** -22
    if same:
        assert all(np.array_equal(again[k], taken[k]) for k in taken), "same grasp, same bits"
    assert np.array_equal(again["seg_status"], taken["seg_status"]) and np.array_equal(given["seg_status"], taken["seg_status"])
    for k in ("seg_lower", "seg_self_lower", "seg_upper", "seg_self_upper"):
        assert np.abs(again[k] - taken[k]).max() <= 1e-5 and np.abs(given[k] - taken[k]).max() <= 1e-5, k


def test_identities_with_the_scene_only_entry_point():
    """e. byte for byte against mir_certify_path: _carry without a self query and without a probe on the carried body; _self with an
    all-zero mask and no extra sphere (scene outputs, leaves, stats); the same on the budget, depth and nan inputs of tests/cert_cases.py,
    so that BUDGET, DEPTH and NOT_FINITE cross the three instantiations too"""
    zero = dict(link_mask=np.zeros(32, np.uint32), n_extra=0, self_margin=0.0, max_distance=1.0)
    for name in ("carry_under", "carry_clear"):
        c, sc = rc.case(name), _scene(name)
        n = c["n_arm"]
        kw = dict(probes=c["probes"][:n], links=c["links"][:n], dof_qadr=c["qadr"], skip_geoms=c["skip"], max_leaves=MAX_LEAVES, **c["par"])
        plain = {k: v.cpu().numpy() for k, v in sc.certify_path(paths=c["paths"], **kw).items()}
        carry = {k: v.cpu().numpy() for k, v in sc.certify_path(paths=c["paths"], carry=dict(body=c["carry"][0], link=c["carry"][1]), **kw).items()}
        for k in plain:
            assert carry[k].tobytes() == plain[k].tobytes(), (name, k)
        assert np.isposinf(carry["seg_self_lower"]).all() and np.isfinite(carry["grasp"]).all()
        own = {k: v.cpu().numpy() for k, v in sc.certify_path(paths=c["paths"], self_model=zero, **kw).items()}
        for k in SCENE_KEYS:
            assert own[k].tobytes() == plain[k].tobytes(), (name, k)
        assert np.array_equal(own["seg_status"], plain["seg_status"])
        done = plain["seg_status"] != S.CERT_BLOCKED
        assert (own["seg_self_upper"] == 1.0).all() and (own["seg_self_lower"][done] == np.float32(1.0) - np.float32(rc.GUARD)).all()
    # BUDGET, DEPTH and NOT_FINITE with their -inf lowers, on the inputs of tests/cert_cases.py: the carried body is the cube on the floor,
    # which no probe sits on (its geom skipped in all three calls), the self model an all-zero mask
    import cert_cases

    from gym_genesis.backend.lib import MirScene

    sb = cert_cases.case("budget")["sb"]
    sc = MirScene(cert_cases.case("budget")["spec"], B)
    cube = carry_cases.EntityView(sc, sb, "cube", ())
    want = {"budget": S.CERT_BUDGET, "depth": S.CERT_DEPTH, "nan": S.CERT_NOT_FINITE}
    for name in want:
        c = cert_cases.case(name)
        sc.set_state(qpos=c["q"], qvel=np.zeros((B, sc.nv), np.float32))
        kw = dict(probes=c["probes"], links=c["links"], dof_qadr=c["qadr"], skip_geoms=c["skip"] | cube._own_geoms(), max_leaves=MAX_LEAVES, **c["par"])
        plain = {k: v.cpu().numpy() for k, v in sc.certify_path(paths=c["paths"], **kw).items()}
        assert (plain["seg_status"] == want[name]).any(), (name, plain["seg_status"])
        assert name == "depth" or np.isneginf(plain["seg_lower"][plain["seg_status"] == want[name]]).all()
        carry = {k: v.cpu().numpy() for k, v in sc.certify_path(paths=c["paths"], carry=dict(body=sb.body_index("cube"), link=sb.body_index("hand")), **kw).items()}
        for k in plain:
            assert carry[k].tobytes() == plain[k].tobytes(), (name, k)
        own = {k: v.cpu().numpy() for k, v in sc.certify_path(paths=c["paths"], self_model=zero, **kw).items()}
        for k in SCENE_KEYS + ("seg_status", "row_status", "row_first"):
            assert own[k].tobytes() == plain[k].tobytes(), (name, k)
        assert np.isneginf(own["seg_self_lower"][np.isin(plain["seg_status"], (S.CERT_BUDGET, S.CERT_NOT_FINITE))]).all()


def test_addressing():
    """f. env_idx with repeats, qpos_start against the current state, one launch of R rows against R launches of one"""
    for name in ("self_clear", "carry_given"):
        base, again = _call(name), _call(name)
        assert all(np.array_equal(base[k], again[k], equal_nan=True) for k in base), "two identical calls give identical bits"
        idx = np.array([3, 0, 3, 4, 2, 1, 0])
        got = _call(name, rows=idx)
        assert all(np.array_equal(got[k], base[k][idx], equal_nan=True) for k in base), "env_idx with repeats: row k is the path of env_idx[k]"
        for r in (0, 4):
            one = _call(name, rows=[r])
            assert all(np.array_equal(one[k][0], base[k][r], equal_nan=True) for k in base), "one launch of R rows equals R launches of one row"
        c = rc.case(name)
        rows = _call(name, qpos_start=c["q"])
        assert all(np.array_equal(rows[k], base[k], equal_nan=True) for k in base), "qpos_start rows equal to the state give the same bits"
    # start rows that differ from the state: the carried cube 1 cm further down in the fingers -> another grasp than the state's
    import plan_ref

    c = rc.case("carry_clear")
    base = _call("carry_clear")
    moved = c["q"].copy()
    moved[:, plan_ref.kin_ref.Model(c["spec"]).qadr[c["carry"][0]] + 2] -= 0.01
    other = _call("carry_clear", qpos_start=moved)
    assert not np.array_equal(other["grasp"], base["grasp"]) and not np.array_equal(other["seg_self_upper"], base["seg_self_upper"]), "the start rows are read, not the state"
    assert all(np.array_equal(_call("carry_clear")[k], base[k]) for k in base)


def test_invisible_to_the_scene_and_refusals_write_nothing():
    """f."""
    from gym_genesis.backend.lib import MirError, _ptr

    sc = _scene("carry_clear")
    c, kw = _args("carry_clear", sc)
    state = [x.clone() for x in sc.get_state()]
    launches = sc.__dict__.get("cert_launches", 0)
    sc.step(1)
    after_plain = [x.clone() for x in sc.get_state()]
    sc.set_state(*state)
    version = sc.state_version
    out = sc.certify_path(paths=c["paths"], **kw)
    assert (out["row_status"] == 0).all() and sc.__dict__.get("cert_launches", 0) == launches + 1
    assert all(torch.equal(x, y) for x, y in zip(state, sc.get_state())) and sc.state_version == version
    sc.step(1)
    assert all(torch.equal(x, y) for x, y in zip(after_plain, sc.get_state())), "a following step does not see the call"
    sc.set_state(*state)
    # refusals through the wrapper: each names its entry point
    for bad in (dict(max_depth=21), dict(max_evaluations=0), dict(tol=1e-6), dict(guard=-1.0), dict(margin=-1.0), dict(max_distance=0.0)):
        with pytest.raises(MirError, match="mir_certify_path_carry"):
            sc.certify_path(paths=c["paths"], **{**kw, **bad})
    with pytest.raises(MirError, match="mir_certify_path_carry: a geom of the carried body is not skipped"):
        sc.certify_path(paths=c["paths"], **{**kw, "skip_geoms": c["skip"] & ~carry_cases.views("under", c["sb"])[1]._own_geoms()})
    own = {**kw}
    own.pop("carry")
    with pytest.raises(MirError, match="mir_certify_path_self: link_mask is not symmetric"):
        lop = c["mask"].copy()
        lop[3] |= np.uint32(1 << 9)
        lop[9] &= ~np.uint32(1 << 3)
        sc.certify_path(paths=c["paths"], **{**own, "self_model": {**kw["self_model"], "link_mask": lop}})
    with pytest.raises(ValueError, match="grasp belongs to carry"):
        sc.certify_path(paths=c["paths"], grasp=torch.zeros(B, 7), **own)
    # the raw entry points: a refusal launches nothing and writes no output byte
    K = c["paths"].shape[1]
    q = S.make_cert_query(K, max_leaves=4)
    pq = S.make_plan_query(len(c["probes"]) - c["n_extra"], len(c["qadr"]), skip_geoms=c["skip"])
    sq = S.make_self_query(c["mask"], c["n_extra"], 0.0, 1.0)
    cq = S.make_carry_query(*c["carry"])
    p, lk, qa, idx, R, qs = sc._plan_front(c["probes"], c["links"], c["qadr"], None, None)
    paths = torch.as_tensor(c["paths"], device=sc.device)
    f = lambda *shape: torch.full((B, *shape), -7.0, device=sc.device)  # noqa: E731
    i = lambda *shape: torch.full((B, *shape), -7, dtype=torch.int32, device=sc.device)  # noqa: E731
    bufs = dict(seg_lower=f(K - 1), seg_upper=f(K - 1), seg_self_lower=f(K - 1), seg_self_upper=f(K - 1), seg_status=i(K - 1), row_lower=f(), row_upper=f(),
                row_self_lower=f(), row_self_upper=f(), row_status=i(), row_first=i(), grasp_used=f(7), leaves=i(4, 3), stats=i(4))
    front = (_ptr(p), lk.ctypes.data_as(C.c_void_p), qa.ctypes.data_as(C.c_void_p), _ptr(idx), R, _ptr(qs))

    def carry_call(q, sq, cq, grasp=None, **null):
        o = [None if k in null else _ptr(b) for k, b in bufs.items()]
        rcode = sc.lib.mir_certify_path_carry(sc.h, C.byref(q), C.byref(pq), None if sq is None else C.byref(sq), None if cq is None else C.byref(cq),
                                              *front, _ptr(grasp), _ptr(paths), *o, sc._stream())
        return rcode, sc.lib.mir_last_error().decode() if rcode else ""

    def self_call(q, sq, **null):
        o = [None if k in null else _ptr(b) for k, b in bufs.items() if k != "grasp_used"]
        rcode = sc.lib.mir_certify_path_self(sc.h, C.byref(q), C.byref(pq), None if sq is None else C.byref(sq), *front, _ptr(paths), *o, sc._stream())
        return rcode, sc.lib.mir_last_error().decode() if rcode else ""

    sc.lib.mir_last_error.restype = C.c_char_p
    bad = S.make_cert_query(K, max_depth=21, max_leaves=4)
    assert carry_call(bad, sq, cq) == (-1, "mir_certify_path_carry: max_depth outside 0 .. 20")
    assert carry_call(q, None, None) == (-1, "mir_certify_path_carry: neither a MirSelfQuery nor a MirCarryQuery (mir_certify_path judges the scene test alone)")
    assert carry_call(q, None, cq) == (-1, "mir_certify_path_carry: seg_self_lower / seg_self_upper / row_self_lower / row_self_upper without a MirSelfQuery")
    assert carry_call(q, sq, None) == (-1, "mir_certify_path_carry: grasp_used without a MirCarryQuery")
    assert carry_call(q, sq, None, grasp=bufs["grasp_used"], grasp_used=1) == (-1, "mir_certify_path_carry: grasp without a MirCarryQuery")
    assert self_call(q, None) == (-1, "mir_certify_path_self: null self query")
    assert self_call(bad, sq) == (-1, "mir_certify_path_self: max_depth outside 0 .. 20")
    torch.cuda.synchronize()
    assert all(bool((b == -7).all()) for b in bufs.values()), "a refusal writes no output byte"
    assert carry_call(q, sq, cq, **{k: 1 for k in bufs}) == (-1, "mir_certify_path_carry: max_leaves > 0 without leaves")
    q0 = S.make_cert_query(K, max_leaves=0)
    assert carry_call(q0, sq, cq, **{k: 1 for k in bufs})[0] == 0, "every output NULL: MIR_OK, nothing to do"
    torch.cuda.synchronize()
    assert all(bool((b == -7).all()) for b in bufs.values())
    assert carry_call(q, sq, cq)[0] == 0
    torch.cuda.synchronize()
    assert all(bool((b != -7).any()) for k, b in bufs.items()), "the good call writes every output"
    none = sc.certify_path(paths=c["paths"][:0], env_idx=torch.zeros(0, dtype=torch.long), **kw)
    assert none["seg_self_lower"].shape == (0, K - 1) and none["grasp"].shape == (0, 7) and sc.__dict__.get("cert_launches", 0) == launches + 1, "no rows: no launch"
    step_bufs = (sc.empty(sc.agent_dim), sc.empty(sc.env_dim), sc.empty(), sc.empty(dtype=torch.uint8))
    sc.step_begin(None, *step_bufs)
    try:
        with pytest.raises(MirError, match="mir_certify_path_carry: a step is pending"):
            sc.certify_path(paths=c["paths"], **kw)
    finally:
        sc.step_end()
        sc.set_state(*state)
        torch.cuda.synchronize()


def test_entity_view():
    """shapes, keys, the unbatched form; certify_path keeps its refusal; without self test and carried object certify_sweep is certify_path"""
    from gym_genesis.backend.lib import MirScene

    c, sc = rc.case("carry_clear"), _scene("carry_clear")
    robot, obj, _ = carry_cases.views("under", c["sb"], sc)
    path = torch.as_tensor(c["paths"], device=sc.device).permute(1, 0, 2)
    att = dict(attached_entity=obj, ee_link_name="hand", self_collision=False)
    raw = _call("carry_clear", max_leaves=0)
    status = robot.certify_sweep(path, **att)
    assert status.dtype == torch.int32 and status.shape == (B,) and np.array_equal(status.cpu().numpy(), raw["row_status"])
    assert bool(robot.sweep_is_certified_clear(path, **att).all())
    det = robot.certify_sweep(path, return_detail=True, bracket=True, max_leaves=4, **att)
    assert set(det) == {"status", "first", "lower", "upper", "seg_lower", "seg_upper", "seg_status", "stats", "leaves", "self_lower", "self_upper",
                        "seg_self_lower", "seg_self_upper", "grasp"}
    assert det["leaves"].shape == (B, 4, 3) and det["seg_self_lower"].shape == (B, 1) and det["self_upper"].shape == (B,) and det["grasp"].shape == (B, 7)
    assert np.array_equal(det["grasp"].cpu().numpy(), raw["grasp"])
    g = torch.as_tensor(rc.given_grasp()[0], device=sc.device)
    one = robot.certify_sweep(path, grasp_pose=g, return_detail=True, **att)["grasp"]
    assert torch.equal(one[:, :3], g[:3].expand(B, 3))
    both = robot.certify_sweep(path, return_detail=True, **{**att, "self_collision": True})
    assert (both["status"] == 0).all() and (both["self_upper"] <= det["self_upper"]).all(), "arm against arm on top of the carried pairs"
    plain = robot.certify_sweep(path, self_collision=False, ignore_entities=[obj], return_detail=True)
    scene_only = robot.certify_path(path, ignore_entities=[obj], return_detail=True)
    assert all(torch.equal(plain[k], scene_only[k]) for k in scene_only) and torch.isposinf(plain["self_lower"]).all() and torch.isnan(plain["grasp"]).all()
    with pytest.raises(ValueError, match="sampled only"):
        robot.certify_path(path, self_collision=True)
    with pytest.raises(ValueError, match="sampled only"):
        robot.certify_path(path, attached_entity=obj)
    with pytest.raises(ValueError, match="path must be"):
        robot.certify_sweep(path[:1], **att)
    with pytest.raises(ValueError, match="belong to attached_entity"):
        robot.certify_sweep(path, ee_link_name="hand")
    s1 = MirScene(c["spec"], 1)
    s1.set_state(qpos=c["q"][:1], qvel=np.zeros((1, s1.nv), np.float32))
    single, obj1, _ = carry_cases.views("under", c["sb"], s1)
    single.unbatched = True
    d1 = single.certify_sweep(path[:, 0], return_detail=True, attached_entity=obj1, ee_link_name="hand", self_collision=False)
    assert d1["status"].dim() == 0 and d1["seg_self_upper"].shape == (1,) and d1["grasp"].shape == (7,) and d1["self_lower"].dim() == 0
    assert int(d1["status"]) == int(raw["row_status"][0]) and float(d1["self_lower"]) == float(raw["row_self_lower"][0])
    assert single.sweep_is_certified_clear(path[:, 0], attached_entity=obj1, ee_link_name="hand", self_collision=False).dim() == 0
