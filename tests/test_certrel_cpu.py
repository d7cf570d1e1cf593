"""CPU tier of the certified clearance with the self test and a carried object (include/mirigid.h: mir_certify_path_self,
mir_certify_path_carry): the bound the rule rests on, the host half of the entry points (`make certrel-host`) bit for bit against the
float32 port of tests/certrel_ref.py, and the conditions the GPU tests of tests/test_gpu_certrel.py lean on.  If a condition fails for an
input, the input changes, not the condition.

  1. the bound itself: on the five tree_cases and the Franka, at 20 random segments (a configuration inside the limits and a dq), for
     every pair of spheres on different links the float64 central difference of s_ij along the segment never exceeds v_ij (without its
     factor 1.0001) by more than 1e-9 relative, and |s_ij(t1) - s_ij(t0)| <= |t1 - t0| v_ij at random t; the same with a body carried by
     the Franka's hand at random grasps.
  2. the float32 v_ij is never below the float64 v_ij without its 1.0001: the smallest ratio is printed.
  3. soundness: for every case and row, reference and port, lower and lower_s <= the dense float64 minima at 2048 samples per segment, and
     a CLEAR or UNDECIDED segment has each bracket closed to tol or its lower at the margin.
  4. what makes the GPU comparisons fair: the segment minima of self_clear, carry_clear and carry_given lie >= tol + 0.9 mm clear of their
     margins (whichever leaves a float32 run accepts, the segment is CLEAR); self_thin and carry_arm pass the sampled check at resolution
     0.1 by >= 1 mm in both number formats while their witnesses lie >= 1 mm under; carry_under's witness lies >= 1 mm under; budget,
     depth, nan and the NaN grasp end as the rule says; common takes three evaluations where the naive bound v_i + v_j cannot close its
     first node.
  5. the host half: every refusal with its text; the scalar functions, the branch sums and the LCA table bit for bit against the port.
(derive_carry_arm() takes about a minute and is not run here; 4. checks what it promises.)
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import carry_cases
import carry_ref
import cert_ref
import certrel_cases as rc
import certrel_ref as rr
import kin_ref
import plan_cases as pc
import self_ref
import tree_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MM = 1e-3
ROWS = range(rc.B)
FACTOR = float(np.float32(1.0001))


# ---- 1. the bound itself
def _tree_problem(name, dtype=np.float64):
    """one sphere per link (the Franka: the coarse model), every pair of different links enabled -> (problem, a full start row)"""
    if name == "franka":
        c = pc.case("clear")
        links, probes, spec, qadr, skip, q = c["links"], c["probes"], c["spec"], c["qadr"], c["skip"], c["q"][0].astype(np.float64)
    else:
        _, spec = tree_cases.build(name)
        m = kin_ref.Model(spec)
        rng = np.random.default_rng(7)
        qadr = [m.qadr[b] for b in range(1, m.nbody) if m.jtype[b] in (kin_ref.REVOLUTE, kin_ref.PRISMATIC)]
        links = np.arange(1, m.nbody)
        probes = np.concatenate([rng.uniform(-0.1, 0.1, (len(links), 3)), np.full((len(links), 1), 0.03)], 1)
        skip, q = (1 << spec.ngeom) - 1, np.zeros(m.nq)
        for b in range(1, m.nbody):
            if m.jtype[b] == kin_ref.FREE:
                q[m.qadr[b]:m.qadr[b] + 7] = (0.1, -0.2, 0.6, 0.8, 0.0, 0.6, 0.0)
    n = spec.nbody
    mask = [((1 << n) - 1) & ~(1 << a) for a in range(n)] + [0] * (32 - n)
    return self_ref.SelfProblem(spec, probes, links, qadr, 0, mask, skip, 1.0, 0.0, 1.0, dtype), q


def _pair_distances64(pb, q):
    pw = pb.centres(q).astype(np.float64)
    rad = np.asarray(pb.probes[:, 3], np.float64)
    return np.linalg.norm(pw[:, None] - pw[None], axis=2) - (rad[:, None] + rad[None])


def _check_bound(pb, qrow, rng, label, segments=20):
    h, worst, worst_sec = 1e-6, -np.inf, -np.inf
    for _ in range(segments):
        lo, hi = pb.lo.astype(np.float64), pb.hi.astype(np.float64)
        a = lo + rng.uniform(0.02, 0.98, pb.D) * (hi - lo)
        b = np.clip(a + rng.uniform(-0.5, 0.5, pb.D) * rng.integers(0, 2, pb.D), lo, hi)   # (some joints stand still)
        row = qrow.copy()
        row[pb.qadr] = a
        pb.set_row(row)
        V = rr.speeds(pb, a, b)[1] / FACTOR
        on = pb.enabled
        for t in rng.uniform(0.05, 0.95, 3):
            q = lambda x: a + x * (b - a)  # noqa: E731
            fd = np.abs(_pair_distances64(pb, q(t + h)) - _pair_distances64(pb, q(t - h))) / (2 * h)
            gap = np.where(on, fd - V * (1 + 1e-9), -np.inf)
            worst = max(worst, float(gap.max()))
            assert (gap <= 1e-9).all(), (label, float(gap.max()), np.unravel_index(gap.argmax(), gap.shape))
        t0, t1 = rng.uniform(0, 1, 2)
        sec = np.abs(_pair_distances64(pb, a + t1 * (b - a)) - _pair_distances64(pb, a + t0 * (b - a)))
        gap = np.where(on, sec - abs(t1 - t0) * V * (1 + 1e-9), -np.inf)
        worst_sec = max(worst_sec, float(gap.max()))
        assert (gap <= 1e-12).all(), (label, float(gap.max()))
    print(f"\n[{label}] largest (finite difference - v_ij) {worst:+.3e}, largest (secant - |dt| v_ij) {worst_sec:+.3e}")


@pytest.mark.parametrize("name", tree_cases.CASES + ("franka",))
def test_pair_speed_never_exceeds_the_bound(name):
    pb, qrow = _tree_problem(name)
    _check_bound(pb, qrow, np.random.default_rng(23), name)


def test_pair_speed_with_a_carried_body_at_random_grasps():
    c = carry_cases.case("rod")
    n = c["spec"].nbody
    mask = [((1 << n) - 1) & ~(1 << a) for a in range(n)] + [0] * (32 - n)   # (the rod against every link, and arm against arm)
    pb = carry_ref.CarryProblem(c["spec"], c["probes"], c["links"], c["qadr"], c["n_extra"], mask, c["body"], c["link"], c["skip"], 1.0, 0.0, 1.0)
    rng = np.random.default_rng(29)
    for k in range(20):
        quat = rng.normal(size=4)
        pb.grasp = np.concatenate([rng.uniform(-0.15, 0.15, 3), quat / np.linalg.norm(quat)])
        _check_bound(pb, c["q"][0].astype(np.float64), rng, f"franka + rod, grasp {k}", segments=1)
        assert abs(float(rr.cn(pb)[c["links"] == c["body"]][0]) - (np.linalg.norm(pb.grasp[:3]) + np.linalg.norm(c["probes"][c["links"] == c["body"]][0, :3]))) < 1e-6


# ---- 2. the float32 bound is not below the float64 one
def test_the_float32_speed_bound_covers_the_float64_one():
    smallest = np.inf
    for name in tree_cases.CASES + ("franka",):
        p64, qrow = _tree_problem(name)
        p32, _ = _tree_problem(name, np.float32)
        rng = np.random.default_rng(31)
        for _ in range(20):
            lo, hi = p64.lo.astype(np.float64), p64.hi.astype(np.float64)
            a = (lo + rng.uniform(0.02, 0.98, p64.D) * (hi - lo)).astype(np.float32)
            b = np.clip(a + rng.uniform(-0.5, 0.5, p64.D) * rng.integers(0, 2, p64.D), lo, hi).astype(np.float32)
            row = qrow.copy()
            row[p64.qadr] = a
            p64.set_row(row)
            p32.set_row(row)
            V64, V32 = rr.speeds(p64, a, b)[1] / FACTOR, rr.speeds(p32, a, b)[1].astype(np.float64)
            assert (V32 >= V64).all(), (name, float((V32 - V64).min()))
            some = V64 > 0
            if some.any():
                smallest = min(smallest, float((V32[some] / V64[some]).min()))
    for name in ("self_clear", "carry_clear", "carry_arm"):
        c = rc.case(name)
        for r in ROWS:
            p64, p32 = rc.row_problem(name, r), rc.row_problem(name, r, "float32")
            p64.set_row(c["q"][r])
            p32.set_row(c["q"][r])
            for s in range(c["paths"].shape[1] - 1):
                v64, V64 = rr.speeds(p64, c["paths"][r, s], c["paths"][r, s + 1])
                v32, V32 = rr.speeds(p32, c["paths"][r, s], c["paths"][r, s + 1])
                assert (V32.astype(np.float64) >= V64 / FACTOR).all() and (v32.astype(np.float64) >= v64 / FACTOR).all(), (name, r, s)
                some = V64 > 0
                smallest = min(smallest, float((V32[some] / (V64[some] / FACTOR)).min()))
    print(f"\n[certrel] smallest float32 v_ij over float64 v_ij without its factor: {smallest:.8f} (the factor is {FACTOR:.8f})")
    assert smallest >= 1.0


# ---- 3. soundness
@pytest.mark.parametrize("name", rc.NAMES)
def test_lower_bounds_hold_against_the_dense_minima(name):
    c = rc.case(name)
    par, on = c["par"], rc.self_on(name)
    tol = float(np.float32(par["tol"]))
    for dtn in ("float64", "float32"):
        for r in ROWS:
            ref, (dense, dense_s) = rc.reference(name, r, dtn), rc.dense(name, r)
            for s, st in enumerate(ref["seg_status"]):
                lo, up = float(ref["seg_lower"][s]), float(ref["seg_upper"][s])
                lo_s, up_s = float(ref["seg_self_lower"][s]), float(ref["seg_self_upper"][s])
                assert lo <= dense[s] and (not on or lo_s <= dense_s[s]), (name, dtn, r, s, lo, dense[s], lo_s, dense_s[s])
                if st in (cert_ref.CLEAR, cert_ref.UNDECIDED):
                    assert up - lo <= tol or lo >= par["margin"], (name, dtn, r, s, lo, up)
                    assert not on or up_s - lo_s <= tol or lo_s >= c["self_margin"], (name, dtn, r, s, lo_s, up_s)
                    assert up >= dense[s] - 1e-6 and (not on or up_s >= min(dense_s[s], float(c["self_max"])) - 1e-6)
            done = [s for s, st in enumerate(ref["seg_status"]) if st in (cert_ref.CLEAR, cert_ref.UNDECIDED, cert_ref.DEPTH)]
            for s in done:
                assert cert_ref.tiles([(l, k) for (ss, l, k) in ref["leaves"] if ss == s]), (name, dtn, r, s)
            assert ref["stats"][3] == len(done)


def test_bracket_mode_closes_both_brackets():
    tol = float(np.float32(rc.TOL))
    for dtn in ("float64", "float32"):
        for r in ROWS:
            ref, (dense, dense_s) = rc.reference("self_clear", r, dtn, True), rc.dense("self_clear", r)
            assert (ref["seg_status"] == cert_ref.CLEAR).all()
            assert (ref["seg_upper"] - ref["seg_lower"] <= tol + 1e-7).all() and (ref["seg_lower"] <= dense).all()
            assert (ref["seg_self_upper"] - ref["seg_self_lower"] <= tol + 1e-7).all() and (ref["seg_self_lower"] <= dense_s).all()


# ---- 4. what makes the GPU comparisons fair
def test_status_deciding_minima_are_a_millimetre_from_the_margins():
    tol = float(np.float32(rc.TOL))
    for name in ("self_clear", "carry_clear", "carry_given"):
        for r in ROWS:
            dense, dense_s = rc.dense(name, r)
            assert (dense >= tol + 0.9 * MM).all() and (dense_s >= tol + 0.9 * MM).all(), (name, r, dense, dense_s)
            for dtn in ("float64", "float32"):
                assert (rc.reference(name, r, dtn)["seg_status"] == cert_ref.CLEAR).all()
    for r in ROWS:
        for dtn in ("float64", "float32"):
            ref = rc.reference("carry_under", r, dtn)
            assert ref["seg_status"][0] == cert_ref.BLOCKED and float(ref["seg_upper"][0]) <= -MM and float(ref["seg_self_upper"][0]) >= 0.1
            b = rc.reference("budget", r, dtn)
            assert b["seg_status"].tolist() == [cert_ref.CLEAR, cert_ref.BUDGET] and b["stats"][0] == 8
            d = rc.reference("depth", r, dtn)
            assert d["row_status"] == cert_ref.DEPTH and d["stats"][2] == 2
            n = rc.reference("nan", r, dtn)
            assert n["seg_status"].tolist() == ([5, 5] if r == 1 else [0, 0])
            g = rc.reference("nan_grasp", r, dtn)
            assert g["seg_status"].tolist() == ([5] if r == 2 else [0]) and (r != 2 or g["stats"] == (0, 0, 0, 0))


@pytest.mark.parametrize("name,resolution", [("self_thin", rc.THIN_RESOLUTION), ("carry_arm", rc.ARM_RESOLUTION)])
def test_the_sampled_check_passes_and_the_certified_one_does_not(name, resolution):
    c = rc.case(name)
    for dtn in ("float64", "float32"):
        for r in ROWS:
            pb = rc.row_problem(name, r, dtn)
            seg, seg_self, samples = self_ref.polyline_clearances(pb, c["q"][r], c["paths"][r].astype(pb.dtype), resolution)
            assert float(seg.min()) >= MM and float(seg_self.min()) >= MM, (name, dtn, r, seg, seg_self)
            assert len(samples) >= 3, "the dip lies between samples, not between the waypoints alone"
            ref = rc.reference(name, r, dtn)
            assert rc.dense(name, r)[1][0] <= -MM and rc.dense(name, r)[0][0] >= 0.1
            assert ref["seg_status"][0] == cert_ref.BLOCKED and float(ref["seg_self_upper"][0]) <= -MM and float(ref["seg_upper"][0]) >= 0.1, (name, dtn, r)
            last = ref["nodes"][-1]
            assert last.get("witness") and float(last["us"]) <= -MM and (last["l"], last["k"]) != (0, 0), "the witness is not the midpoint of the edge"
    if name == "self_thin":   # the thin sphere rides on the base link and is a self-only sphere; a finger or hand sphere meets it
        assert c["links"][-1] == rc.BASE_LINK and c["n_extra"] == 9 and float(c["probes"][-1, 3]) == np.float32(rc.THIN_RADIUS)
    else:                     # the partner of the rod's sphere rides on a link between the shoulder and the wrist
        pb = rc.row_problem(name, 0)
        pb.set_row(c["q"][0])
        a, b = c["paths"][0].astype(np.float64)
        s = rr.pair_distances(pb, pb.centres(a + 0.25 * (b - a)))
        i, j = np.unravel_index(s.argmin(), s.shape)
        pair = {int(c["links"][i]), int(c["links"][j])}
        assert pair == {c["carry"][0], 2} and (int(c["mask"][c["carry"][0]]) >> 2) & 1, pair


def test_common_takes_three_evaluations_where_the_naive_bound_cannot():
    for name in ("common", "common_capped"):
        c = rc.case(name)
        guard, tol = np.float32(rc.GUARD), np.float32(rc.TOL)
        for r in ROWS:
            for dtn in ("float64", "float32"):
                ref = rc.reference(name, r, dtn)
                assert ref["stats"] == (3, 1, 0, 1) and ref["seg_status"].tolist() == [0], (name, r, dtn, ref["stats"])
                if name == "common_capped":
                    assert ref["seg_self_upper"][0] == rc.COMMON_CAP and ref["seg_self_lower"][0] == ref["seg_self_upper"].dtype.type(rc.COMMON_CAP) - guard.astype(ref["seg_self_upper"].dtype)
            pb = rc.row_problem(name, r)
            pb.set_row(c["q"][r])
            a, b = c["paths"][r].astype(np.float64)
            v, V = rr.speeds(pb, a, b)
            assert (np.where(pb.enabled, V, 0.0) == 0.0).all(), "every enabled pair hangs below joint 1"
            assert rc.dense(name, r)[1][0] > rc.COMMON_CAP + MM, "the cap lies below every pair distance of the sweep"
            # the naive bound: each sphere's own speed against the world, as the scene test uses it
            p_all = self_ref.SelfProblem(c["spec"], c["probes"], c["links"], c["qadr"], 0, c["mask"], c["skip"], c["max_distance"], 0.0, c["self_max"])
            p_all.set_row(c["q"][r])
            vi = rr.speeds(p_all, a, b)[0]
            naive = vi[:, None] + vi[None, :]
            s = rr.pair_distances(pb, pb.centres(0.5 * (a + b)))
            lo_naive = float(np.where(pb.enabled, np.minimum(s, pb.self_max) - 0.5 * naive, np.inf).min()) - float(guard)
            up = float(min(pb.self_max, s.min()))
            assert lo_naive < 0.0 and lo_naive < up - float(tol), (name, r, lo_naive, up)


# ---- 5. the host half
@pytest.fixture(scope="module")
def host():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "gym-genesis_amd", "csrc"), "certrel-host"], stdout=subprocess.DEVNULL)
    lib = C.CDLL(os.path.join(ROOT, "tests", "_build", "libmircertrel.so"))
    f, fp, ip, i, ll = C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_int, C.c_longlong
    lib.certrel_host_check.argtypes = [i, C.c_uint, C.c_char_p]
    lib.certrel_host_lds_bytes.argtypes, lib.certrel_host_lds_bytes.restype = [ll, ll, ll, i], ll
    lib.certrel_host_check_lds.argtypes = [ll, ll, ll, i, C.c_char_p]
    lib.certrel_host_rel.argtypes, lib.certrel_host_rel.restype = [f] * 4, f
    lib.certrel_host_speed.argtypes, lib.certrel_host_speed.restype = [f] * 2, f
    lib.certrel_host_steps.argtypes = [i, i]
    lib.certrel_host_cn_carried.argtypes, lib.certrel_host_cn_carried.restype = [f] * 2, f
    lib.certrel_host_pair_bound.argtypes, lib.certrel_host_pair_bound.restype = [f] * 4, f
    lib.certrel_host_status.argtypes = [i, i, i, f, f, f, i, f, f, f]
    lib.certrel_host_lca.argtypes = [i, ip, ip, i, i, C.POINTER(C.c_uint8)]
    lib.certrel_host_branch.argtypes = [i, ip, ip, ip, fp, fp, fp, fp]
    return lib


def _check(host, carry_form, present):
    what = C.create_string_buffer(128)
    return host.certrel_host_check(int(carry_form), present, what), what.value.decode()


def test_host_refusals(host):
    SQ, CQ, GRASP, USED = 1, 2, 4, 8
    ok, inv = (0, ""), -1
    assert _check(host, True, SQ | CQ | GRASP | USED | 0xf0) == ok and _check(host, True, SQ | 0xf0) == ok and _check(host, True, CQ | GRASP | USED) == ok
    assert _check(host, False, SQ | 0xf0) == ok and _check(host, False, SQ) == ok
    assert _check(host, False, 0) == (inv, "null self query") and _check(host, False, 0xf0) == (inv, "null self query")
    assert _check(host, True, 0) == (inv, "neither a MirSelfQuery nor a MirCarryQuery (mir_certify_path judges the scene test alone)")
    for bit in range(4, 8):
        assert _check(host, True, CQ | (1 << bit)) == (inv, "seg_self_lower / seg_self_upper / row_self_lower / row_self_upper without a MirSelfQuery")
    assert _check(host, True, SQ | GRASP | USED) == (inv, "grasp without a MirCarryQuery")
    assert _check(host, True, SQ | USED) == (inv, "grasp_used without a MirCarryQuery")
    # the capacity: F + 4 N + 4 (N + E), and 16 (N + E) more with a self query
    assert host.certrel_host_lds_bytes(24864, 57, 65, 1) == 24864 + 4 * 57 + 20 * 65 and host.certrel_host_lds_bytes(24864, 57, 57, 0) == 24864 + 8 * 57
    what = C.create_string_buffer(128)
    assert host.certrel_host_check_lds(24864, 1024, 1024, 1, what) == 0, "1024 spheres fit"
    rcode = host.certrel_host_check_lds(24864, 1024, 2048, 1, what)
    assert rcode not in (0, inv) and what.value.decode() == "the speed bounds and the sphere list do not fit 64 KB of LDS (n_probes, n_probes + n_extra)"


def _host_tables(host, pb, a, b):
    """the LCA table and every body's branch sums from the host functions, on the port's own S"""
    f32, m, st, cst, e = np.float32, pb.model, rr._struct(pb), cert_ref._structure(pb), rr.eff(pb)
    n = m.nbody
    rows, S, _, _, _ = rr.branch(pb, a, b)
    adq_d = np.abs((np.asarray(b, f32) - np.asarray(a, f32)).astype(f32))
    kind = np.array([0 if cst["jd"][k] < 0 else (1 if m.jtype[k] == kin_ref.REVOLUTE else 2) for k in range(n)], np.int32)
    adq = np.array([adq_d[cst["jd"][k]] if cst["jd"][k] >= 0 else 0 for k in range(n)], f32)
    axl = np.ascontiguousarray(cst["axis_len"], f32)
    par, dep = np.ascontiguousarray(m.parent, np.int32), np.ascontiguousarray(st["depth"], np.int32)
    p = lambda x: x.ctypes.data_as(C.POINTER({np.dtype(f32): C.c_float, np.dtype(np.int32): C.c_int32, np.dtype(np.uint8): C.c_uint8}[x.dtype]))  # noqa: E731
    Cb, Lk = rr._carry(pb)
    table = np.zeros((n, n), np.uint8)
    host.certrel_host_lca(n, p(par), p(dep), Cb, Lk, p(table))
    S32 = np.ascontiguousarray(S, f32)
    got = []
    for body in range(n):
        out = np.zeros(3 * (dep[e[body]] + 2), f32)
        host.certrel_host_branch(e[body], p(par), p(dep), p(kind), p(adq), p(axl), p(S32), p(out))
        got.append(out.reshape(-1, 3))
    return table, got, rows


@pytest.mark.parametrize("name", ("self_clear", "carry_clear", "carry_arm") + tree_cases.CASES)
def test_host_scalar_rules_match_the_port_bit_for_bit(host, name):
    f32 = np.float32
    if name in tree_cases.CASES:
        pb, qrow = _tree_problem(name, f32)
        rng = np.random.default_rng(37)
        a = (pb.lo + rng.uniform(0.1, 0.9, pb.D).astype(f32) * (pb.hi - pb.lo)).astype(f32)
        segs = [(qrow, a, np.clip(a + rng.uniform(-0.4, 0.4, pb.D), pb.lo, pb.hi).astype(f32))]
    else:
        c = rc.case(name)
        pb = rc.row_problem(name, 0, "float32")
        segs = [(c["q"][0], c["paths"][0, s], c["paths"][0, s + 1]) for s in range(c["paths"].shape[1] - 1)]
    for qrow, a, b in segs:
        pb.set_row(qrow)
        table, got, rows = _host_tables(host, pb, a, b)
        assert np.array_equal(table.astype(int), rr.lca(pb)), name
        for body, (g, w) in enumerate(zip(got, rows)):
            if rr.eff(pb)[body] == 0:
                continue
            assert g.tobytes() == w.astype(f32).tobytes(), (name, body, g, w)
        v, V = rr.speeds(pb, a, b)
        cn, st, e, lk = rr.cn(pb), rr._struct(pb), rr.eff(pb), pb.links
        for i in range(0, len(lk), max(1, len(lk) // 12)):
            for j in range(len(lk)):
                ti = host.certrel_host_steps(st["depth"][e[lk[i]]] if e[lk[i]] else -1, int(table[lk[i], lk[j]]))
                tj = host.certrel_host_steps(st["depth"][e[lk[j]]] if e[lk[j]] else -1, int(table[lk[j], lk[i]]))
                assert ti == rr.steps(pb, lk[i], lk[j]) and tj == rr.steps(pb, lk[j], lk[i])
                ri = host.certrel_host_rel(cn[i], *rows[lk[i]][ti])
                rj = host.certrel_host_rel(cn[j], *rows[lk[j]][tj])
                assert f32(host.certrel_host_speed(ri, rj)).tobytes() == f32(V[i, j]).tobytes(), (name, i, j)
    if name == "carry_arm":   # cn of a carried sphere, and one evaluation's pair value
        on = pb.links == rc.case(name)["carry"][0]
        g = rr._norm(pb.G[0].astype(f32), f32)
        plain = np.array([rr._norm(x, f32) for x in pb.probes[on, :3]], f32)
        assert all(f32(host.certrel_host_cn_carried(g, x)).tobytes() == f32(y).tobytes() for x, y in zip(plain, rr.cn(pb)[on]))
    for s, smax, hw, vv in ((0.25, 1.0, 0.5, 0.3), (1.5, 1.0, 0.125, 0.7), (-0.01, 0.03125, 0.0, 5.0)):
        want = f32(f32(min(f32(s), f32(smax))) - f32(f32(hw) * f32(vv)))
        assert f32(host.certrel_host_pair_bound(s, smax, hw, vv)).tobytes() == want.tobytes()
    # the status order, with and without the self half
    st = host.certrel_host_status
    assert st(1, 1, 1, 0.0, -1.0, 0.0, 1, 0.0, -1.0, 0.0) == 5 and st(0, 1, 1, 0.0, -1.0, 0.0, 1, 0.0, -1.0, 0.0) == 3
    assert st(0, 0, 1, 0.1, 0.2, 0.0, 1, -0.1, -0.05, 0.0) == 4 and st(0, 0, 1, 0.1, 0.2, 0.0, 0, -0.1, -0.05, 0.0) == 2
    assert st(0, 0, 0, 0.1, 0.2, 0.0, 1, -0.001, 0.0005, 0.0) == 1 and st(0, 0, 0, 0.1, 0.2, 0.0, 0, -0.001, 0.0005, 0.0) == 0
    assert st(0, 0, 0, 0.1, 0.2, 0.0, 1, 0.01, 0.02, 0.01) == 0 and st(0, 0, 0, 0.1, 0.2, 0.0, 1, 0.009, 0.02, 0.01) == 1
    assert st(0, 0, 0, -0.001, 0.001, 0.0, 1, 0.5, 0.6, 0.0) == 1 and st(0, 0, 0, 0.1, -0.2, 0.0, 1, 0.5, 0.6, 0.0) == 4
