"""The synthetic trees of tests/tree_cases.py and the per-block metrics of tests/tree_metrics.py, CPU tier.

  * the scene compilers accept the five cases as the table of tree_cases.py says: the first four compile for the 16-lane model
    (mir_debug_emit_spec through load_library(), as tests/test_spec_cpu.py does), `many` is refused there with MIR_E_CAPACITY and
    compiles for the wave model (the two compilers as a plain g++ library, tests/compile_host.cpp, `make compile-host`);
  * the shapes the cases promise: path lengths, dofs per path, the free roots, full inertias, oblique axes;
  * the grouping and the bar of tree_metrics on arrays with known blocks.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kin_ref
import tree_cases
import tree_metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIR_E_CAPACITY = -2


@pytest.fixture(scope="module")
def host():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "gym-genesis_amd", "csrc"), "compile-host"], stdout=subprocess.DEVNULL)
    L = C.CDLL(os.path.join(ROOT, "tests", "_build", "libmircompile.so"))
    L.compile_host_rc.argtypes = [C.c_void_p, C.c_int, C.c_char_p]
    L.compile_host_rc.restype = C.c_int
    return L


@pytest.mark.parametrize("name", tree_cases.CASES)
def test_the_compilers_accept_the_cases_as_the_table_says(name, host):
    from gym_genesis.backend.lib import load_library

    sb, spec = tree_cases.build(name)
    buf, err = C.create_string_buffer(1 << 16), C.create_string_buffer(256)
    n = load_library().mir_debug_emit_spec(C.byref(spec), b"X", buf, len(buf))
    rc16 = host.compile_host_rc(C.byref(spec), 16, err)
    msg16 = err.value
    rc64 = host.compile_host_rc(C.byref(spec), 64, err)
    if tree_cases.KERNEL[name] == 16:
        assert n > 0 and buf.value.decode().startswith("struct X {") and rc16 == 0, (n, rc16, msg16)
    else:
        assert n == MIR_E_CAPACITY and rc16 == MIR_E_CAPACITY, (n, rc16, msg16)
        assert rc64 == 0, (rc64, err.value)


def test_the_cases_have_the_shapes_they_are_for():
    nd = {0: 0, 1: 1, 2: 1, 3: 6}
    seen = {}
    for name in tree_cases.CASES:
        sb, spec = tree_cases.build(name)
        again = tree_cases.build(name)[1]
        assert bytes(spec) == bytes(again), "deterministic"
        m = kin_ref.Model(spec)
        assert (m.nbody, m.nv) == tree_cases.DIMS[name]
        paths = {b: m.path(b) for b in range(1, m.nbody)}
        seen[name] = dict(longest=max(len(p) for p in paths.values()), dofs={sum(nd[m.jtype[c]] for c in p) for p in paths.values()},
                          children=[sum(1 for c in range(m.nbody) if m.parent[c] == b and c) for b in range(m.nbody)], model=m)
        for b in range(1, m.nbody):
            s = spec.body[b]
            if m.jtype[b] in (kin_ref.REVOLUTE, kin_ref.PRISMATIC):
                assert min(abs(v) for v in s.axis) > 1e-3 and abs(np.linalg.norm(list(s.axis)) - 1) < 1e-6, "oblique unit axis"
                assert min(abs(v) for v in s.quat) > 1e-3, "no quarter turn"
            if name != "many" or b != m.nbody - 1:
                assert all(abs(v) > 0 for v in list(s.inertia)[3:]) and any(abs(v) > 1e-3 for v in s.ipos), "full inertia, off-origin centre of mass"
    m = seen["oblique_chain"]["model"]
    assert m.jtype[1] == kin_ref.FIXED and [m.jtype[b] for b in range(2, 12)] == [1, 2, 1, 0, 1, 2, 1, 1, 0, 2]
    assert seen["deep"]["longest"] == 15 and max(seen["deep"]["dofs"]) == 15, "a full row of 16 bodies, dof 14 beside the 4-bit code 15"
    assert [seen["deep"]["model"].jtype[b] for b in (4, 8, 12)] == [2, 2, 2]
    assert seen["bushy"]["dofs"] == {1, 2, 3, 4} and seen["bushy"]["children"][1:].count(2) == 7 and seen["bushy"]["children"][1:].count(0) == 8
    assert {1, 2} <= set(seen["bushy"]["model"].jtype[2:])
    m = seen["floating"]["model"]
    assert m.jtype[1] == kin_ref.FREE and seen["floating"]["children"][1] == 3 and seen["floating"]["dofs"] == {6, 7, 8, 9}
    assert m.jtype.count(kin_ref.PRISMATIC) == 1 and float(np.float32(tree_cases.build("floating")[1].body[1].mass)) == 3.0
    m = seen["many"]["model"]
    assert [m.jtype[b] for b in range(1, 10)] == [0, 1, 2, 1, 0, 1, 1, 2, 1] and m.jtype[10] == kin_ref.FREE and m.jtype[16] == kin_ref.FREE
    assert seen["many"]["children"][10] == 2 and seen["many"]["children"][16] == 0
    assert [k for k, _ in tree_metrics.dof_groups(m)] == [(1, "joint"), (10, "lin"), (10, "ang"), (10, "joint"), (16, "lin"), (16, "ang")]


def test_the_metrics_keep_the_blocks_apart():
    m = kin_ref.Model(tree_cases.build("many")[1])
    nv, B = m.nv, 2
    groups = dict(tree_metrics.dof_groups(m))
    assert sorted(np.concatenate(list(groups.values())).tolist()) == list(range(nv)), "every dof in exactly one group"
    assert groups[(10, "ang")].tolist() == [10, 11, 12] and groups[(16, "lin")].tolist() == [18, 19, 20]
    assert groups[(10, "joint")].tolist() == [13, 14, 15, 16, 17] and groups[(1, "joint")].tolist() == list(range(7))
    rng = np.random.default_rng(0)
    scale = np.ones(nv)
    scale[groups[(16, "ang")]] = 1e-7                      # a block ten million times smaller than the rest
    ref = rng.uniform(1, 2, (B, nv)) * scale
    port = ref * (1 + 1e-7)
    got = port.copy()
    assert not tree_metrics.report("unit", tree_metrics.vector_blocks(m, got, port, ref))
    got[:, groups[(16, "ang")][0]] *= 1.5                 # half its size wrong: < 1e-7, below the pooled 4 x 2e-7 of the large blocks
    assert np.abs(got - ref).max() < 4 * np.abs(port - ref).max(), "the pooled rule passes it"
    missed = tree_metrics.report("unit", tree_metrics.vector_blocks(m, got, port, ref))
    assert [x[1] for x in missed] == [(16, "ang")]
    # the floor: a block the port has exactly is owed one float32 rounding of its largest entry, not zero
    port2 = ref.copy()
    got2 = ref * (1 + 0.9 * tree_metrics.EPS32)
    assert not tree_metrics.report("unit", tree_metrics.vector_blocks(m, got2, port2, ref))
    assert tree_metrics.report("unit", tree_metrics.vector_blocks(m, ref * (1 + 1.1 * tree_metrics.EPS32), port2, ref))
    # matrices: pairs of groups of the same tree only; a window addresses `got` from its own dof0
    M = rng.uniform(1, 2, (B, nv, nv))
    rows = tree_metrics.matrix_blocks(m, M, M, M)
    assert len(rows) == 1 + 9 + 4 and all(e == 0 for _, e, _, _ in rows)
    bad = M.copy()
    bad[:, 11, 14] += 1.0
    assert [x[1] for x in tree_metrics.report("unit", tree_metrics.matrix_blocks(m, bad, M, M))] == [(10, "ang", "joint")]
    w = tree_metrics.matrix_blocks(m, bad[:, 9:16, 9:16], M, M, window=(9, 7))
    assert [lab for lab, e, _, _ in w if e > 0] == [(10, "ang", "joint")] and len(w) == 9
    # per-link outputs and Jacobians go by the tree of the link
    links = [9, 12, 15, 16]
    assert [(k, v.tolist()) for k, v in tree_metrics.link_groups(m, links)] == [(1, [0]), (10, [1, 2]), (16, [3])]
    J = rng.uniform(1, 2, (B, len(links), 6, nv))
    Jb = J.copy()
    Jb[:, 2, 4, 15] += 1.0
    assert [x[1] for x in tree_metrics.report("unit", tree_metrics.jac_blocks(m, links, Jb, J, J))] == [(10, "ang", "joint")]
    V = rng.uniform(1, 2, (B, len(links), 6))
    Vb = V.copy()
    Vb[:, 3, 1] += 1.0
    assert [x[1] for x in tree_metrics.report("unit", tree_metrics.link_blocks(m, links, Vb, V, V))] == [(16, "lin")]
