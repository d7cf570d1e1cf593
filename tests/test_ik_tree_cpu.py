"""CPU tier: the tree builder the two inverse-kinematics kernels share (build_ik_tree, the host half of
gym-genesis_amd/csrc/mir_ik_front.h) compiled with plain g++ around a fake model (tests/ik_tree_host.cpp, `make ik-tree-host`) and
called through ctypes.  A wrong table shows on the GPU only as a wrong pose somewhere down a chain; here every entry the kernels read is
compared with what the rules give when they are written once more with numpy in float64: the folded base transforms, the element order,
the pointer-doubling table, the link lanes and ancestor masks, the dof mask, and the refusals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, FIXED, REVOLUTE, PRISMATIC, FREE = 16, 0, 1, 2, 3
INVALID, CAPACITY = -1, -2


class IkElems(C.Structure):
    _fields_ = [("n", C.c_int), ("jtype", C.c_int * G), ("qcol", C.c_int * G), ("pos", C.c_float * 3 * G), ("quat", C.c_float * 4 * G),
                ("axis", C.c_float * 3 * G), ("lo", C.c_float * G), ("hi", C.c_float * G), ("limited", C.c_int * G)]


class IkTree(C.Structure):
    _fields_ = [("el", IkElems), ("par_el", C.c_int * G), ("nsteps", C.c_int), ("anc", C.c_byte * G * 4), ("moving", C.c_int * G),
                ("link_lane", C.c_int * 4), ("anc_mask", C.c_uint * 4), ("moving_cols", C.c_ulonglong), ("n_arm", C.c_int),
                ("arm_qadr", C.c_int * 48)]


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "gym-genesis_amd", "csrc"), "ik-tree-host"], stdout=subprocess.DEVNULL)
    L = C.CDLL(os.path.join(ROOT, "tests", "_build", "libmiriktree.so"))
    assert L.ik_tree_sizeof() == C.sizeof(IkTree)
    return L


class Model:
    """bodies in the order they are added (world = 0), random base transforms and limits seeded by the number of bodies"""

    def __init__(self):
        self.parent, self.jtype = [-1], [FIXED]

    def add(self, parent, jtype):
        self.parent.append(parent)
        self.jtype.append(jtype)
        return len(self.parent) - 1

    def chain(self, parent, jtypes):
        out = []
        for jt in jtypes:
            parent = self.add(parent, jt)
            out.append(parent)
        return out

    def arrays(self):
        nb = len(self.parent)
        rng = np.random.default_rng(nb)
        quat = rng.normal(size=(nb, 4))
        self.pos = rng.uniform(-0.4, 0.4, (nb, 3)).astype(np.float32)
        self.quat = (quat / np.linalg.norm(quat, axis=1, keepdims=True)).astype(np.float32)
        self.axis = np.eye(3, dtype=np.float32)[rng.integers(0, 3, nb)]
        self.lo, self.hi = rng.uniform(-3, -1, nb), rng.uniform(1, 3, nb)
        self.limited = rng.integers(0, 2, nb).astype(np.int32)
        self.qadr = (100 + 3 * np.arange(nb)).astype(np.int32)   # (any addresses: the builder only copies them)
        return nb

    def build(self, lib, links, dof_mask=None):
        nb = self.arrays()
        par, jt = np.asarray(self.parent, np.int32), np.asarray(self.jtype, np.int32)
        p = lambda a, t: a.ctypes.data_as(C.POINTER(t))   # noqa: E731
        t, what = IkTree(), C.create_string_buffer(128)
        lk = np.asarray(links, np.int32)
        dm = None if dof_mask is None else np.asarray(dof_mask, np.uint8)
        rc = lib.ik_tree_build(nb, p(par, C.c_int32), p(jt, C.c_int32), p(self.qadr, C.c_int32), p(self.pos, C.c_float), p(self.quat, C.c_float),
                               p(self.axis, C.c_float), p(self.lo, C.c_double), p(self.hi, C.c_double), p(self.limited, C.c_int32),
                               p(lk, C.c_int32), len(lk), None if dm is None else p(dm, C.c_uint8), C.byref(t), what)
        return rc, t, what.value.decode()

    def col(self, b):
        """column of body b's joint: its rank among the scalar joints in body order"""
        return sum(j in (REVOLUTE, PRISMATIC) for j in self.jtype[1:b]) if self.jtype[b] in (REVOLUTE, PRISMATIC) else -1


def qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def rotm(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def expected(m, links):
    """the rules once more: the union of the chains by depth then body index; a FIXED body that is no link is folded into its children.
    -> [(body, parent element, pos64, quat64)]"""
    on, depth = set(), {}
    for lb in links:
        b = lb
        while b > 0:
            on.add(b)
            b = m.parent[b]
    for b in on:
        d, c = 0, b
        while c > 0:
            d, c = d + 1, m.parent[c]
        depth[b] = d
    el_of, carried, out = {}, {}, []   # carried[b] = (parent element, pos, quat) of a folded body
    for b in sorted(on, key=lambda b: (depth[b], b)):
        p, q, pe = m.pos[b].astype(np.float64), m.quat[b].astype(np.float64), -1
        pb = m.parent[b]
        if pb in carried:
            pe, fp, fq = carried[pb]
            n2 = fq @ fq   # (the model's quaternions are unit to float32 rounding: q v q* and R(q / |q|) differ by |q|^2)
            p, q = fp + n2 * (rotm(fq / np.sqrt(n2)) @ p), qmul(fq, q)
        elif pb > 0:
            pe = el_of[pb]
        if m.jtype[b] == FIXED and b not in links:
            carried[b] = (pe, p, q)
            continue
        el_of[b] = len(out)
        out.append((b, pe, p, q))
    return out


def one_rounding(got, want):
    """got (float32) is the float64 value `want` rounded once: half an ulp, plus the float64 noise of a differently ordered sum"""
    return bool(np.all(np.abs(np.asarray(got, np.float64) - want) <= 2.0 ** -24 * np.abs(want) + 1e-12))


def check(m, t, links, dof_mask=None):
    exp = expected(m, links)
    n = len(exp)
    assert t.el.n == n
    par = [pe for _, pe, _, _ in exp]
    for i, (b, pe, p, q) in enumerate(exp):
        c = m.col(b)
        assert (t.el.jtype[i], t.el.qcol[i], t.par_el[i]) == (m.jtype[b], c, pe), i
        assert one_rounding(t.el.pos[i][:], p) and one_rounding(t.el.quat[i][:], q), (i, t.el.pos[i][:], p)
        assert list(t.el.axis[i]) == list(m.axis[b])
        if c >= 0:
            assert (t.el.lo[i], t.el.hi[i], t.el.limited[i]) == (np.float32(m.lo[b]), np.float32(m.hi[b]), m.limited[b])
            assert t.arm_qadr[c] == m.qadr[b]
        mv = c >= 0 and (dof_mask is None or bool(dof_mask[c]))
        assert t.moving[i] == int(mv) and bool((t.moving_cols >> c) & 1 if c >= 0 else 0) == mv
    for i in range(n, G):   # what the kernels read of a lane behind the last element
        assert (t.el.jtype[i], t.el.qcol[i], t.el.limited[i], t.moving[i]) == (FIXED, -1, 0, 0)
    assert t.n_arm == sum(j in (REVOLUTE, PRISMATIC) for j in m.jtype)
    assert bin(t.moving_cols).count("1") == sum(t.moving[:n])
    # pointer doubling, as the kernel runs it: every element starts with its own transform; step s puts what anc[s] covers in front
    cover = [[i] for i in range(n)]
    for s in range(t.nsteps):
        cover = [cover[i] if t.anc[s][i] < 0 else cover[t.anc[s][i]] + cover[i] for i in range(n)]
    for i in range(n):
        path, j = [], i
        while j >= 0:
            path.insert(0, j)
            j = par[j]
        assert cover[i] == path, (i, cover[i], path)
    depth_max = max(len(c) for c in cover)
    assert t.nsteps == int(np.ceil(np.log2(depth_max))) if depth_max > 1 else t.nsteps == 0
    assert all(t.anc[s][i] == -1 for s in range(t.nsteps, 4) for i in range(G)) and all(t.anc[s][i] == -1 for s in range(4) for i in range(n, G))
    for l, lb in enumerate(links):
        lane = [b for b, *_ in exp].index(lb)
        assert t.link_lane[l] == lane and t.anc_mask[l] == sum(1 << j for j in cover[lane])
    return exp


def panda():
    m = Model()
    base = m.add(0, FIXED)
    arm = m.chain(base, [REVOLUTE] * 7)
    hand = m.add(arm[-1], FIXED)
    lf, rf = m.add(hand, PRISMATIC), m.add(hand, PRISMATIC)
    return m, base, arm, hand, lf, rf


def test_panda_chain_to_the_hand(lib):
    m, base, arm, hand, lf, rf = panda()
    rc, t, _ = m.build(lib, [hand])
    assert rc == 0
    exp = check(m, t, [hand])
    assert [b for b, *_ in exp] == arm + [hand] and t.el.n == 8 and t.nsteps == 3           # the base is folded, the hand stays
    # the base folded into joint 1: p_f + R_f p, q_f q
    pf, qf = m.pos[base].astype(np.float64), m.quat[base].astype(np.float64)
    want = pf + rotm(qf / np.linalg.norm(qf)) @ m.pos[arm[0]].astype(np.float64) * (qf @ qf)
    assert one_rounding(t.el.pos[0][:], want) and one_rounding(t.el.quat[0][:], qmul(qf, m.quat[arm[0]].astype(np.float64)))
    assert (t.el.jtype[7], t.el.qcol[7]) == (FIXED, -1) and list(t.el.pos[7]) == list(m.pos[hand]) and list(t.el.quat[7]) == list(m.quat[hand])
    assert list(t.anc[0][:8]) == [-1, 0, 1, 2, 3, 4, 5, 6] and t.anc_mask[0] == 0xff and t.link_lane[0] == 7
    assert t.n_arm == 9 and t.moving_cols == 0x7f


def test_fingers_with_and_without_the_hand_as_a_link(lib):
    m, base, arm, hand, lf, rf = panda()
    rc, t, _ = m.build(lib, [lf, rf])
    assert rc == 0
    exp = check(m, t, [lf, rf])
    assert [b for b, *_ in exp] == arm + [lf, rf] and t.el.n == 9                            # the hand is folded into BOTH fingers
    assert t.par_el[7] == 6 and t.par_el[8] == 6 and t.moving_cols == 0x1ff
    rc, t, _ = m.build(lib, [hand, lf, rf])
    assert rc == 0
    exp = check(m, t, [hand, lf, rf])
    assert [b for b, *_ in exp] == arm + [hand, lf, rf] and t.el.n == 10                     # a link is never folded
    assert t.par_el[8] == 7 and t.par_el[9] == 7
    assert list(t.el.pos[8]) == list(m.pos[lf]) and list(t.el.pos[9]) == list(m.pos[rf])
    rc, t, _ = m.build(lib, [lf, hand])                                                      # ... wherever it stands in the list
    assert rc == 0 and t.el.n == 9 and (t.link_lane[0], t.link_lane[1]) == (8, 7)
    check(m, t, [lf, hand])


def test_pointer_doubling_on_a_chain_of_sixteen_and_on_a_branching_tree(lib):
    m = Model()
    ch = m.chain(0, [REVOLUTE, PRISMATIC] * 8)
    rc, t, _ = m.build(lib, [ch[-1]])
    assert rc == 0 and t.el.n == 16 and t.nsteps == 4
    check(m, t, [ch[-1]])
    for s in range(4):
        assert list(t.anc[s]) == [i - 2 ** s if i >= 2 ** s else -1 for i in range(G)]
    m = Model()
    trunk = m.chain(0, [REVOLUTE] * 3)
    a = m.chain(trunk[-1], [REVOLUTE, FIXED, PRISMATIC, REVOLUTE])     # (a fixed body inside a branch: folded)
    b = m.chain(trunk[1], [PRISMATIC] * 6)                             # (a second branch from further up, the deepest)
    rc, t, _ = m.build(lib, [a[-1], b[-1], trunk[-1]])
    assert rc == 0 and t.el.n == 12 and t.nsteps == 3
    check(m, t, [a[-1], b[-1], trunk[-1]])


def test_a_chain_of_exactly_one_element(lib):
    m = Model()
    j = m.add(0, REVOLUTE)
    rc, t, _ = m.build(lib, [j])
    assert rc == 0 and t.el.n == 1 and t.nsteps == 0 and t.link_lane[0] == 0 and t.anc_mask[0] == 1
    check(m, t, [j])
    m, base, arm, *_ = panda()                      # ... and one element after folding: the first arm link behind the fixed base
    rc, t, _ = m.build(lib, [arm[0]])
    assert rc == 0 and t.el.n == 1 and t.nsteps == 0 and t.par_el[0] == -1
    check(m, t, [arm[0]])


def test_refusals(lib):
    m = Model()
    ch = m.chain(0, [REVOLUTE] * 17)
    rc, _, what = m.build(lib, [ch[-1]])
    assert rc == CAPACITY and what == "more than 16 elements"
    assert m.build(lib, [ch[15]])[0] == 0
    m = Model()
    f = m.add(0, FREE)
    ch = m.chain(f, [REVOLUTE] * 2)
    rc, _, what = m.build(lib, [ch[-1]])
    assert rc == INVALID and what == "the link hangs off a free body"
    for bad in (0, -1, len(m.parent)):
        rc, _, what = m.build(lib, [bad])
        assert rc == INVALID and what == "link out of range"


def test_dof_mask_clears_the_masked_columns_only(lib):
    m, base, arm, hand, lf, rf = panda()
    mask = [1, 0, 1, 1, 0, 1, 1, 0, 1]
    rc, t, _ = m.build(lib, [lf, rf], mask)
    assert rc == 0
    check(m, t, [lf, rf], mask)
    assert list(t.moving[:9]) == mask and t.moving_cols == sum(b << k for k, b in enumerate(mask))
    rc, t, _ = m.build(lib, [hand], mask)          # (the fingers' columns are off the chain whatever the mask says)
    assert rc == 0 and t.moving_cols == 0b1101101
    check(m, t, [hand], mask)


def test_two_links_that_share_their_first_four_elements(lib):
    m = Model()
    trunk = m.chain(0, [REVOLUTE] * 4)
    a = m.chain(trunk[-1], [REVOLUTE] * 2)
    b = m.chain(trunk[-1], [PRISMATIC] * 3)
    rc, t, _ = m.build(lib, [a[-1], b[-1]])
    assert rc == 0 and t.el.n == 9
    check(m, t, [a[-1], b[-1]])
    # by depth, then body: trunk 0-3, a1 b1, a2 b2, b3
    assert (t.link_lane[0], t.link_lane[1]) == (6, 8)
    assert t.anc_mask[0] == 0b001010000 | 0xf and t.anc_mask[1] == 0b110100000 | 0xf
    assert t.anc_mask[0] & t.anc_mask[1] == 0xf
