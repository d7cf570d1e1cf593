"""CPU tier: the routing decisions of exact contacts (gym-genesis_amd/csrc/mir_route.h) compiled with plain g++
(tests/route_host.cpp, `make route-host`) and called through ctypes.  Every route computes the same bits, so the GPU twin tests cannot
see a wrong decision -- it shows only as a slower step.  Here the rules are spelled out once more, independently of the header, and
compared case by case: plan_begin over every combination of its inputs, the phase transitions and the statistics of close_step, and
the front / back partition that orders the envs of the next launch."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL, POST, ROTATED, HEAVY48, POST48, ROTATED_LIST = 2, 4, 5, 7, 9, 11   # StepKind (mir_step.h)
GAP = 40.0


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "gym-genesis_amd", "csrc"), "route-host"], stdout=subprocess.DEVNULL)
    L = C.CDLL(os.path.join(ROOT, "tests", "_build", "libmirroute.so"))
    L.route_plan_begin.restype = None
    L.route_close_step.restype = None
    return L


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def test_plan_begin_every_combination(lib):
    """exact x big_on x split_step x sync_mode x gap (none / below / at the threshold) x the twelve yes/no inputs: 995 328 cases in one
    call; the expected plan is the rule list of the design, written here with numpy."""
    axes = [(0, 1, 2), (0, 1, 2), (0, 1, 2), (0, 2, 3), (-1.0, GAP - 0.5, GAP), (GAP,)] + [(0, 1)] * 12
    idx = np.indices([len(a) for a in axes], dtype=np.int8).reshape(18, -1)
    n = idx.shape[1]
    cases = np.empty((18, n), np.float32)   # (one column per input)
    for i, a in enumerate(axes):
        cases[i] = np.asarray(a, np.float32)[idx[i]]
    assert n == 3 ** 5 * 2 ** 12
    out = np.zeros((n, 8), np.int32)
    lib.route_plan_begin(_ptr(cases, C.c_float), C.c_int(n), _ptr(out, C.c_int32))
    (exact, big_on, split_step, sync_mode, gap, _, exact_big, bigmode, heavy_phase, rt_ok, big_side, big_lists, pre_valid, same, fk_leaf,
     pre_big, side, next_host) = cases
    b = lambda a: a != 0  # noqa: E731
    eligible = ((exact == 1) & b(exact_big) & b(bigmode) & b(pre_big) & (sync_mode == 3) & b(side) & b(split_step) & b(pre_valid) & b(same)
                & b(fk_leaf))
    bigrot = eligible & ((big_on == 2) | ((gap >= 0) & (gap >= GAP)))
    heavy = b(exact) & b(exact_big) & b(heavy_phase) & (sync_mode == 3) & ~bigrot
    split = b(split_step) & (sync_mode != 2) & ~heavy
    have_pre = split & b(pre_valid) & b(same)
    rotated = have_pre & b(fk_leaf) & (split_step != 2) & ~bigrot
    kind = np.where(heavy, HEAVY48, np.where(bigrot, POST48, np.where(rotated, ROTATED, np.where(have_pre, POST, FULL))))
    lists = bigrot & b(rt_ok) & b(big_side) & b(next_host) & b(big_lists)
    perm = np.where(heavy | bigrot, 1, -1)   # (the driver sets perm_next = 1)
    want = np.stack([kind, heavy, bigrot, split, have_pre, rotated, lists, perm], 1).astype(np.int32)
    bad = np.nonzero((want != out).any(1))[0]
    assert bad.size == 0, (bad.size, cases[:, bad[0]], want[bad[0]], out[bad[0]])
    # (the enumeration reaches every launch and both answers of every flag)
    assert set(np.unique(kind)) == {FULL, POST, ROTATED, HEAVY48, POST48}
    assert all(0 < int(x.sum()) < n for x in (heavy, bigrot, split, have_pre, rotated, lists))
    # big_on == 1: the gap decides, and no previous end never qualifies
    one = eligible & (big_on == 1)
    assert not bigrot[one & (gap < GAP)].any() and bigrot[one & (gap >= GAP)].all()


def test_plan_lists(lib):
    k = C.c_int32(0)
    B = 30
    assert lib.route_plan_lists(POST48, 0, B, C.byref(k)) == 0 and k.value == ROTATED_LIST
    for nh in (B, B + 2):   # (padded to whole workgroups, the count can pass B)
        assert lib.route_plan_lists(POST48, nh, B, C.byref(k)) == 0 and k.value == POST48
    for nh in (4, 28):
        assert lib.route_plan_lists(POST48, nh, B, C.byref(k)) == 1 and k.value == POST48


class _Run:
    """a handle's phase and counters, steps closed one after the other"""

    def __init__(self, lib, exact_big=1, big_on=1, enter=0, leave=0, sort=1):
        self.lib = lib
        self.cfg = np.array([exact_big, big_on, enter, leave, sort], np.int32)
        self.phase = np.array([0, 0, -1, 0], np.int32)   # heavy, bigmode, perm_next, rt_ok
        self.stats = np.zeros(3, np.uint64)               # steps with overflow, overflow env-steps, most in a step

    def close(self, ndefer, nover, heavy=0, big=0, rt_ok=0):
        self.phase[3] = rt_ok
        self.phase[2] = 1   # (close_step forgets the order of the step before)
        out = np.zeros(2, np.int32)
        self.lib.route_close_step(_ptr(self.cfg, C.c_int32), _ptr(self.phase, C.c_int32), _ptr(np.array([heavy, big], np.int32), C.c_int32),
                                  _ptr(self.stats, C.c_uint64), C.c_int(ndefer), C.c_int(nover), _ptr(out, C.c_int32))
        assert self.phase[2] == (-1 if self.cfg[0] else 1)
        return bool(out[0]), int(out[1])

    @property
    def heavy(self):
        return int(self.phase[0])

    @property
    def bigmode(self):
        return int(self.phase[1])


def test_overflow_run_starts_behind_a_deferral_and_ends_with_a_clean_two_launch_step(lib):
    r = _Run(lib)
    assert r.bigmode == 0
    assert r.close(3, 0) == (True, 0x80) and r.bigmode == 1          # a light step that deferred: sort on "deferred"
    assert r.close(0, 5, big=1) == (True, 0x40) and r.bigmode == 1   # a two-launch step with envs above 16 points: on "above 16 points"
    assert r.close(0, 0, big=1)[0] is False and r.bigmode == 0       # a clean one ends the run: nothing to sort for
    assert list(r.stats) == [2, 8, 5]
    # a clean LIGHT step inside a run does not end it (the first-half launch of the run's next step decides), a deferral does not either
    r = _Run(lib)
    r.close(1, 0)
    r.close(0, 0)
    assert r.bigmode == 1
    r.close(2, 4, big=1)
    assert r.bigmode == 1
    # MIR_EXACT_BIG=0: never a run
    r = _Run(lib, big_on=0)
    assert r.close(9, 0)[0] is False and r.bigmode == 0


def test_heavy_phase_enters_at_the_threshold_and_leaves_below_the_other(lib):
    r = _Run(lib, big_on=0, enter=4, leave=2)
    assert r.close(3, 0) == (False, 0x80) and r.heavy == 0
    assert r.close(4, 0) == (True, 0x80) and r.heavy == 1              # enters on the envs a light step DEFERRED ...
    assert r.close(0, 2, heavy=1) == (True, 0x40) and r.heavy == 1     # ... stays while a heavy step has >= leave envs above 16 points
    assert r.close(7, 1, heavy=1)[0] is False and r.heavy == 0         # ... and leaves on ITS count of those, not on what it deferred
    assert list(r.stats) == [4, 10, 7]
    r = _Run(lib, big_on=0, enter=0, leave=0)
    for nd in (1, 30, 4096):
        assert r.close(nd, 0)[0] is False and r.heavy == 0             # enter == 0: never
    r = _Run(lib, exact_big=0, big_on=0, enter=1, leave=1)             # no list instantiation: no phases, the statistics alone
    assert r.close(5, 0) == (False, 0) and r.heavy == 0 and r.bigmode == 0 and list(r.stats) == [1, 5, 5]


def test_sort_is_suppressed_exactly_when_the_first_half_launch_gives_the_next_order(lib):
    for heavy_phase, bigmode, sort, big, rt_ok in itertools.product((0, 1), repeat=5):
        # thresholds that keep the phase where it is: enter above any count, leave 0; big_on 0 keeps bigmode
        r = _Run(lib, big_on=0, enter=10 ** 6, leave=0, sort=sort)
        r.phase[0], r.phase[1] = heavy_phase, bigmode
        got = r.close(1, 1, big=big, rt_ok=rt_ok)[0]
        assert got == bool((heavy_phase or bigmode) and sort and not (big and rt_ok and not heavy_phase))


def test_statistics_count_bit_6_of_a_heavy_or_two_launch_step_and_the_deferred_envs_of_a_light_one(lib):
    for heavy, big in ((0, 0), (1, 0), (0, 1)):
        r = _Run(lib)
        steps = [(0, 0), (3, 9), (0, 6), (2, 0), (0, 0)]
        for nd, no in steps:
            r.close(nd, no, heavy=heavy, big=big)
        cnt = [no if (heavy or big) else nd for nd, no in steps]
        # (the most in one step also sees the envs a heavy or two-launch step deferred, as it always has)
        assert list(r.stats) == [sum(c > 0 for c in cnt), sum(cnt), max(max(cnt), max(nd for nd, _ in steps))]
    r = _Run(lib)
    r.close(5, 2, heavy=1)
    assert list(r.stats) == [1, 2, 5]


@pytest.mark.parametrize("permuted", [False, True])
@pytest.mark.parametrize("bit,stride", [(0x40, 16), (0x80, 16), (0x01, 1)])
def test_partition_by_bit_30_envs(lib, permuted, bit, stride):
    """B = 30: the last workgroup holds two envs, and the two bytes behind them carry the bit -- they must not be read as envs."""
    B, nwg = 30, 8
    rng = np.random.default_rng(bit + stride)
    flags = rng.random(32) < 0.4
    flags[30:] = True
    assert 0 < flags[:B].sum() < B
    by = np.where(flags, bit, 0).astype(np.uint8) | (rng.integers(0, 64, 32).astype(np.uint8) & np.uint8(~bit & 0x3e))   # (tag bits around it)
    words = np.zeros(nwg * stride, np.uint32)
    words[::stride] = by.view(np.uint32)
    perm = rng.permutation(B).astype(np.int32) if permuted else None
    out = np.full(B + 2, -7, np.int32)
    nh = lib.route_partition_by_bit(_ptr(words, C.c_uint32), stride, _ptr(perm, C.c_int32) if permuted else None, B, C.c_uint32(bit), _ptr(out, C.c_int32))
    order = perm if permuted else np.arange(B, dtype=np.int32)
    front = order[flags[:B]]
    back = order[~flags[:B]]
    assert nh == front.size
    assert np.array_equal(out[:nh], front)                 # the envs with the bit: from the front, in scan order
    assert np.array_equal(out[nh:B], back[::-1])           # the others: packed from the back
    assert sorted(out[:B]) == list(range(B)) and (out[B:] == -7).all()
