"""The deal of a grouped weight-gradient launch (net.hip wg_deal through udapose_wgrad_deal), a pure host function: which XCD's list holds a
(layer, split) unit and where.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from uda_poseestimation_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "uda_poseestimation_amd", "csrc"), "-j8"], check=True)
    return _hip.lib()


def _units_like_the_benched_plan(rng):
    """(nblk, stages) shaped like the 128x128 class of PoseResNet-101 at N = 32, 256 x 256 (profiles/tail_timeline.txt): almost every unit
    reduces 128 stages - layer3's unsplit layers (16 - 36 work-groups each) and the 128-stage splits of layer1 / layer2 / the deconvolutions -
    and only layer4's eight layers are short (32 stages, 64 - 512 work-groups); plus random extras so that the test does not hang on one
    hand-made list."""
    units = [(256, 128), (64, 128)]                       # deconvolutions
    units += [(512, 32), (144, 32), (128, 32)] + [(64, 32)] * 5       # layer4
    for _ in range(23):
        units += [(16, 128), (16, 128)]                   # layer3 bottleneck 1x1s
    units += [(36, 128), (32, 128), (32, 128)]
    for _ in range(4):
        units += [(16, 128)] * 2 + [(36, 128)]            # layer2 splits
    units += [(4, 40), (9, 17)]                           # (remainder splits)
    for _ in range(int(rng.integers(0, 20))):
        units.append((int(rng.integers(1, 150)), int(rng.integers(1, 129))))
    return units


def _deal(lib, units, order):
    """-> per-XCD lists of (unit, first, count) runs in list order, modelled finish times"""
    n = len(units)
    nblk = (C.c_int * n)(*[u[0] for u in units])
    st = (C.c_int * n)(*[u[1] for u in units])
    cap = sum(u[0] for u in units)
    ex, eu, ef, ec, fin = (C.c_int * cap)(), (C.c_int * cap)(), (C.c_int * cap)(), (C.c_int * cap)(), (C.c_double * 8)()
    ne = lib.udapose_wgrad_deal(nblk, st, n, order, ex, eu, ef, ec, cap, fin)
    assert 0 < ne <= cap
    lists = [[] for _ in range(8)]
    for i in range(ne):
        assert 0 <= ex[i] < 8
        lists[ex[i]].append((eu[i], ef[i], ec[i]))
    return lists, list(fin)


def _model_finish(units, runs, slots=128):
    """The model, restated: work-groups start in list order, each on the slot that frees first, and take stages + 4."""
    import heapq
    free = [0.0] * slots
    heapq.heapify(free)
    end = 0.0
    for u, _, cnt in runs:
        for _ in range(cnt):
            t = heapq.heappop(free) + units[u][1] + 4
            heapq.heappush(free, t)
            end = max(end, t)
    return end


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("order", [0, 1])
def test_every_work_group_is_dealt_exactly_once(lib, order, seed):
    units = _units_like_the_benched_plan(np.random.default_rng(seed))
    lists, fin = _deal(lib, units, order)
    seen = [np.zeros(u[0], dtype=int) for u in units]
    for k in range(8):
        for u, first, cnt in lists[k]:
            assert cnt >= 1 and first >= 0 and first + cnt <= units[u][0]
            seen[u][first:first + cnt] += 1           # (a run is consecutive work-groups of ONE unit, contiguous in ONE list)
            if order == 0:
                assert (first, cnt) == (0, units[u][0])       # (the parent's deal keeps units whole)
            else:
                assert cnt <= 32
        assert abs(_model_finish(units, lists[k]) - fin[k]) < 1e-9
    assert all((s == 1).all() for s in seen)


@pytest.mark.parametrize("seed", range(6))
def test_new_order_runs_long_work_groups_first_and_levels_the_finish_times(lib, seed):
    """Order 1: inside a list the stages per work-group never increase (so a list ends with its shortest work-groups), and the modelled finish
    times are level.  The bound is reasoned, not observed: dealing runs to the least loaded list keeps the lists' summed loads within one
    run's load of each other whatever the dealing order - here at most 32 work-groups of the longest kind, i.e. 32 x longest / 128 slots in
    time - and a list started in order on 128 slots ends between its load / 128 and that plus one work-group lifetime."""
    units = _units_like_the_benched_plan(np.random.default_rng(seed))
    lists, fin = _deal(lib, units, 1)
    for k in range(8):
        st = [units[u][1] for u, _, _ in lists[k]]
        assert st == sorted(st, reverse=True), (k, st)
    longest = max(s + 4 for _, s in units)
    assert max(fin) - min(fin) <= 32 * longest / 128.0 + longest, (fin, longest)
    total = sum(n * (s + 4) for n, s in units)
    assert max(fin) <= total / (8 * 128.0) + 32 * longest / 128.0 + longest
    # every XCD gets its share of every kind of work-group: the short ones (<= 32 stages) are spread over all eight lists
    short = [sum(cnt for u, _, cnt in lists[k] if units[u][1] <= 32) for k in range(8)]
    assert min(short) > 0 and max(short) - min(short) <= max(64, sum(short) // 16), short


def test_deal_rejects_bad_arguments(lib):
    one = (C.c_int * 1)(1)
    zero = (C.c_int * 1)(0)
    assert lib.udapose_wgrad_deal(one, one, 1, 2, None, None, None, None, 0, None) < 0
    assert lib.udapose_wgrad_deal(zero, one, 1, 1, None, None, None, None, 0, None) < 0
    assert lib.udapose_wgrad_deal(one, one, 1, 1, None, None, None, None, 0, None) == 1
