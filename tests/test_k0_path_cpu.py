"""The method of the 3-DoF initialiser's interior-point path comparison (tests/k0_path_reference.py, tests/test_gpu_k0_path.py), checked
without a GPU on the CPU twin alone:

  * yardstick drift: the yardstick recomputed here agrees with tests/golden/k0_path_yardstick.npz within a factor of 3 (the native
    build differs from machine to machine: nothing tighter means anything), above an absolute 1e-15 (depth 1 sits on single
    roundings) -- at depth 1, over the other truncated depths and, for the cases with K >= 3, at full depth; the parity twin's statuses and iteration counts equal the fixture's at every depth; its two builds agree on every
    status and meet the iteration-count rule the device is held to (cases with K >= 3) -- K = 1 and 2 end optimal or almost optimal
    on both;
  * depths: a solve stopped by max_iter = n < 13 ends on the iteration cap with n iterations on every start, so a truncated depth
    compares iterates and never a finished solve; depth 1 is sharp -- Y below 1e-13 in every group of every case;
  * the random class is the first of the eight drawn whose starts all end optimal on the twin;
  * mutation: the twin without its refinement pass (refine = 0 against 1) leaves max(10 Y, floor) by a factor of more than 1000 at
    depth 1 on the flyable K = 30 case and ends every full solve optimal with the objective within the 1e-9 of
    tests/test_gpu_threedof.py: the path bound sees what the end bounds do not."""
import numpy as np
import pytest

import k0_path_reference as kp

_MEASURED = {}


def _measure(case):
    if case not in _MEASURED:
        _MEASURED[case] = kp.measure(case)
    return _MEASURED[case]


@pytest.mark.parametrize("case", list(kp.CASES))
def test_yardstick_agrees_with_the_fixture(case):
    g = np.load(kp.FIXTURE)
    assert tuple(g["depths"]) == kp.DEPTHS and tuple(g["groups"]) == kp.GROUPS and list(g["cases"]) == list(kp.CASES)
    m = _measure(case)
    k = kp.key(case)
    assert np.array_equal(m["iters"], g["iters_" + k]) and np.array_equal(m["status"], g["status_" + k])
    assert np.allclose(m["mag"], g["mag_" + k], rtol=1e-6, atol=1e-12)
    if case in kp.COUNTED:
        assert np.array_equal(m["status"], m["native_status"]) and np.array_equal(g["status_" + k], g["native_status_" + k])
    else:
        for st in (m["status"][-1], m["native_status"][-1], g["status_" + k][-1], g["native_status_" + k][-1]):
            assert np.all(np.isin(st, (0, 4))), st
        assert np.array_equal(m["status"][:-1], m["native_status"][:-1])
    Y, Yf = np.maximum(m["native"], m["perturb"]), kp.yardstick(case, g)
    # per group: depth 1, the largest over the other truncated depths, and the full depth (the table in tests/test_gpu_k0_path.py)
    # The full-depth row of K = 1 and 2 is left out: which starts the two builds finish in the same number of iterations there depends
    # on the CPU the native build is made for, so that row cannot be re-derived within any factor (it is no bound either).
    rows = lambda a: np.stack([a[0], a[1:-1].max(axis=0)] + ([] if case in kp.TINY else [a[-1]]))   # noqa: E731
    ratio = np.maximum(rows(Y), 1e-15) / np.maximum(rows(Yf), 1e-15)
    print("%s: yardstick here / fixture between %.2f and %.2f; depth 1 %s" % (case, ratio.min(), ratio.max(), " ".join("%.1e" % v for v in Y[0])))
    assert ratio.max() <= 3.0 and ratio.min() >= 1.0 / 3.0, ratio


def test_the_twins_two_builds_meet_the_iteration_count_rule():
    g = np.load(kp.FIXTURE)
    here, fixed = [], []
    for case in kp.COUNTED:
        m = _measure(case)
        k = kp.key(case)
        assert np.all(m["status"][-1] == 0) and np.all(m["native_status"][-1] == 0)
        here += list(zip(m["iters"][-1], m["native_iters"][-1]))
        fixed += list(zip(g["iters_" + k][-1].astype(int), g["native_iters_" + k][-1].astype(int)))
    for pairs in (here, fixed):
        differ, total, worst, holds = kp.count_rule(pairs)
        print("full solves on which the twin's two builds take another iteration count: %d of %d (largest difference %d)" % (differ, total, worst))
        assert total == kp.B * len(kp.COUNTED) and holds, (differ, total, worst)


@pytest.mark.parametrize("case", list(kp.CASES))
def test_truncated_depths_stop_on_the_cap_and_depth_one_is_sharp(case):
    m = _measure(case)
    for i, n in enumerate(kp.DEPTHS[:-1]):
        for st, its in ((m["status"][i], m["iters"][i]), (m["native_status"][i], m["native_iters"][i])):
            assert np.all(st == 1) and np.all(its == n), (n, st, its)
    Y1 = np.maximum(m["native"], m["perturb"])[0]
    assert Y1.max() < 1e-13, dict(zip(kp.GROUPS, Y1))
    assert kp.yardstick(case)[0].max() < 1e-13


def test_random_class_is_the_first_whose_starts_are_all_optimal():
    import oracle
    from oracle import model, port
    oracle.use_native(False)
    first = None
    for n, po in enumerate(kp.random_classes()):
        _, st, _ = port.threedof(po, model.disperse_ics(po, kp.B, kp.SEED))
        if np.all(st == 0):
            first = n
            break
    assert first == kp.RANDOM_CLASS, first


def test_missing_refinement_shows_on_the_path_and_not_at_the_end():
    import oracle
    from oracle import port
    oracle.use_native(False)
    case = "flyable K=30"
    po, ic = kp.problem(case)
    Y = kp.yardstick(case)
    res = {}
    for i, n in enumerate(kp.DEPTHS):
        for refine in (1, 0):
            res[refine] = kp.as_run(*port.threedof(po, ic, max_iter=n, refine=refine))
        bound = np.maximum(kp.FACTOR * Y[i], kp.floor(po.K, kp.magnitudes(res[1])))
        dist = kp.distance(res[1], res[0])
        ratio = float(kp.ratios(dist, bound)[:8].max())
        print("depth %2d: refine 0 against 1, worst minimiser group at %.1e x max(10 Y, floor); iterations %s / %s" % (n, ratio, res[1]["iters"], res[0]["iters"]))
        if n == 1:
            first = ratio
    assert first > 1000.0, first
    assert np.all(res[1]["status"] == 0) and np.all(res[0]["status"] == 0)
    assert (np.abs(res[1]["pobj"] - res[0]["pobj"]) / np.maximum(1.0, np.abs(res[1]["pobj"]))).max() <= 1e-9
