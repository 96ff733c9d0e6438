"""The 3-DoF initialiser's kernel (K0: threedof_kernel) against its CPU twin ALONG the interior-point path, on the MI355X.

tests/test_gpu_threedof.py compares finished solves: statuses, iteration counts "within 1", objectives to 1e-8 ... 1e-9 and minimisers
to 1e-7 ... 2e-4.  An interior-point method corrects itself (tests/test_gpu_k4_path.py), so that is next to blind to a band entry
dropped by a register sweep, a chunk mis-padded at the end of the band or a lane left out of a reduction -- and those are the parts
of K0 that no CPU build runs (WaveEx3::band_sweeps with kRegisterSweep = true, the 64-lane butterflies, lanes that own several rows of
the long cone at K = 100; the twin has one lane and the plain sweeps).  Here every solve is also stopped by max_iter = n for n = 1, 2,
3, 4, 6, 8, 10, 12 (n - 1 Newton steps; n = 1 is the start point: one band factorisation at W = I and one kkt_solve through both
sweeps) and compared with the parity twin stopped at the same depth.

Cases (tests/k0_path_reference.py), B = 4 dispersed starts each: the flyable problem at K = 1, 2, 3, 30, 100 -- band lengths on
either side of one 64-column round of the sweeps, just past it, the usual size and the long cone with more rows than lanes --
config0 at K = 30 and the first all-optimal random class of test_device_random_instances_match_twin.

Bounds, none of them taken from the device (fixture tests/golden/k0_path_yardstick.npz written by
tests/golden/make_k0_path_yardstick.py from the twin alone; tests/test_k0_path_cpu.py keeps it honest):
  * truncated depths: status and iteration count equal the parity twin's; every group (T, r, v, ma, ga, kaR, ar, nkaR absolute; pobj
    relative; gap, pres, dres relative to the larger value) within max(10 Y(case, n, group), floor), Y = the larger of parity-vs-native
    build of the twin and parity twin vs itself on starts perturbed by one ulp relative, floor = 2^-52 (K+1) 15 max|entry of the
    group| (K4's convention for re-ordered sums: the device contracts and reduces over 64 lanes).  The factor 10 is the convention of
    tests/test_k4_fused_sweeps_twin.py;
  * full depth (max_iter 60): status equal to the twin's; over all (case, start) pairs of the cases with K >= 3 at most 5 % may take
    another iteration count than the twin and none may differ by more than 1 (the twin's two builds: 0 of 20; the fixture maker refuses
    to write otherwise).  K = 1 and 2 are outside the count rule -- the twin's own builds differ there on 16 of 64 starts by up to 4
    and on which starts depends on the CPU the native build is made for, so a full-depth yardstick there is the luck of one build
    -- and are held at full depth to the finished-solve bounds alone: status in (0, 4) and the objective within 2e-7 relative
    (tests/test_threedof_twin.py), and where both sides end optimal the objective within 1e-8 and the minimiser within 2e-4
    (tests/test_gpu_threedof.py::test_device_tiny_horizons).  At K >= 3 starts with the twin's count meet 10 Y(case, full), Y taken
    over the starts on which the two runs compared take the same count; starts with another count meet the finished-solve bounds
    of tests/test_gpu_threedof.py (objective 1e-8 relative, minimiser 2e-4).

Y as recorded (largest over T, r, v, ma, ga, kaR, ar, nkaR | pobj), written out so that the bounds do not move with the file:

    case            depth 1            depths 2 - 12      full
    flyable K=1     1.1e-15 | 0.0e+00   9.9e-06 | 1.3e-06   (no bound)
    flyable K=2     1.7e-15 | 0.0e+00   2.7e-06 | 6.9e-07   (no bound)
    flyable K=3     1.1e-15 | 0.0e+00   9.8e-06 | 3.0e-06   1.2e-07 | 1.1e-13
    flyable K=30    2.7e-15 | 0.0e+00   2.3e-09 | 1.1e-10   9.7e-10 | 2.0e-14
    flyable K=100   6.2e-15 | 0.0e+00   9.1e-11 | 6.7e-12   3.9e-10 | 2.2e-15
    config0 K=30    1.4e-14 | 0.0e+00   1.8e-10 | 3.8e-13   1.4e-09 | 1.2e-15
    random class    4.0e-15 | 0.0e+00   7.3e-10 | 1.1e-09   6.9e-09 | 2.9e-15

Depth 1 pins the device-only factorisation and sweeps about a million times tighter than anything else in the suite; at K <= 3 the
first Newton step amplifies one ulp by 1e9, so those horizons are pinned at depth 1 and only as far as the yardstick allows beyond.

Measured on one MI355X when the test was added (profiles/k0_path_parity.md): every status and truncated iteration count equal, 0 of the
20 full solves with K >= 3 with another iteration count than the twin, worst distance / bound 0.23 (depth 1: 0.10; full depth at K >= 3: 0.19; the finished solves of K = 1 and 2: 0.07 of the 1e-8 on the objective, 0.06 of the 2e-4 on the minimiser);
kaR at the start point is exactly zero on both sides (its bound there is zero).

Every comparison prints one markdown row (case, depth, group, distance, bound, ratio) before it asserts: profiles/k0_path_parity.md."""
import numpy as np
import pytest

import k0_path_reference as kp

pytestmark = pytest.mark.gpu

_RUNS = {}          # case -> list of rows; filled once per case


def run(case):
    """every depth of one case: the device and the parity twin.  Nothing is asserted here."""
    if case in _RUNS:
        return _RUNS[case]
    import oracle
    oracle.use_native(False)
    po, ic = kp.problem(case)
    Y = kp.yardstick(case)
    c = kp.device_cache(po)
    rows = []
    try:
        _depths(case, c, po, ic, Y, rows)
    finally:
        c.close()
    _RUNS[case] = rows
    return rows


def _depths(case, c, po, ic, Y, rows):
    from successiveconvexification_amd import first_round
    for i, n in enumerate(kp.DEPTHS):
        dev = kp.as_run(*first_round.solve_initial_batch(c, ic, max_iter=n))
        tw = kp.run_twin(po, ic, n)
        bound = np.maximum(kp.FACTOR * Y[i], kp.floor(po.K, kp.magnitudes(tw))) if n != kp.FULL else kp.FACTOR * Y[i]
        per = np.array([kp.distance(dev, tw, np.arange(kp.B) == t) for t in range(kp.B)])
        rows.append(dict(depth=n, K=po.K, dist=kp.distance(dev, tw), per=per, bound=bound, st=dev["status"], its=dev["iters"], tst=tw["status"],
                         tits=tw["iters"], pobj=dev["pobj"], tpobj=tw["pobj"],
                         linf=np.array([max(np.abs(dev[k][t] - tw[k][t]).max() for k in kp.KEYS) for t in range(kp.B)])))


def _report(case, r):
    """the markdown rows of one depth; returns the worst ratio of a distance to its bound (full depth: over the starts with the twin's
    iteration count, each against 10 Y)"""
    full = r["depth"] == kp.FULL
    if full and case in kp.TINY:     # finished solves of K = 1 and 2: the finished-solve bounds alone
        rel, both = _rel_pobj(r), (r["st"] == 0) & (r["tst"] == 0)
        q = [(rel.max(), kp.TINY_POBJ, "pobj, every start"), (rel[both].max(initial=0.0), kp.OTHER_COUNT_POBJ, "pobj, both optimal"),
             (r["linf"][both].max(initial=0.0), kp.OTHER_COUNT_LINF, "minimiser, both optimal")]
        for dist, bound, g in q:
            print("| %s | full | %s | %.1e | %.1e | %.2f |" % (case, g, dist, bound, dist / bound))
        return float(max(dist / bound for dist, bound, _ in q))
    same = (r["its"] == r["tits"]) & (r["st"] == r["tst"])
    d = r["per"][same].max(axis=0) if full and same.any() else (np.zeros(len(kp.GROUPS)) if full else r["dist"])
    ratio = kp.ratios(d, r["bound"])
    for g, dist, bound, q in zip(kp.GROUPS, d, r["bound"], ratio):
        print("| %s | %s | %s | %.1e | %.1e | %.2f |" % (case, "full" if full else r["depth"], g, dist, bound, q))
    return float(ratio.max())


def _rel_pobj(r):
    return np.abs(r["pobj"] - r["tpobj"]) / np.maximum(1.0, np.abs(r["tpobj"]))


@pytest.mark.parametrize("case", list(kp.CASES))
def test_device_takes_the_twins_path(case):
    rows = run(case)
    print("\n| case | depth | group | distance | bound | ratio |\n|---|---|---|---|---|---|")
    ratios = [_report(case, r) for r in rows]
    print("%s: worst ratio of a device / twin distance to its bound %.2f at depth 1, %.2f at depths 2 - 12, %.2f at full depth; iterations "
          "of the full solves %s, the twin's %s; statuses %s / %s"
          % (case, ratios[0], max(ratios[1:-1]), ratios[-1], rows[-1]["its"], rows[-1]["tits"], rows[-1]["st"], rows[-1]["tst"]))
    for r in rows:
        n = r["depth"]
        if n != kp.FULL:
            assert np.array_equal(r["st"], r["tst"]) and np.array_equal(r["its"], r["tits"]), (n, r["st"], r["tst"], r["its"], r["tits"])
            assert np.all(r["dist"] <= r["bound"]), (n, dict(zip(kp.GROUPS, kp.ratios(r["dist"], r["bound"]))))
            continue
        rel = _rel_pobj(r)
        if case in kp.TINY:
            both = (r["st"] == 0) & (r["tst"] == 0)
            assert np.all(np.isin(r["st"], (0, 4))) and np.all(np.isin(r["tst"], (0, 4))), (r["st"], r["tst"])
            assert np.all(rel <= kp.TINY_POBJ), rel
            assert np.all(rel[both] <= kp.OTHER_COUNT_POBJ) and np.all(r["linf"][both] < kp.OTHER_COUNT_LINF), (rel, r["linf"])
            continue
        assert np.array_equal(r["st"], r["tst"]) and np.all(r["st"] == 0), (r["st"], r["tst"])
        assert np.abs(r["its"] - r["tits"]).max() <= 1, (r["its"], r["tits"])      # how MANY may differ: the test below
        for t in range(kp.B):
            if r["its"][t] == r["tits"][t]:
                assert np.all(r["per"][t] <= r["bound"]), (t, dict(zip(kp.GROUPS, kp.ratios(r["per"][t], r["bound"]))))
            else:
                assert rel[t] <= kp.OTHER_COUNT_POBJ and r["linf"][t] < kp.OTHER_COUNT_LINF, (t, rel[t], r["linf"][t])


def test_iteration_counts_of_full_solves_equal_the_twins_within_the_cap():
    """over all (case, start) pairs of the cases with K >= 3: at most 5 % of the full solves take another iteration count than the
    twin, and none differs by more than 1.  A condition, not a measurement: the twin's two builds differ in 0 of 20."""
    pairs = []
    for case in kp.COUNTED:
        r = run(case)[-1]
        assert r["depth"] == kp.FULL
        pairs += list(zip(r["its"], r["tits"]))
    differ, total, worst, holds = kp.count_rule(pairs)
    print("full solves with another iteration count than the twin: %d of %d (largest difference %d)" % (differ, total, worst))
    assert holds, (differ, total, worst)
