"""The conic kernel (K4: socp_kernel_t / socp_block_kernel) against its CPU twin ALONG the interior-point path, on the MI355X.

An interior-point method corrects itself: a Newton direction that is slightly wrong costs an iteration or two and lands on the same
flat optimum, so a comparison of finished solves (1e-6 / 2e-6 / "counts within 1" elsewhere in the suite) is next to blind to a bad
element of an MFMA fragment map, a coupling tile off at one end of the two-ended chain or a reduction that drops a lane.  Here every
solve is also stopped after n = 1, 2, 3, 4, 6, 8, 10, 12 iterations (scvx_solver_opts.max_iter = n, retries = 0: the best iterate so
far, status 1) and compared with the parity twin stopped at the same depth, on the DEVICE'S OWN linearisation (K1 does not enter).

Bounds, none of them taken from the device (tests/k4_path_reference.py, fixture tests/golden/k4_path_yardstick.npz written by
tests/golden/make_k4_path_yardstick.py from the twin alone; tests/test_k4_path_cpu.py keeps the fixture honest and holds the depth
lists):
  * truncated depths: status and iteration count equal the twin's; every group (dx, du, dsigma, nu absolute; merit, pobj relative)
    within max(10 Y(case, n, group), floor), Y = the larger of parity-vs-native build of the twin and parity twin vs itself on inputs
    perturbed by one ulp relative, floor = 2^-52 (K+1) (14+2NU+1) max|entry of the group| -- the first-order bound on re-ordering the
    longest sums the start point goes through (the depth-1 yardstick is 1e-16; the device contracts and sums in MFMA order).  The
    factor 10 is the convention of tests/test_k4_fused_sweeps_twin.py;
  * full depth (max_iter 60): status 0 on both sides; iteration counts equal the twin's, with the cap of the last test -- over all
    (case, executor, trajectory) triples at most 5 % may differ and none by more than 1 (the twin's two builds: 0 of 320);
    trajectories with equal counts meet 10 Y(case, full), those with another count the 1e-6 of test_gpu_scvx.py;
  * a trajectory the twin reports infeasible at node 1 (status 5; two of the eight starts of the fuzz class) is compared by status only.
The aero case uses the yardstick of a CPU aero linearisation (oracle.dynamics with the spline tables), not the exo K = 50 one.

Y per case as recorded (largest over the depths <= 12 | full depth), written out so that the bounds do not move with the file:

    case                      dx       du       dsigma   nu       merit    pobj    |  dx       du       dsigma   nu       merit    pobj
    exo K=50                  2.4e-10  6.1e-11  6.3e-11  8.5e-13  2.8e-09  4.3e-11 |  8.7e-10  9.2e-10  3.2e-11  1.0e-11  4.9e-04  2.3e-13
    exo K=4                   2.5e-10  5.4e-11  1.1e-11  8.2e-12  3.1e-07  5.9e-12 |  8.3e-09  1.8e-09  2.9e-10  8.2e-11  7.3e-05  8.6e-14
    exo K=8                   2.4e-10  4.7e-11  1.4e-11  2.9e-12  1.1e-06  1.3e-11 |  4.6e-10  8.5e-11  7.5e-11  9.9e-11  3.4e-04  1.1e-13
    exo K=9                   1.6e-10  3.3e-11  2.1e-11  4.2e-12  1.2e-06  1.9e-11 |  4.5e-10  5.6e-11  2.4e-11  4.5e-10  1.9e-04  8.3e-14
    exo K=31                  2.2e-10  1.2e-10  3.7e-11  2.4e-12  5.5e-08  3.7e-11 |  6.3e-10  4.2e-10  3.0e-11  1.5e-11  6.7e-05  3.4e-15
    fins K=50                 4.7e-10  2.2e-10  9.5e-11  1.3e-12  2.0e-08  4.7e-11 |  2.8e-10  3.2e-10  1.6e-11  1.4e-11  6.2e-05  2.8e-14
    fins K=9                  2.2e-10  4.6e-11  1.7e-11  6.1e-12  1.5e-06  1.9e-11 |  3.3e-09  6.2e-10  6.2e-11  2.0e-10  4.6e-04  1.5e-13
    fuzz class 3 (dp cone)    2.1e-12  8.6e-13  1.1e-11  3.2e-14  1.1e-09  3.7e-12 |  2.8e-10  2.8e-10  5.0e-11  2.5e-13  1.1e-05  4.0e-15
    float tiles               1.8e-10  5.2e-11  5.6e-11  8.4e-13  2.9e-09  4.9e-11 |  8.5e-10  9.0e-10  3.9e-11  1.1e-11  5.4e-04  2.6e-13
    aero K=50                 2.1e-10  6.8e-11  4.8e-11  8.6e-13  2.3e-09  4.0e-11 |  1.8e-09  1.9e-09  5.6e-11  2.2e-11  8.2e-04  3.9e-13
    thrust back-offs          8.9e-10  2.6e-10  6.7e-10  2.2e-12  8.3e-09  4.2e-10 |  5.4e-11  1.1e-11  1.9e-12  3.1e-14  1.2e-05  2.9e-14
    (all 11 cases x 9 depths: iteration counts and statuses identical between the twin's two builds)

Measured on one MI355X when the test was added (profiles/k4_path_parity.md): every status and truncated iteration count equal, 0 of 237 full
solves with another iteration count than the twin, worst distance / bound 0.37 (1 / 2 / 4 wavefronts: 0.22 / 0.37 / 0.33) -- the two-ended
executors need no bound of their own.

Every comparison prints its figures before it asserts (one markdown row per case, executor and depth: profiles/k4_path_parity.md)."""
import ctypes as C

import numpy as np
import pytest

import k4_path_reference as kp

pytestmark = pytest.mark.gpu

WAVES = ("1", "2", "4")
_RUNS = {}          # (case, waves) -> list of rows; filled once per pair


def _set_depth(b, n):
    from successiveconvexification_amd import _lib
    o = _lib.ScvxSolverOpts()
    b._L.scvx_solver_default_opts(C.byref(o))
    o.max_iter, o.retries = int(n), 0
    _lib.check(b.cache.handle, b._L.scvx_batch_set_solver(b.handle, C.byref(o)), "scvx_batch_set_solver")


def _run(case, waves):
    """every depth of one case on one executor: the device and the parity twin on the device's linearisation.  Returns rows of
    dict(depth, dist, bound, status / iters of both sides, keep, per-trajectory distance at full depth); nothing is asserted here."""
    if (case, waves) in _RUNS:
        return _RUNS[(case, waves)]
    import oracle
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache
    oracle.use_native(False)
    spec = kp.CASES[case]
    po, ic, marg, nsub = kp.oracle_problem(case)
    pp = kp.device_problem(case)
    B, K, NU = ic.shape[0], po.K, po.nu
    Y = kp.yardstick(case)
    c = IntegratorCache(pp, npts=nsub)
    b = ScvxBatch(c, B)
    if spec.get("lin32"):
        b.set_linearization_f32(True)
    b.init(ic)
    if marg is not None:
        b.set_thrust_margins(marg[..., 0], marg[..., 1])
    xb, ub, sg = b.trajectory()
    e, d = b.linearization()
    rows = []
    for n in kp.depths_of(case):
        _set_depth(b, n)
        x, u, snew, nu = b.socp_solve()
        st, its, merit, pobj = b.solver_stats()
        tw = kp.run_twin(case, po, ic, marg, xb, ub, e, d, n)
        keep = tw["status"] != 5
        dev = dict(dx=x, du=u, ds=snew, nu=nu, merit=merit, pobj=pobj)
        ref = dict(dx=xb + tw["dx"], du=ub + tw["du"], ds=sg + tw["ds"], nu=tw["nu"], merit=tw["merit"], pobj=tw["pobj"])
        i = kp.DEPTHS.index(n)
        bound = np.maximum(kp.FACTOR * Y[i], kp.floor(K, NU, kp.magnitudes(tw, keep))) if n != kp.FULL else kp.FACTOR * Y[i]
        per = np.array([kp.distance(dev, ref, np.arange(B) == t) if keep[t] else np.zeros(len(kp.GROUPS)) for t in range(B)])
        rows.append(dict(depth=n, dist=kp.distance(dev, ref, keep), bound=bound, st=st.copy(), its=its.copy(), tst=tw["status"], tits=tw["iters"],
                         keep=keep, per=per))
    b.close(), c.close()
    _RUNS[(case, waves)] = rows
    return rows


def _print(case, waves, r):
    same = r["keep"] & (r["its"] == r["tits"])
    d = r["per"][same].max(axis=0) if (r["depth"] == kp.FULL and same.any()) else r["dist"]
    ratio = float((d / np.maximum(r["bound"], 1e-300)).max())
    print("| %s | %s | %s | %s | %.2f | %s | %s |" % (case, waves, "full" if r["depth"] == kp.FULL else r["depth"], " | ".join("%.1e" % v for v in d), ratio,
                                                  " ".join(str(v) for v in r["its"]), " ".join(str(v) for v in r["tits"])))
    return ratio


@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("case", list(kp.CASES))
def test_device_takes_the_twins_path(case, waves, monkeypatch):
    monkeypatch.setenv("SCVX_K4_WAVES", waves)
    rows = _run(case, waves)
    print("\n| case | wavefronts | depth | dx | du | dsigma | nu | merit | pobj | worst ratio to the bound | device iterations | twin iterations |")
    ratios = [_print(case, waves, r) for r in rows]
    print("%s, %s wavefront(s): worst ratio of a device / twin distance to max(10 Y, floor) %.2f" % (case, waves, max(ratios)))
    for r in rows:
        n, keep = r["depth"], r["keep"]
        assert np.array_equal(r["st"] == 5, r["tst"] == 5), (n, r["st"], r["tst"])
        if n != kp.FULL:
            assert np.array_equal(r["st"], r["tst"]) and np.array_equal(r["its"][keep], r["tits"][keep]), (n, r["st"], r["tst"], r["its"], r["tits"])
            assert np.all(r["dist"] <= r["bound"]), (n, r["dist"], r["bound"])
        else:
            assert np.all(r["st"][keep] == 0) and np.all(r["tst"][keep] == 0), (r["st"], r["tst"])
            diff = np.abs(r["its"] - r["tits"])[keep]
            assert diff.max(initial=0) <= 1, (r["its"], r["tits"])          # how MANY may differ: the cap below
            for t in np.nonzero(keep)[0]:
                if r["its"][t] == r["tits"][t]:
                    assert np.all(r["per"][t] <= r["bound"]), (t, r["per"][t], r["bound"])
                else:
                    assert np.all(r["per"][t][:4] < 1e-6), (t, r["per"][t])


def test_iteration_counts_of_full_solves_equal_the_twins_within_the_cap(monkeypatch):
    """over all (case, executor, trajectory) triples: at most 5 % of the full solves take another iteration count than the twin, and
    none differs by more than 1.  A condition, not a measurement: the twin's two builds differ in 0 of 320."""
    total = differ = worst = 0
    for case in kp.CASES:
        for waves in WAVES:
            monkeypatch.setenv("SCVX_K4_WAVES", waves)
            r = _run(case, waves)[-1]
            assert r["depth"] == kp.FULL
            diff = np.abs(r["its"] - r["tits"])[r["keep"]]
            total, differ, worst = total + diff.size, differ + int((diff != 0).sum()), max(worst, int(diff.max(initial=0)))
    print("full solves with another iteration count than the twin: %d of %d (largest difference %d)" % (differ, total, worst))
    assert worst <= 1 and differ <= 0.05 * total, (differ, total, worst)
