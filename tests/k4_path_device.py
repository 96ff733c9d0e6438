"""Device side of the interior-point path comparison (tests/k4_path_reference.py holds the case tables and the CPU side) -- a helper
module, not a test file.  Used by tests/test_gpu_k4_path.py (kp.CASES) and tests/test_gpu_endgame.py (kp.ENDGAME_CASES).

run(case, waves) solves every kept depth of a case on the device and on the parity twin, both on the device's linearisation;
check_path asserts the comparison, check_counts the iteration-count cap.  `finished` is a hook for a FINISHED solve (full depth, the
twin's iteration count): finished(row, t) returns (bound [group], nu_by_norm) for trajectory t, or None for the rule of kp.CASES,
10 Y on every group.  tests/test_gpu_k4_path.py passes none."""
import ctypes as C

import numpy as np

import k4_path_reference as kp

WAVES = ("1", "2", "4")
_RUNS = {}          # (case, waves) -> list of rows; filled once per pair


def set_depth(b, n, tol=None):
    from successiveconvexification_amd import _lib
    o = _lib.ScvxSolverOpts()
    b._L.scvx_solver_default_opts(C.byref(o))
    o.max_iter, o.retries = int(n), 0
    if tol is not None:
        o.tol = o.accept_tol = float(tol)
    _lib.check(b.cache.handle, b._L.scvx_batch_set_solver(b.handle, C.byref(o)), "scvx_batch_set_solver")


def run(case, waves):
    """every depth of one case on one executor: the device and the parity twin on the device's linearisation.  Returns rows of
    dict(depth, dist, bound, status / iters of both sides, keep, per-trajectory distance at full depth, |nu| and the twin's merit per
    trajectory); nothing is asserted here.  A case of kp.ENDGAME_CASES starts from its recorded iterates, trust radii and tolerance."""
    if (case, waves) in _RUNS:
        return _RUNS[(case, waves)]
    import oracle
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache
    oracle.use_native(False)
    spec = kp.spec_of(case)
    endgame = case in kp.ENDGAME_CASES
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
    if endgame:
        _, x0, u0, s0, rk0 = kp.endgame_states(case)
        b.set_trajectory(x0, u0, s0)
        b.set_scalars(rk=rk0)
    xb, ub, sg = b.trajectory()
    e, d = b.linearization()
    rows = []
    for n in kp.depths_of(case):
        set_depth(b, n, kp.tol_of(case) if endgame else None)
        x, u, snew, nu = b.socp_solve()
        st, its, merit, pobj = b.solver_stats()
        tw = kp.run_twin(case, po, ic, marg, xb, ub, e, d, n)
        keep = tw["status"] != 5
        dev = dict(dx=x, du=u, ds=snew, nu=nu, merit=merit, pobj=pobj)
        ref = dict(dx=xb + tw["dx"], du=ub + tw["du"], ds=sg + tw["ds"], nu=tw["nu"], merit=tw["merit"], pobj=tw["pobj"])
        i = kp.all_depths(case).index(n)
        bound = np.maximum(kp.FACTOR * Y[i], kp.floor(K, NU, kp.magnitudes(tw, keep))) if n != kp.FULL else kp.FACTOR * Y[i]
        per = np.array([kp.distance(dev, ref, np.arange(B) == t) if keep[t] else np.zeros(len(kp.GROUPS)) for t in range(B)])
        rows.append(dict(depth=n, dist=kp.distance(dev, ref, keep), bound=bound, st=st.copy(), its=its.copy(), tst=tw["status"], tits=tw["iters"],
                         keep=keep, per=per, nun=np.sqrt((nu ** 2).sum((1, 2))), tnun=np.sqrt((tw["nu"] ** 2).sum((1, 2))), tmerit=tw["merit"].copy()))
    b.close(), c.close()
    _RUNS[(case, waves)] = rows
    return rows


def _rule(r, t, finished):
    got = finished(r, t) if finished is not None else None
    return (r["bound"], False) if got is None else got


def print_row(case, waves, r, finished=None):
    same = r["keep"] & (r["its"] == r["tits"])
    full = r["depth"] == kp.FULL and same.any()
    if full:      # per trajectory with the twin's count, each against its own bound
        q = []
        for t in np.nonzero(same)[0]:
            bound, by_norm = _rule(r, t, finished)
            v = r["per"][t] / np.maximum(bound, 1e-300)
            q.append(np.delete(v, 3) if by_norm else v)
        d, ratio = r["per"][same].max(axis=0), float(max(v.max() for v in q))
    else:
        d = r["dist"]
        ratio = float((d / np.maximum(r["bound"], 1e-300)).max())
    print("| %s | %s | %s | %s | %.2f | %s | %s |" % (case, waves, "full" if r["depth"] == kp.FULL else r["depth"], " | ".join("%.1e" % v for v in d), ratio,
                                                  " ".join(str(v) for v in r["its"]), " ".join(str(v) for v in r["tits"])))
    return ratio


def check_path(case, waves, finished=None, nu_floor=None):
    """the assertions of the path comparison on one case and executor (SCVX_K4_WAVES already set); returns the worst ratio"""
    rows = run(case, waves)
    print("\n| case | wavefronts | depth | dx | du | dsigma | nu | merit | pobj | worst ratio to the bound | device iterations | twin iterations |")
    ratios = [print_row(case, waves, r, finished) for r in rows]
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
            assert diff.max(initial=0) <= 1, (r["its"], r["tits"])          # how MANY may differ: check_counts
            for t in np.nonzero(keep)[0]:
                if r["its"][t] == r["tits"][t]:
                    bound, by_norm = _rule(r, t, finished)
                    if by_norm:
                        print("trajectory %d, nu-cone on its vertex: |nu| device %.1e, twin %.1e" % (t, r["nun"][t], r["tnun"][t]))
                        assert r["nun"][t] <= max(kp.FACTOR * r["tnun"][t], nu_floor), (t, r["nun"][t], r["tnun"][t])
                        assert np.all(np.delete(r["per"][t], 3) <= np.delete(bound, 3)), (t, r["per"][t], bound)
                    else:
                        assert np.all(r["per"][t] <= bound), (t, r["per"][t], bound)
                else:
                    assert np.all(r["per"][t][:4] < 1e-6), (t, r["per"][t])
    return max(ratios)


def check_counts(cases, monkeypatch):
    """over all (case, executor, trajectory) triples: at most 5 % of the full solves take another iteration count than the twin, and
    none differs by more than 1"""
    total = differ = worst = 0
    for case in cases:
        for waves in WAVES:
            monkeypatch.setenv("SCVX_K4_WAVES", waves)
            r = run(case, waves)[-1]
            assert r["depth"] == kp.FULL
            diff = np.abs(r["its"] - r["tits"])[r["keep"]]
            total, differ, worst = total + diff.size, differ + int((diff != 0).sum()), max(worst, int(diff.max(initial=0)))
    print("full solves with another iteration count than the twin: %d of %d (largest difference %d)" % (differ, total, worst))
    assert worst <= 1 and differ <= 0.05 * total, (differ, total, worst)
