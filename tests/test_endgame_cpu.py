"""What tests/test_gpu_endgame.py stands on, checked without a GPU (tests/endgame_reference.py, tests/k4_path_reference.ENDGAME_CASES):

  * fixture integrity: tests/golden/oracle_endgame_runs.npz has every key, its exo runs end bit for bit on oracle_flight_runs.npz, the
    accept / reject sequences and radii follow from the recorded rho, every rho is at least 0.05 from rh0, rh1 and rh2 (no decision
    is a near-tie; at the one step of endgame_reference.NEAR_TIES the twin's rho is, on the oracle's side of every threshold), sub_tol is 1e-9 except where the oracle's own interior-point method does not end "optimal" there;
  * recomputed distances: TO (parity twin against the oracle) and R (the twin's response to a relative 1e-11 on its tiles) recomputed
    here agree with the fixture within a factor 3 above an absolute 1e-15 (the rule of test_k4_path_cpu.py), for the subproblem and for
    the whole step;
  * cap: TO <= 2e-5 on x, u, dsigma, nu and 1e-8 relative on the objective at every step -- the twin itself meets the widest bound the
    device test can apply.  One step has another objective cap: at the last step of exo3 the oracle's interior-point method stalls at
    a duality gap of 1.1e-7 whatever its tolerance (accepted by its numerical-floor rule from 1.1e-9 up), so its own objective is known
    to 1.2e-7 relative only and that is the cap there (the twin's objective is 5.9e-8 below the oracle's; x 6.6e-8, u 2.4e-8);
  * endgame yardstick: the drift and depth-choice tests of test_k4_path_cpu.py on ENDGAME_CASES;
  * mutation: the twin with its Schur factor forced to float on "nu at the vertex" against the path bound;
  * the straight-line guess of the aero run: two CPU linearisations of it differ, and the twin's solves on them by more than the bound."""
import ctypes as C
import os

import numpy as np
import pytest

import endgame_reference as er
import k4_path_reference as kp
from conftest import GOLDEN

_MEASURED = {}


def _g():
    return er.load()


def _measure(case):
    if case not in _MEASURED:
        _MEASURED[case] = kp.measure(case)
    return _MEASURED[case]


def test_fixture_integrity():
    g = _g()
    flight = np.load(os.path.join(GOLDEN, "oracle_flight_runs.npz"))
    assert list(g["runs"]) == list(er.RUNS) and tuple(g["groups"]) == er.GROUPS and tuple(g["step_groups"]) == er.STEP_GROUPS
    assert tuple(g["sub32_steps"]) == er.SUB32_STEPS and int(g["nsub"]) == er.NSUB and float(g["run_tol"]) == er.RUN_TOL
    assert os.path.getsize(er.FIXTURE) < 1_000_000
    for run, spec in er.RUNS.items():
        po = er.oracle_problem(run)
        n = er.steps_of(g, run)
        for k in er.STEP_KEYS + ("ic", "iterate_x", "iterate_u", "iterate_sigma", "final_x", "final_u", "final_sigma"):
            assert run + "_" + k in g, (run, k)
        for k in er.STEP_KEYS:
            assert g[run + "_" + k].shape[0] == n, (run, k)
        K = po.K
        assert g[run + "_xr"].shape == (n, K + 1, 14) and g[run + "_ur"].shape == (n, K + 1, 3) and g[run + "_nur"].shape == (n, K, 14)
        assert np.array_equal(g[run + "_ic"], er.start(run))
        if spec["flight"] is not None:
            f = spec["flight"]
            assert np.array_equal(g[run + "_final_x"], flight["x"][f]) and np.array_equal(g[run + "_final_u"], flight["u"][f])
            assert g[run + "_final_sigma"] == flight["sigma"][f] and n == flight["steps"][f] and np.array_equal(g[run + "_ic"], flight["ic"][f])
        acc, of, rk, nrk, rho, cost = (g[run + "_" + k] for k in ("accepted", "iterate_of", "rk", "next_rk", "rho", "cost"))
        assert np.array_equal(g[run + "_iter"], np.arange(n)) and rk[0] == 100.0 and np.isinf(cost[0]) and of[0] == 0
        assert np.array_equal(rk[1:], nrk[:-1])
        assert np.array_equal(of[1:], np.cumsum(acc[:-1])) and g[run + "_iterate_x"].shape[0] == of[-1] + 1
        for s in range(n):
            for r in (rho[s], g[run + "_run_rho"][s]):
                want = po.bet * rk[s] if (np.isnan(r) or r >= po.rh2) else rk[s] / po.alph if r < po.rh1 else rk[s]
                assert nrk[s] == want and bool(acc[s]) == (not r < po.rh0), (run, s, r)
                clear = np.isnan(r) or min(abs(r - t) for t in (po.rh0, po.rh1, po.rh2)) >= er.RHO_CLEARANCE
                assert clear != ((run, s + 1) in er.NEAR_TIES), (run, s + 1, r)
                if not clear:    # the twin's rho keeps the clearance, on the oracle's side of every threshold
                    tr = g[run + "_twin_step"][s][2]
                    assert min(abs(tr - t) for t in (po.rh0, po.rh1, po.rh2)) >= er.RHO_CLEARANCE and [tr < t for t in (po.rh0, po.rh1, po.rh2)] == [r < t for t in (po.rh0, po.rh1, po.rh2)]
            assert np.isinf(g[run + "_dJ"][s]) == (not acc[s] or s == 0)
            if acc[s] and s + 1 < n:       # an accepted step's cost is the next step's previous cost, its solution the next iterate (at the run's 1e-8)
                assert abs(cost[s + 1] - g[run + "_jK"][s]) <= 1e-4 * max(1.0, abs(cost[s + 1]))
                assert np.abs(g[run + "_iterate_x"][of[s + 1]] - g[run + "_xr"][s]).max() < 1e-4
        # the run converges at its last step and at no earlier one
        conv = (g[run + "_run_nu_norm"] <= po.nuTol) & (g[run + "_run_dJ"] <= po.delTol)
        assert conv[-1] and not conv[:-1].any()
        tol = g[run + "_sub_tol"]
        assert np.isin(tol, (er.SUB_TOL, er.RUN_TOL)).all() and np.all(g[run + "_twin_status"] == 0)
        print("%s: %d steps %s; sub_tol 1e-8 at steps %s; Tmin nodes %s; rho clearance >= %.3f"
              % (run, n, "".join("ar"[1 - int(a)] for a in acc), list(np.nonzero(tol == er.RUN_TOL)[0] + 1), list(g[run + "_tmin_nodes"]),
                 g[run + "_rho_clearance"].min()))
    assert "".join("ar"[1 - int(a)] for a in g["exo2_accepted"]) == "arrrrrrraaaaa" and np.all(g["exo2_sub_tol"] == er.SUB_TOL)
    assert np.all(g["exo3_sub_tol"][:5] == er.SUB_TOL) and g["exo3_sub_tol"][5] == er.RUN_TOL
    assert er.subproblem_list(g, "exo2") == [0, 1, 5, 7, 8, 9, 10, 11, 12] and [g["exo2_rk"][s] for s in (1, 5, 7)] == [320.0, 20.0, 5.0]
    assert g["exo2_sub32_xr"].shape[0] == len(er.SUB32_STEPS)
    # the regime the fixture is for: the nu-cone on its vertex, a dozen nodes on Tmin, a trust region that binds, a step of 1e-7
    assert g["exo2_nu_norm"][9:].max() < 1e-15 and g["exo2_tmin_nodes"][10] >= 12 and abs(g["exo2_Jtr"][8] - g["exo2_rk"][8]) < 1e-8
    assert np.abs(g["exo2_xr"][12] - g["exo2_iterate_x"][g["exo2_iterate_of"][12]]).max() < 1e-6


@pytest.mark.parametrize("run", list(er.RUNS))
def test_recorded_distances_are_reproduced_and_the_twin_meets_the_cap(run):
    g = _g()
    po, ic = er.oracle_problem(run), g[run + "_ic"]
    worst = 0.0
    for s in range(er.steps_of(g, run)):
        x, u, sigma, rk, cost, itn = er.state(g, run, s)
        it = er.iterate(po, ic, x, u, sigma, rk, cost, itn)
        tol = float(g[run + "_sub_tol"][s])
        sets = [(er.reference(g, run, s), False, "")]
        if run == "exo2" and s + 1 in er.SUB32_STEPS:
            sets.append((er.reference(g, run, er.SUB32_STEPS.index(s + 1), "sub32_"), True, "sub32_"))
        for ref, lin32, pre in sets:
            m = er.measure_step(po, ic, it, ref, tol, lin32)
            names = ("TO", "R") if pre else ("TO", "R", "step_TO", "step_R")
            i = er.SUB32_STEPS.index(s + 1) if pre else s
            for k in names:
                a, f = np.maximum(m[k], 1e-15), np.maximum(g["%s_%s%s" % (run, pre, k)][i], 1e-15)
                ok = np.isfinite(a) & np.isfinite(f)
                assert np.array_equal(np.isfinite(a), np.isfinite(f)), (run, s + 1, k)
                ratio = a[ok] / f[ok]
                worst = max(worst, float(ratio.max()), float(1.0 / ratio.min()))
                assert ratio.max() <= 3.0 and ratio.min() >= 1.0 / 3.0, (run, s + 1, pre + k, m[k], g["%s_%s%s" % (run, pre, k)][i])
            TO = g["%s_%sTO" % (run, pre)][i]
            print("%s step %2d %stol %.0e: TO %s | R %s | bound %s" % (run, s + 1, "float tiles " if pre else "", tol, " ".join("%.1e" % v for v in TO),
                                                                     " ".join("%.1e" % v for v in g["%s_%sR" % (run, pre)][i]),
                                                                     " ".join("%.1e" % v for v in er.sub_bound(g, run, i, pre))))
            # the objective's cap is 1e-8 but where the oracle's own duality gap is larger: at the last step of exo3 alone (1.2e-7 of its
            # objective; the twin is 5.9e-8 BELOW it)
            cap = er.obj_cap(g, run, i, pre)
            assert (cap == er.OBJ_CAP) != ((run, s + 1) == ("exo3", 6)) and cap < 1.3e-7
            assert np.all(TO[:4] <= er.CAP) and TO[4] <= cap, (run, s + 1, TO)
            if not pre:
                assert m["twin_status"] == 0 and m["twin_iters"] == g[run + "_twin_iters"][s]
    print("%s: recomputed / recorded distances within a factor %.2f" % (run, worst))


@pytest.mark.parametrize("case", list(kp.ENDGAME_CASES))
def test_endgame_yardstick_agrees_with_the_fixture_and_the_two_builds_take_the_same_path(case):
    g = np.load(kp.ENDGAME_FIXTURE)
    assert tuple(g["depths"]) == kp.ENDGAME_DEPTHS and tuple(g["groups"]) == kp.GROUPS and list(g["cases"]) == list(kp.ENDGAME_CASES)
    m = _measure(case)
    k = kp.key(case)
    assert np.array_equal(m["iters"], m["native_iters"]) and np.array_equal(m["status"], m["native_status"])
    assert bool(g["counts_identical_" + k])
    assert np.array_equal(m["iters"], g["iters_" + k]) and np.array_equal(m["status"], g["status_" + k])
    assert np.all(m["status"][-1] == 0)
    Y, Yf = np.maximum(m["native"], m["perturb"]), kp.yardstick(case, g)
    rows = lambda a: np.stack([a[:-1].max(axis=0), a[-1]])   # noqa: E731
    ratio = np.maximum(rows(Y), 1e-15) / np.maximum(rows(Yf), 1e-15)
    print("%s: yardstick here / fixture between %.2f and %.2f; largest at a truncated depth %s, full %s; iterations of the full solve %s"
          % (case, ratio.min(), ratio.max(), " ".join("%.1e" % v for v in Y[:-1].max(axis=0)), " ".join("%.1e" % v for v in Y[-1]), m["iters"][-1]))
    assert ratio.max() <= 3.0 and ratio.min() >= 1.0 / 3.0, ratio


@pytest.mark.parametrize("case", list(kp.ENDGAME_CASES))
def test_kept_endgame_depths_have_a_clear_best_iterate(case):
    import oracle
    oracle.use_native(False)
    po, ic, marg, xb, ub, sg, e, d = kp.cpu_inputs(case)
    top = kp.ENDGAME_DEPTHS[-2]
    res = {n: kp.run_twin(case, po, ic, marg, xb, ub, e, d, n) for n in range(1, top + 1)}
    tie = [n for n in range(2, top + 1) if not np.all(res[n]["merit"] < res[n - 1]["merit"] * (1.0 - 1e-6))]
    done = [n for n in range(1, top + 1) if np.any(res[n]["status"] == 0)]
    print("%s: depths without a clear best iterate %s; depths at which a trajectory has finished %s; dropped %s"
          % (case, tie, done, kp.ENDGAME_DROPPED_DEPTHS.get(case, ())))
    assert set(kp.ENDGAME_DROPPED_DEPTHS.get(case, ())) == (set(tie) | set(done)) & set(kp.ENDGAME_DEPTHS)
    assert not set(kp.depths_of(case)) & (set(tie) | set(done))
    for n in kp.depths_of(case)[:-1]:
        assert np.all((res[n]["status"] == 1) & (res[n]["iters"] == n)), (n, res[n]["status"], res[n]["iters"])
    assert len(kp.depths_of(case)) >= 6


def test_aero_straight_line_guess_has_no_linearisation_to_compare_with():
    """Why step 1 of the aero run is compared with the twin on the device's own linearisation and not with the oracle
    (tests/test_gpu_endgame.py): on the straight-line guess the velocity lies along the body axis, the aero model has no derivative
    there, and two CPU linearisations of that state -- the C oracle's variational equations and automatic differentiation of the
    segment map (tests/aero_torque_reference.py) -- differ by 2.5e-6 in the tiles (endpoints 1e-15).  The twin's solves on the two are
    5.3e-5 apart in x, 1.4e-5 in u, 1.8e-6 relative in the objective, 3.6e-3 in the cost: x and the objective beyond the bounds of that
    step (2e-5, 1.8e-9), a factor 20 from tile to solution.  At steps 9 and 13 of the same run the two linearisations agree to 4e-15 and
    the solves to 7e-12 / 4e-15."""
    import aero_torque_reference as ar
    g = _g()
    run = "aero2"
    po, ic = er.oracle_problem(run), g[run + "_ic"]
    for s in (0, 8, 12):
        x, u, sigma, rk, cost, itn = er.state(g, run, s)
        it = er.iterate(po, ic, x, u, sigma, rk, cost, itn)
        e2, d2 = ar.linearize(ar.Params(po), x[None], u[None], np.array([sigma]), 1.0 / (po.K + 1), er.NSUB)
        e2, d2 = np.asarray(e2)[0], np.asarray(d2)[0]
        tol = float(g[run + "_sub_tol"][s])
        a, b = er.twin_point(it, er.twin_sub(po, ic, it, tol)), er.twin_point(it, er.twin_sub(po, ic, it, tol, e=e2, d=d2))
        dist, bound = er.distance(po, x, u, a, b), er.sub_bound(g, run, s)
        sd = er.step_distance(er.step_figures(po, it, a), er.step_figures(po, it, b))
        gap_e, gap_d = float(np.abs(e2 - it.endpoint).max()), float(np.abs(d2 - it.deriv).max())
        print("aero2 step %2d: the two linearisations differ by %.1e (endpoint) %.1e (tiles); the twin on the two: %s (bound %s); cost %.1e"
              % (s + 1, gap_e, gap_d, " ".join("%.1e" % v for v in dist), " ".join("%.1e" % v for v in bound), sd[0]))
        if s == 0:
            assert gap_e < 1e-12 and gap_d > 1e-7 and dist[0] > bound[0] and dist[4] > bound[4]
        else:
            assert gap_d < 1e-12 and np.all(dist[[0, 1, 2, 4]] <= 0.1 * bound[[0, 1, 2, 4]])


def test_float_factor_mutation_on_nu_at_the_vertex(monkeypatch):
    """The twin with its Schur factor forced to float (SCVX_PORT_FAC32=1 against =0) on "nu at the vertex", against the path bound
    max(10 Y, floor) at every kept depth.  Measured: 2.4e6 x the bound at depth 2, 6e5 to 1.3e6 at depths 3 to 8 (dx 2e-4), 3.5e5 at
    depth 10, 6.6e4 at depth 12, 1.1e3 at depth 16 and 56 x at full depth (dx 2.3e-10, du 2.9e-10: five orders below the 2e-5 of an
    end-of-solve comparison), with equal iteration counts throughout.  Asserted: more than 1000 x at some truncated depth, as
    test_k4_path_cpu.py asserts of the first subproblem, and less than 1e-5 apart at full depth."""
    import oracle
    from oracle import port, port_lib
    oracle.use_native(False)
    case = "nu at the vertex"
    po, ic, marg, xb, ub, sg, e, d = kp.cpu_inputs(case)
    B, K = ic.shape[0], po.K
    port_lib().scvx_port_work_doubles_nu.restype = C.c_size_t
    nw = port_lib().scvx_port_work_doubles_nu(C.c_int(K), C.c_int(0), C.c_int(3))
    Y = kp.yardstick(case)
    worst, res = 0.0, {}
    for n in kp.depths_of(case):
        i = kp.ENDGAME_DEPTHS.index(n)
        for fac in ("0", "1"):
            monkeypatch.setenv("SCVX_PORT_FAC32", fac)
            res[fac] = port.socp(po, xb, ub, e, d, kp.rk_of(case), ic, tol=kp.ENDGAME_TOL, max_iter=n, retries=0, work=np.zeros((B, nw)), warm=np.zeros(B, np.int32))
        dist = kp.distance(res["0"], res["1"])[:4]
        bound = np.maximum(kp.FACTOR * Y[i], kp.floor(K, 3, kp.magnitudes(res["0"])))[:4] if n != kp.FULL else kp.FACTOR * Y[i][:4]
        ratio = float((dist / bound).max())
        print("depth %2d: float factor against double factor dx %.1e du %.1e dsigma %.1e nu %.1e = %.1e x the path bound; iterations %s / %s, status %s / %s"
              % (n, dist[0], dist[1], dist[2], dist[3], ratio, res["0"]["iters"], res["1"]["iters"], res["0"]["status"], res["1"]["status"]))
        if n != kp.FULL:
            worst = max(worst, ratio)
    assert worst > 1000.0, worst
    assert dist.max() < 1e-5 and np.all(res["0"]["status"] == 0) and np.all(res["1"]["status"] == 0)
