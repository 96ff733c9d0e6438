"""The conic solve (K4) and the SCvx step (K1, K2, K3, K5) in the CONVERGING regime on the MI355X, against the independent CPU oracle
re-run step by step on runs that converge (tests/endgame_reference.py; fixture tests/golden/oracle_endgame_runs.npz): the nu-cone
collapsed onto its vertex, a dozen or more nodes riding Tmin, a trust region that binds, steps of 1e-7, rho as a ratio of small
differences.  Everywhere else in the suite the subproblem compared with something outside the device is the first one (straight-line
guess, rk = 100, cost = Inf).  All tests are B <= 2, K = 50.

Bounds, none of them taken from the device (tests/test_endgame_cpu.py keeps the fixtures honest):
  * one subproblem at a recorded step against the oracle, both sides at the step's sub_tol: status 0, merit < sub_tol, and per group
    (x, u, dsigma, nu absolute; objective relative) min(10 max(TO, R), cap) with TO = the parity twin against the oracle and R = the
    twin's response to a relative 1e-11 on its tiles (the K1 parity bound), both from the fixture; cap = 2e-5 on the minimiser and
    1e-8 on the objective, the bounds the suite uses on the first subproblem.  At the last steps that is about 2e-7 on x where 2e-5
    would be blind.  Where the oracle's |nu| is below 1e-15 (the vertex of the nu-cone) the entries of nu are noise on every side: there
    the nu group is held by its norm instead, |nu|_device <= max(10 |nu|_twin, 1e-12);
  * the path: test_gpu_k4_path.py's comparison with the twin on the device's own linearisation, depth by depth, over
    k4_path_reference.ENDGAME_CASES at the recorded trust radii (yardstick tests/golden/k4_endgame_yardstick.npz), same factor, floor
    and iteration-count cap, both sides at 1e-9.  A FINISHED solve has two rules of its own (_finished below, derived there): on the
    vertex the nu group is held by the norm rule above (the entries are 1e-19 .. 1e-25 on every side), and the merit has the floor
    of one rounding of an O(1) residual term, 2^-52 / merit.  Every truncated depth, and every other group, keeps max(10 Y, floor);
  * one solve_step from a recorded state (rk, cost, iter set): the oracle's accept / reject decision, its next rk EXACTLY (products
    of alph and bet), its (|nu| <= nuTol) and (dJ <= delTol); cost, dJ, rho and |nu| within 10 max(step_TO, step_R) of the oracle's, the
    whole-step counterparts of TO and R (rho at the last step is a ratio of two differences of 6e-4: R, not TO, is what bounds it
    there); the new iterate within the subproblem bound after an accepted step, and bit for bit the state that was set after a
    rejected one.  rho is not part of the ABI: it is recomputed from cost, the new cost, the new final mass and |nu| after an accepted
    step; after a rejected one the status and the halved radius are all there is to see.  At step 1 of the aero run the reference of the
    figures is the parity twin on the DEVICE's linearisation instead of the oracle (same bounds; decision, radius and counters stay the
    oracle's): on the straight-line guess the velocity lies along the body axis, where the aero model has no derivative, two CPU
    linearisations differ by 2.5e-6 there and the twin's solves on them by 5.3e-5 in x (tests/test_endgame_cpu.py), and the device
    is 1.7e-4 in x from the oracle's solve of ITS tiles.  The complete aero run below starts from that very guess and meets the
    oracle's plan;
  * a complete run from the straight-line guess at the default tolerance: CONVERGED, the oracle's accept / reject sequence and step
    count, re-propagation defect < 1e-5, final mass, r and v within 1e-4 (the project's contract for a run at 1e-8).
On one MI355X (profiles/endgame_parity.md): every decision, radius and iteration count equal; worst
device-vs-oracle distance / bound 0.96 (step 1 of exo2: x 1.9e-5 of 2e-5, the twin's own distance), 0.48 at the last step of exo3, 0.10
everywhere else -- the device sits on the twin; the path within 0.26 / 0.42 / 0.47 of its bound for 1 / 2 / 4 wavefronts, 0 of 27
full solves with another iteration count; step 1 of the aero run x 5e-11, cost 1e-8 from the twin on the device's tiles; device |nu| on the vertex 4e-19 .. 7e-16 (the twin's: 4e-19 .. 7e-16).
Every comparison prints its figures before it asserts."""
import ctypes as C

import numpy as np
import pytest

import endgame_reference as er
import k4_path_reference as kp
import k4_path_device as kd
from k4_path_device import WAVES

pytestmark = pytest.mark.gpu

VERTEX = 1e-15          # the oracle's |nu| below this: the nu-cone sits on its vertex
NU_FLOOR = 1e-12
_G = {}


def _fixture():
    if not _G:
        _G["g"] = er.load()
    return _G["g"]


def _solver(b, tol):
    from successiveconvexification_amd import _lib
    o = _lib.ScvxSolverOpts()
    b._L.scvx_solver_default_opts(C.byref(o))
    o.tol = o.accept_tol = float(tol)
    _lib.check(b.cache.handle, b._L.scvx_batch_set_solver(b.handle, C.byref(o)), "scvx_batch_set_solver")


def _batch(run, lin32=False):
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache
    c = IntegratorCache(er.device_problem(run), npts=er.NSUB)
    b = ScvxBatch(c, 1)
    if lin32:
        b.set_linearization_f32(True)
    b.init(_fixture()[run + "_ic"][None])
    return c, b


def _fmt(v):
    return " ".join("%.1e" % a for a in v)


SUBPROBLEMS = {"exo2": ("exo2", None, ""), "exo3": ("exo3", None, ""), "exo2 float tiles": ("exo2", "sub32", "sub32_"),
               "aero2 last three steps": ("aero2", "last3", "")}


@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("variant", list(SUBPROBLEMS))
def test_one_subproblem_at_every_recorded_step_against_the_independent_oracle(variant, waves, monkeypatch):
    monkeypatch.setenv("SCVX_K4_WAVES", waves)
    g = _fixture()
    run, pick, pre = SUBPROBLEMS[variant]
    po = er.oracle_problem(run)
    n = er.steps_of(g, run)
    steps = [s - 1 for s in er.SUB32_STEPS] if pick == "sub32" else list(range(n - 3, n)) if pick == "last3" else er.subproblem_list(g, run)
    c, b = _batch(run, lin32=pick == "sub32")
    print("\n| run | wavefronts | step | rk | sub_tol | status | iterations | merit | x | u | dsigma | nu | objective | bound | worst ratio | device nu norm "
          "(oracle, twin) |")
    bad, worst = [], 0.0
    for j, s in enumerate(steps):
        x, u, sigma, rk, cost, it = er.state(g, run, s)
        tol = float(g[run + "_sub_tol"][s])
        ref = er.reference(g, run, j if pick == "sub32" else s, pre)
        bound = er.sub_bound(g, run, j if pick == "sub32" else s, pre)
        b.set_trajectory(x[None], u[None], np.array([sigma]))
        b.set_scalars(rk=rk)
        _solver(b, tol)
        xs, us, ss, nu = b.socp_solve()
        st, its, merit, _ = b.solver_stats()
        dev = dict(xr=xs[0], ur=us[0], dsr=float(ss[0] - sigma), nur=nu[0])
        dist = er.distance(po, x, u, dev, ref)
        nun, onun, tnun = float(np.linalg.norm(nu[0])), float(g[run + "_nu_norm"][s]), float(g[run + "_twin_step"][s][3])
        vertex = onun < VERTEX
        ok = dist <= bound
        if vertex:
            ok[3] = nun <= max(er.FACTOR * tnun, NU_FLOOR)
        ratio = float(np.delete(dist / bound, 3).max()) if vertex else float((dist / bound).max())
        worst = max(worst, ratio)
        print("| %s | %s | %d | %g | %.0e | %d | %d | %.1e | %s | %s | %.2f | %.1e (%.1e, %.1e)%s |"
              % (variant, waves, s + 1, rk, tol, st[0], its[0], merit[0], " | ".join("%.1e" % v for v in dist), _fmt(bound), ratio, nun, onun, tnun,
                 " vertex" if vertex else ""))
        if not (st[0] == 0 and merit[0] < tol and ok.all()):
            bad.append((s + 1, int(st[0]), float(merit[0]), dist, bound))
    print("%s, %s wavefront(s): worst device-vs-oracle distance / bound %.2f" % (variant, waves, worst))
    b.close(), c.close()
    assert not bad, bad


def _finished(r, t):
    """the bound of a finished solve of trajectory t with the twin's iteration count (the hook of k4_path_device.check_path): 10 Y, and
      * the merit is a norm of residuals whose terms are O(1): no two evaluation orders reproduce it to better than one rounding of
        such a term, 2^-52 absolute, 2^-52 / merit relative.  (One trajectory's Y(merit) on the B = 1 aero case is 7.9e-9 of a merit
        of 5e-10: 4e-18 absolute.  On kp.CASES the floor would be below 2.2e-7 against 10 Y(merit) >= 1e-4.);
      * with the nu-cone on its vertex (the twin's |nu| below 1e-15) the entries of nu are what the last Newton step's rounding left
        of a variable that is zero -- 1e-19 .. 1e-25, another residue in every build and executor, 10 Y(nu) = 6e-21 / 6e-23 on the two
        last-step cases -- so the nu group is held by its norm, the rule of the subproblem test: |nu|_device <= max(10 |nu|_twin, 1e-12)."""
    b = r["bound"].copy()
    b[4] = max(b[4], kp.EPS / max(float(r["tmerit"][t]), 1e-300))
    return b, bool(r["tnun"][t] < VERTEX)


@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("case", list(kp.ENDGAME_CASES))
def test_device_takes_the_twins_path_in_the_endgame(case, waves, monkeypatch):
    monkeypatch.setenv("SCVX_K4_WAVES", waves)
    kd.check_path(case, waves, finished=_finished, nu_floor=NU_FLOOR)


def test_iteration_counts_of_full_endgame_solves_equal_the_twins_within_the_cap(monkeypatch):
    """at most 5 % of the full solves take another iteration count than the twin, none differs by more than 1 (the twin's two builds
    differ in none: tests/test_endgame_cpu.py)"""
    kd.check_counts(kp.ENDGAME_CASES, monkeypatch)


@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("run", list(er.RUNS))
def test_one_solve_step_from_every_recorded_state(run, waves, monkeypatch):
    monkeypatch.setenv("SCVX_K4_WAVES", waves)
    g = _fixture()
    po = er.oracle_problem(run)
    K = po.K
    c, b = _batch(run)
    bad, worst = [], 0.0
    print("\n| run | wavefronts | step | rk -> next | status (oracle accepted) | cost | dJ | rho | nu norm | bound | device cost dJ rho nu norm | iterate x u dsigma |")
    for s in range(er.steps_of(g, run)):
        x, u, sigma, rk, cost, it = er.state(g, run, s)
        tol = float(g[run + "_sub_tol"][s])
        ref, sb, tb = er.reference(g, run, s), er.sub_bound(g, run, s), er.step_bound(g, run, s)
        acc, next_rk = bool(g[run + "_accepted"][s]), float(g[run + "_next_rk"][s])
        # the aero model has no derivative on the straight-line guess (velocity along the body axis: angle of attack on the edge of its
        # clamp, lift direction 0 / 0).  Two CPU linearisations of that state, the C oracle's and automatic differentiation, are 2.5e-6
        # apart in the tiles and the twin's solves on them 5.3e-5 in x, 1.8e-6 in the objective (tests/test_endgame_cpu.py asserts
        # it): the oracle's solve of ITS tiles is no reference for the device's solve of K1's.  So at step 1 of the aero run the
        # decision, radius and counters are the oracle's, and cost, dJ, rho, |nu| and the new iterate are held, under the same bounds, to
        # the parity twin on the DEVICE's linearisation pushed through the oracle's propagation (K2, K3, K4, K5; not K1)
        no_derivative = er.RUNS[run]["model"] == "aero" and s == 0
        want = dict(jK=float(g[run + "_jK"][s]), dJ=float(g[run + "_dJ"][s]), rho=float(g[run + "_rho"][s]), nu_norm=float(g[run + "_nu_norm"][s]))
        b.set_trajectory(x[None], u[None], np.array([sigma]))
        if no_derivative:
            from oracle import port
            ic = g[run + "_ic"]
            e, d = b.linearization()
            it0 = er.iterate(po, ic, x, u, sigma, rk, cost, it)
            tw = port.socp(po, x[None], u[None], e, d, np.array([rk]), ic[None], tol=tol)
            assert tw["status"][0] == 0
            ref = er.twin_point(it0, tw)
            want = er.step_figures(po, it0, ref)
        b.set_scalars(rk=rk, cost=cost, it=it)
        b.set_flags(status=1, active=1, live=1)
        _solver(b, tol)
        rec0 = b.trajectory_record()
        st, nun, dj = b.solve_step()
        rk1, cost1, it1 = b.scalars()
        x1, u1, s1 = b.trajectory()
        fails = []
        if st[0] not in (0, 1, 2) or (st[0] != 2) != acc:
            fails.append("decision")
        if rk1[0] != next_rk or it1[0] != it + 1:
            fails.append("rk / iter")
        if (nun[0] <= po.nuTol) != (g[run + "_run_nu_norm"][s] <= po.nuTol) or (dj[0] <= po.delTol) != (g[run + "_run_dJ"][s] <= po.delTol):
            fails.append("convergence test")
        if (st[0] == 0) != (nun[0] <= po.nuTol and dj[0] <= po.delTol):
            fails.append("CONVERGED")
        got = dict(jK=float(cost1[0]) if acc else np.nan, dJ=float(dj[0]), rho=np.nan, nu_norm=float(nun[0]))
        dist_it = np.zeros(3)
        if acc and st[0] != 2:
            with np.errstate(invalid="ignore"):
                got["rho"] = float((cost - cost1[0]) / (cost - (-x1[0, K, 0] + po.wNu * nun[0]))) if np.isfinite(cost) else np.nan
            d = er.step_distance(got, want)
            if want["nu_norm"] < VERTEX:
                d[3] = 0.0 if nun[0] <= max(er.FACTOR * float(g[run + "_twin_step"][s][3]), NU_FLOOR) else np.inf
            dist_it = np.array([np.abs(x1[0] - ref["xr"]).max(), np.abs(u1[0] - ref["ur"]).max(), abs(s1[0] - sigma - ref["dsr"])])
            if not (d <= tb).all():
                fails.append("step figures")
            if not (dist_it <= sb[:3]).all():
                fails.append("iterate")
            worst = max(worst, float((d[:3] / np.maximum(tb[:3], 1e-300)).max()), float((dist_it / sb[:3]).max()))
        else:
            d = np.array([0.0, 0.0 if np.isinf(dj[0]) else np.inf, 0.0, abs(nun[0] - want["nu_norm"])])
            if not (np.array_equal(b.trajectory_record(), rec0) and cost1[0] == cost and np.isinf(dj[0]) and d[3] <= tb[3]):
                fails.append("rejected step")
        print("| %s | %s | %d | %g -> %g (%g) | %d (%d) | %s | %s | %.10g %.4e %.6f %.2e | %s |%s"
              % (run, waves, s + 1, rk, rk1[0], next_rk, st[0], acc, " | ".join("%.1e" % v for v in d), _fmt(tb), cost1[0], dj[0], got["rho"], nun[0],
                 _fmt(dist_it), (" FAILS: " + ", ".join(fails)) if fails else ""))
        if fails:
            bad.append((s + 1, fails))
    print("%s, %s wavefront(s): worst distance / bound over the accepted steps %.2f" % (run, waves, worst))
    b.close(), c.close()
    assert not bad, bad


FULL_RUNS = [("exo", w) for w in WAVES] + [("aero", None)]


@pytest.mark.parametrize("model,waves", FULL_RUNS)
def test_complete_run_from_the_guess_converges_on_the_oracles_plan(model, waves, monkeypatch):
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache, propagate_batch
    if waves is not None:
        monkeypatch.setenv("SCVX_K4_WAVES", waves)
    g = _fixture()
    runs = ("exo2", "exo3") if model == "exo" else ("aero2",)
    pp = er.device_problem(runs[0])
    B, K = len(runs), pp.K
    ic = np.stack([g[r + "_ic"] for r in runs])
    c = IntegratorCache(pp, npts=er.NSUB)
    b = ScvxBatch(c, B).init(ic)
    st, it, nu, dj = b.solve()
    x, u, s = b.trajectory()
    # the accept / reject sequence, from a second batch stepped one solve_step at a time
    twin = ScvxBatch(c, B).init(ic)
    seq, done = [[] for _ in range(B)], np.zeros(B, bool)
    for _ in range(pp.imax - 1):
        s1 = twin.solve_step()[0]
        for t in range(B):
            if not done[t]:
                seq[t].append(0 if s1[t] == 2 else 1)
                done[t] = s1[t] not in (1, 2)
        if done.all():
            break
    want = [[int(v) for v in g[r + "_accepted"]] for r in runs]
    gx, gu, gs = (np.stack([g[r + k] for r in runs]) for k in ("_final_x", "_final_u", "_final_sigma"))
    defect = float(np.abs(propagate_batch(c, x, u, s, 1.0 / (K + 1)) - x[:, 1:]).max())
    em, er_, ev = np.abs(x[:, -1, 0] - gx[:, -1, 0]).max(), np.abs(x[:, :, 1:4] - gx[:, :, 1:4]).max(), np.abs(x[:, :, 4:7] - gx[:, :, 4:7]).max()
    print("%s, %s wavefront(s): status %s steps %s (oracle %s); sequences %s (oracle %s); |nu| %s dJ %s; defect %.3e"
          % (model, waves or "default", st, it, [len(w) for w in want], ["".join("ar"[1 - v] for v in q) for q in seq],
             ["".join("ar"[1 - v] for v in q) for q in want], nu, dj, defect))
    print("final mass %s (oracle %s); device-vs-oracle: mass %.2e r %.2e v %.2e | q %.2e w %.2e u %.2e sigma %.2e (the last four: printed only)"
          % (x[:, -1, 0], gx[:, -1, 0], em, er_, ev, np.abs(x[:, :, 7:11] - gx[:, :, 7:11]).max(), np.abs(x[:, :, 11:] - gx[:, :, 11:]).max(),
             np.abs(u - gu).max(), np.abs(s - gs).max()))
    b.close(), twin.close(), c.close()
    assert np.all(st == 0), (st, it)
    assert seq == want
    assert [int(v) for v in it] == [len(w) for w in want]
    assert defect < 1e-5
    assert em < 1e-4 and er_ < 1e-4 and ev < 1e-4
