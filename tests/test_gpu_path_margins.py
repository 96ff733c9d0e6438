"""Path-constraint back-offs (mass, glide slope, tilt, rate) in the conic solve on the MI355X (scvx_batch_set_path_margins,
scvx_batch_get_path_margins, scvx_batch_margins_from_cov; include/scvx.h) against the independent CPU oracle under the same back-offs
(tests/path_margin_reference.py; fixture tests/golden/oracle_path_margin_runs.npz) and against the properties that define the feature.

Bounds, none of them taken from the device:
  * one subproblem against the independent oracle: those of test_gpu_margins.test_one_subproblem_with_backoffs_against_the_
    independent_oracle (both sides at 1e-9: 2e-5 on the minimiser, 1e-8 relative on the objective); in the oracle's solution each of
    the four kinds is active at one node or more (asserted by the generator and by test_path_margins_cpu.py); group "k100" (K = 100,
    tests/golden/oracle_path_margin_k100.npz): 4 x the CPU twin's distance from the oracle there, 4.17e-5, see the test;
  * a complete run from the straight-line guess under tilt back-offs: CONVERGED, the oracle's accept / reject sequence (13 steps,
    arrrrrrraaaaa), final mass, r and v within 1e-4 of the oracle's (test_gpu_margins.test_full_run_from_the_straight_line_guess_under_
    backoffs), the tightened tilt cone at every node within ten times the figure to which the oracle's own run resolves it (|smallest
    slack| of that run, 6e-8, stored in the fixture as run0_viol);
  * robustify(constraints=("thrust", "tilt")): N_TILT <= 1e-4 before and >= 2.0 after, N_TMIN and N_TMAX >= 2.0 after (README's
    "about 2.5 - 3 sigma per round" less a margin);
  * scvx_batch_margins_from_cov: exactly the numpy formula on the returned psig (one multiply and one min per entry).
Every comparison prints its figures before it asserts.
"""
import math
import os
from dataclasses import replace

import numpy as np
import pytest

import cov_reference as cr
import path_margin_reference as pr
from conftest import GOLDEN
from test_gpu_flight import _flyable

pytestmark = pytest.mark.gpu

KW = dict(mdry=0.55, nuTol=1e-6, delTol=1e-3, imax=40, tf_guess=8.0)


def _fixture(name=None):
    """the fixture that holds group `name`: "k100" has a file of its own"""
    return np.load(os.path.join(GOLDEN, "oracle_path_margin_k100.npz" if name == "k100" else "oracle_path_margin_runs.npz"))


def _s0(x):
    return np.stack([cr.handover_s0(x[b, 0], 0, 1e-3)[0] for b in range(x.shape[0])])


def _set(b, pm):
    return b.set_path_margins(mass=pm[..., pr.MASS], glide=pm[..., pr.GLIDE], tilt=pm[..., pr.TILT], rate=pm[..., pr.RATE])


def _problems(name):
    """(device problem, oracle problem) of a fixture group"""
    from oracle import model as om
    from successiveconvexification_amd import sample_problems as sp
    if name == "fin":
        return replace(sp.base_prob_fin_scaled(), mdry=0.55, tf_guess=8.0), replace(om.base_prob_fin_scaled(), mdry=0.55, tf_guess=8.0)
    K = {"k9": 9, "k100": 100}.get(name, 50)
    return replace(sp.base_prob_scaled, K=K, **KW), replace(om.base_prob_scaled(), K=K, **KW)


@pytest.mark.parametrize("name,waves", [(n, w) for n in ("k50", "k50f", "fin", "k9", "k100") for w in ("1", "2", "4")],
                         ids=["%s waves%s" % (n, w) for n in ("K50", "K50 float tiles", "K50 fins", "K9", "K100") for w in "124"])
def test_one_subproblem_with_path_backoffs_against_the_independent_oracle(name, waves, monkeypatch):
    """scvx_socp_solve at the straight-line guess, B = 3 with different back-offs of all four kinds per trajectory, against the oracle's
    solves of the edited SOCPs.

    The bound on the minimiser is 2e-5 where the CPU twin of the conic solve (the same algorithm, tests/path_margin_port.cpp) is within
    5e-6 of the oracle -- it is at 4e-6 on the K = 50 groups.  On group "k100" the twin is at d100 = 1.0434e-5 (start 0, in x; 1.2e-6
    and 3.0e-6 on the other two; test_path_margins_cpu.D100, asserted there), so the device's bound at K = 100 is 4 d100 = 4.17e-5:
    taken from the twin against the oracle on the CPU, not from a device run.  The objective keeps 1e-8 relative (the twin: 1.9e-10)."""
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache
    from test_path_margins_cpu import D100
    g = _fixture(name)
    tol = 4.0 * D100 if name == "k100" else 2e-5
    pp, po = _problems(name)
    K = pp.K
    ic, pm = g[name + "_ic"], g[name + "_pm"]
    ref = {k: g["%s_%s" % (name, k)] for k in ("x", "u", "dsig", "nu", "pobj")}
    monkeypatch.setenv("SCVX_K4_WAVES", waves)
    c = IntegratorCache(pp, npts=10)
    b = ScvxBatch(c, 3, tol=1e-9)
    if name == "k50f":
        b.set_linearization_f32(True)
    b.init(ic)
    xb, ub, sg = b.trajectory()
    free = b.socp_solve()
    _set(b, pm)
    assert np.array_equal(b.path_margins(), pm)
    x, u, snew, nu = b.socp_solve()
    st, its, merit, pobj = b.solver_stats()
    for t in range(3):
        ex, eu, es, en = (float(np.abs(x[t] - ref["x"][t]).max()), float(np.abs(u[t] - ref["u"][t]).max()),
                          float(abs(snew[t] - sg[t] - ref["dsig"][t])), float(np.abs(nu[t] - ref["nu"][t]).max()))
        obj = (-x[t, K, 0] + pp.wNu * np.linalg.norm(nu[t]) + 0.5 * np.linalg.norm(np.concatenate([(x - xb)[t].ravel(), (u - ub)[t].ravel()]))
               + abs(snew[t] - sg[t]))
        s = pr.slacks(po, x[t], pm[t])
        print("%s waves %s trajectory %d: status %d merit %.2e its %d; device-vs-oracle x %.2e u %.2e dsigma %.2e nu %.2e (bound %.2e); objective "
              "%.10f vs %.10f; smallest tightened slack per kind %s; moved by the back-offs: %.2e"
              % (name, waves, t, st[t], merit[t], its[t], ex, eu, es, en, tol, obj, ref["pobj"][t], s.min(axis=0), np.abs(x[t] - free[0][t]).max()))
        assert st[t] == 0 and merit[t] < 1e-9
        assert ex < tol and eu < tol and es < tol and en < tol, (tol, ex, eu, es, en)
        assert abs(obj - ref["pobj"][t]) < 1e-8 * abs(ref["pobj"][t])
        assert s.min() > -1e-8                                   # the tightened rows hold
        assert (s.min(axis=0) < tol).all()                       # ... and each kind binds (the oracle: < 1e-7, the minimisers agree to tol)
        assert np.abs(x[t] - free[0][t]).max() > 1e-4            # the unmargined solve of the same subproblem is elsewhere
    b.close(), c.close()


def _state(b, r):
    return tuple(r) + (b.trajectory_record(),) + b.scalars() + b.flags() + b.solver_stats()


@pytest.mark.parametrize("waves", ["1", "2", "4"])
def test_null_zero_and_cleared_backoffs_change_nothing(waves, monkeypatch):
    import bench
    from successiveconvexification_amd import sample_problems as sp
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache
    monkeypatch.setenv("SCVX_K4_WAVES", waves)
    p = sp.base_prob_scaled
    B = 4
    ic = bench.disperse_ics(p, 0, B, 20261018)
    c = IntegratorCache(p, npts=10)
    plain, zero, cleared = (ScvxBatch(c, B).init(ic) for _ in range(3))
    zero.set_path_margins(mass=0.0, glide=0.0, tilt=0.0, rate=0.0)
    cleared.set_path_margins(mass=1e-4, glide=0.1, tilt=0.2, rate=0.3 * p.omMax).set_path_margins()
    assert not zero.path_margins().any() and not cleared.path_margins().any() and not plain.path_margins().any()
    for step in range(2):
        ref = _state(plain, plain.solve_step())
        for name, b in (("zero", zero), ("cleared", cleared)):
            got = _state(b, b.solve_step())
            for a0, a1 in zip(ref, got):
                assert np.array_equal(a0, a1, equal_nan=True), (name, step)
    # reset keeps the back-offs, init clears them; the thrust ones are left alone by all of it
    pm = np.zeros((B, p.K + 1, 4))
    pm[:, 1:p.K, pr.TILT] = 0.05
    pm[:, 1:, pr.MASS] = 1e-5
    _set(zero, pm)
    assert not zero.thrust_margins()[0].any()
    zero.reset()
    assert np.array_equal(zero.path_margins(), pm)
    zero.init(ic)
    assert not zero.path_margins().any()
    got = _state(zero, zero.solve_step())
    plain.init(ic)
    for a0, a1 in zip(_state(plain, plain.solve_step()), got):
        assert np.array_equal(a0, a1, equal_nan=True)
    for b in (plain, zero, cleared):
        b.close()
    c.close()


@pytest.mark.parametrize("tiles,K", [("double", 50), ("float", 50), ("double", 100)], ids=["double", "float", "double K100"])
def test_path_backoffs_of_one_trajectory_disturb_no_other(tiles, K):
    import bench
    from successiveconvexification_amd import sample_problems as sp
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache
    p = sp.base_prob_scaled if K == 50 else replace(sp.base_prob_scaled, K=K)
    B = 4
    ic = bench.disperse_ics(p, 0, B, 20261018)
    c = IntegratorCache(p, npts=10)
    plain, marg = (ScvxBatch(c, B).set_linearization_f32(tiles == "float").init(ic) for _ in range(2))
    sqcm = pr.consts(p)[1]
    pm = np.zeros((B, p.K + 1, 4))
    pm[1, :p.K, pr.TILT] = 0.5 * sqcm
    pm[1, 1:p.K, pr.RATE] = 0.5 * p.omMax
    pm[1, 1:p.K, pr.GLIDE] = 0.05
    pm[1, 1:, pr.MASS] = 0.1 * (p.mwet - p.mdry)
    _set(marg, pm)
    assert np.array_equal(marg.path_margins(), pm)
    others = [0, 2, 3]
    for step in range(2):
        r0, r1 = _state(plain, plain.solve_step()), _state(marg, marg.solve_step())
        for a0, a1 in zip(r0, r1):
            assert np.array_equal(a0[others], a1[others], equal_nan=True), step
        d = float(np.abs(r0[3][1] - r1[3][1]).max())
        print("%s tiles, K = %d, step %d: trajectory 1 moved by %.3e, statuses %s / %s" % (tiles, K, step, d, r0[0], r1[0]))
        assert d > 1e-4
    for b in (plain, marg):
        b.close()
    c.close()


def test_full_run_from_the_straight_line_guess_under_tilt_backoffs():
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache
    g = _fixture()
    pp, po = _flyable()
    ic, pm = g["run0_ic"][None], g["run0_pm"][None]
    c = IntegratorCache(pp, npts=10)
    b = _set(ScvxBatch(c, 1).init(ic), pm)
    st, it, nu, dj = b.solve()
    x, u, s = b.trajectory()
    # the accept / reject sequence, from a twin stepped one solve_step at a time
    twin = _set(ScvxBatch(c, 1).init(ic), pm)
    seq = ""
    for _ in range(pp.imax - 1):
        s1 = twin.solve_step()[0]
        seq += "r" if s1[0] == 2 else "a"
        if s1[0] not in (1, 2):
            break
    want = "".join("a" if a else "r" for a in g["run0_accepted"])
    gx = g["run0_x"]
    viol, oviol = float(-min(pr.slacks(po, x[0], pm[0])[:, pr.TILT].min(), 0.0)), float(g["run0_viol"])
    print("status %s iters %s; sequence %s (oracle %s)" % (st, it, seq, want))
    print("final mass %.6f (oracle %.6f); device-vs-oracle: mass %.2e r %.2e v %.2e | q %.2e w %.2e u %.2e sigma %.2e (the last four: printed only)"
          % (x[0, -1, 0], gx[-1, 0], abs(x[0, -1, 0] - gx[-1, 0]), np.abs(x[0, :, 1:4] - gx[:, 1:4]).max(), np.abs(x[0, :, 4:7] - gx[:, 4:7]).max(),
             np.abs(x[0, :, 7:11] - gx[:, 7:11]).max(), np.abs(x[0, :, 11:] - gx[:, 11:]).max(), np.abs(u[0] - g["run0_u"]).max(),
             abs(s[0] - float(g["run0_sigma"]))))
    print("tightened tilt cone violated by %.2e (oracle's own run %.2e, bound ten times that)" % (viol, oviol))
    assert st[0] == 0, (st, it)
    assert want == "arrrrrrraaaaa" and seq == want and int(it[0]) == len(want)
    assert abs(x[0, -1, 0] - gx[-1, 0]) < 1e-4
    assert np.abs(x[0, :, 1:4] - gx[:, 1:4]).max() < 1e-4 and np.abs(x[0, :, 4:7] - gx[:, 4:7]).max() < 1e-4
    assert viol <= 10.0 * oviol
    _audit_shows_the_headroom(b, po, x, u, pm)
    b.close(), twin.close(), c.close()


def _audit_shows_the_headroom(b, po, x, u, pm):
    """The flight check keeps auditing against the TRUE cone, so the headroom shows as a negative G_TILT at the nodes.  The report
    keeps one figure, the maximum of |q[3:4]| - sqcm over ALL its samples, and for the plan as it stands that one cannot be negative:
    node 0 carries no back-off (psig is 0 there by definition and q_0 is free), the plan rides the true cone at node 0 as every plan
    here does, and the flown state bulges past it between nodes 0 and 1 (the oracle's own run has slack 0 at node 0 too).  So the audit
    kernel is asked for the nodes that carry a back-off: mode "plan" restarts at every planned node, a time scale of 1e-9 keeps every
    sample of a segment on its node (to 1e-9), and node 0 is replaced by a copy of node 1.  Its G_TILT is then the maximum of the tilt
    function over the nodes 1..K-1, and must be below minus the smallest back-off there (to the solver's 1e-6) -- and agree with the
    same function formed here from the states.  The report of the plan as flown is printed."""
    from successiveconvexification_amd.dynamics import flight_check_batch
    K = po.K
    sqcm = pr.consts(po)[1]
    flown = b.flight_check(mode="plan")
    xs, us = x.copy(), u.copy()
    xs[:, 0], us[:, 0] = xs[:, 1], us[:, 1]
    nodes = flight_check_batch(b.cache, xs, us, np.full(x.shape[0], 1e-9), mode="plan")
    gk = np.linalg.norm(x[:, 1:K, 9:11], axis=-1) - sqcm                     # the audit's function at the planned nodes 1..K-1
    t = pm[:, 1:K, pr.TILT]
    print("G_TILT of the audit at the nodes 1..K-1: %s (formed here: %s; smallest back-off there %s); at node 0: %s; of the plan as flown, "
          "all samples: %s" % (nodes.G_TILT, gk.max(axis=1), t.min(axis=1), np.linalg.norm(x[:, 0, 9:11], axis=-1) - sqcm, flown.G_TILT))
    assert (t > 0).all()
    assert np.all(nodes.G_TILT < 0) and np.all(nodes.G_TILT <= -t.min(axis=1) + 1e-6)
    assert np.abs(nodes.G_TILT - gk.max(axis=1)).max() < 1e-8
    assert (gk <= -t + 1e-6).all()                                           # node by node, each against its own back-off


@pytest.fixture(scope="module")
def robustified():
    """(cache, base batch, robustified batch, S0, psig of the base plans, robustify's return, path back-offs) on the fixture's starts,
    made once and closed when the module is done"""
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache
    ic = np.load(os.path.join(GOLDEN, "oracle_flight_runs.npz"))["ic"]
    pp, po = _flyable()
    c = IntegratorCache(pp, npts=10)
    base, rob = (ScvxBatch(c, ic.shape[0]).init(ic) for _ in range(2))
    st0 = base.solve()[0]
    rob.solve()
    assert np.all(st0 == 0), st0
    S0 = _s0(base.trajectory()[0])
    psig = rob.path_sigma(S0)
    out = rob.robustify(S0, nsigma=3, rounds=1, constraints=("thrust", "tilt"))
    yield c, base, rob, S0, psig, out, rob.path_margins()
    base.close(), rob.close(), c.close()


def test_robustify_restores_the_tilt_and_thrust_headroom(robustified):
    from successiveconvexification_amd import _lib
    pp, po = _flyable()
    c, base, rob, S0, psig, (st, it, nu, dj, lo, hi), pm = robustified
    sqcm = pr.consts(po)[1]
    before, after = base.covariance(S0), rob.covariance(S0)
    x0, xr = base.trajectory()[0], rob.trajectory()[0]
    print("replan: status %s in %s steps; final mass %s -> %s" % (st, it, x0[:, -1, 0], xr[:, -1, 0]))
    print("N_TILT %s -> %s, N_TMIN %s -> %s, N_TMAX %s -> %s; N_GLIDE %s -> %s, N_RATE %s -> %s, N_MASS %s -> %s; tilt back-offs up to %s"
          % (before.N_TILT, after.N_TILT, before.N_TMIN, after.N_TMIN, before.N_TMAX, after.N_TMAX, before.N_GLIDE, after.N_GLIDE, before.N_RATE,
             after.N_RATE, before.N_MASS, after.N_MASS, pm[:, :, pr.TILT].max(axis=1)))
    assert np.all(st == 0), (st, it)                             # both CONVERGED: a solver failure is a finding, not a case to skip
    want = np.minimum(3.0 * psig[:, :, _lib.PSIG_INDEX["TILT"]], 0.25 * sqcm)
    want[:, pp.K] = 0.0
    assert np.array_equal(pm[:, :, pr.TILT], want) and not pm[:, :, [pr.MASS, pr.GLIDE, pr.RATE]].any()
    band = pp.Tmax - pp.Tmin
    assert np.array_equal(lo, np.minimum(3.0 * psig[:, :, _lib.PSIG_INDEX["THRUST"]], 0.25 * band)) and np.array_equal(hi, lo)
    assert np.all(before.N_TILT <= 1e-4)
    assert np.all(after.N_TILT >= 2.0)
    assert np.all(after.N_TMIN >= 2.0) and np.all(after.N_TMAX >= 2.0)
    # the replanned trajectories hold the cone they were given; the audit shows the headroom against the true one
    for t in range(xr.shape[0]):
        assert pr.slacks(po, xr[t], pm[t])[:, pr.TILT].min() > -1e-6
    _audit_shows_the_headroom(rob, po, xr, rob.trajectory()[1], pm)
    # the default is the call it always was, and leaves the path back-offs untouched
    assert len(base.robustify(S0)) == 6 and not base.path_margins().any()


def _consts(p):
    """the constants as scvx_batch_create forms them (libm, not numpy): itan, sqcm"""
    d2r = math.pi / 180.0
    return 1.0 / math.tan(p.gammaGs * d2r), math.sqrt((1.0 - math.cos(p.thetaMax * d2r)) / 2.0)


def _formula(p, x, psig, nsigma, cap):
    """(lo = hi [B][K+1], pm [B][K+1][4]) of scvx_batch_margins_from_cov with every constraint selected"""
    K = p.K
    itan, sqcm = _consts(p)
    pm = np.zeros(psig.shape[:2] + (4,))
    pm[..., pr.MASS] = np.minimum(nsigma * psig[..., 0], cap * (p.mwet - p.mdry))
    pm[..., pr.GLIDE] = np.minimum(nsigma * psig[..., 1], cap * (np.maximum(x[..., 1], 0.0) * itan))
    pm[..., pr.TILT] = np.minimum(nsigma * psig[..., 2], cap * sqcm)
    pm[..., pr.RATE] = np.minimum(nsigma * psig[..., 3], cap * p.omMax)
    pm[:, K, [pr.GLIDE, pr.TILT, pr.RATE]] = 0.0
    pm[:, 0, [pr.MASS, pr.GLIDE, pr.RATE]] = 0.0
    return np.minimum(nsigma * psig[..., 4], cap * (p.Tmax - p.Tmin)), pm


def _plans(K, tiles_f32=False):
    """(problem, cache, B = 2 batch, x, u, sigma): at K = 50 the oracle's converged plans (oracle_flight_runs.npz) set into a batch; at
    another horizon the dispersed flyable batch after three solve_steps (horizon_cases.flyable_batch)"""
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache
    pp = _flyable()[0]
    if K == pp.K:
        g = np.load(os.path.join(GOLDEN, "oracle_flight_runs.npz"))
        c = IntegratorCache(pp, npts=10)
        b = ScvxBatch(c, 2).set_linearization_f32(tiles_f32).init(g["ic"])
        b.set_trajectory(g["x"], g["u"], g["sigma"])
        return pp, c, b, g["x"], g["u"], g["sigma"]
    import horizon_cases as hc
    c, b = hc.flyable_batch(K, tiles_f32=tiles_f32)
    return (replace(pp, K=K), c, b) + b.trajectory()


def _capped(p, x, psig, pm, cap):
    """the "every entry capped" assertions as they follow from _formula on the plan in use: wherever s > 0 and the node has such a row,
    nsigma = 1e9 leaves the cap times the width (the glide width is that of the plan's own altitude, 0 where it is below ground)"""
    K = p.K
    itan, sqcm = _consts(p)
    width = np.zeros(pm.shape)
    width[..., pr.MASS], width[..., pr.TILT], width[..., pr.RATE] = cap * (p.mwet - p.mdry), cap * sqcm, cap * p.omMax
    width[..., pr.GLIDE] = cap * (np.maximum(x[..., 1], 0.0) * itan)
    has_row = np.ones(pm.shape, bool)
    has_row[:, K, [pr.GLIDE, pr.TILT, pr.RATE]] = False
    has_row[:, 0, [pr.MASS, pr.GLIDE, pr.RATE]] = False
    live = has_row & (psig[..., :4] > 0)
    assert live[:, 1:K].all() and live[:, K, pr.MASS].all()       # S0 > 0 reaches every later node: every entry that has a row is capped
    assert np.array_equal(pm[live], width[live]) and not pm[~live].any()
    assert not pm[:, K, [pr.GLIDE, pr.TILT, pr.RATE]].any() and not pm[:, 0].any()


def test_margins_from_cov_is_the_formula_exactly():
    _margins_from_cov_is_the_formula(50)


@pytest.mark.parametrize("K", [64, 100])
def test_margins_from_cov_is_the_formula_exactly_where_the_node_loop_takes_a_second_lap(K):
    """K + 1 = 65 puts one node, K + 1 = 101 puts 37 nodes into the second lap of margins_from_psig_kernel's node-strided loop"""
    _margins_from_cov_is_the_formula(K)


def _margins_from_cov_is_the_formula(K):
    pp, c, b, x, u, s = _plans(K)
    S0 = _s0(x)
    # every constraint, uncapped almost everywhere
    psig = b.margins_from_cov(S0, "all", nsigma=3.0, cap=0.25)
    assert np.array_equal(psig, b.path_sigma(S0))
    lo, pm = _formula(pp, x, psig, 3.0, 0.25)
    for name, got, want in (("thrust lo", b.thrust_margins()[0], lo), ("thrust hi", b.thrust_margins()[1], lo), ("path", b.path_margins(), pm)):
        print("%s: largest %.3e, differs in %d entries" % (name, want.max(), int((got != want).sum())))
        assert np.array_equal(got, want), name
    assert psig.shape == (2, K + 1, 5) and pm.shape == (2, K + 1, 4)
    if K == 50:          # the oracle's converged plans: above ground and uncapped at every node
        assert (pm[:, 1:K] > 0).all() and (pm[:, 1:K, pr.TILT] < 0.25 * _consts(pp)[1]).all()
    assert (pm[:, 1:K, [pr.MASS, pr.TILT, pr.RATE]] > 0).all() and (lo[:, 1:] > 0).all()
    # every entry capped
    psig2 = b.margins_from_cov(S0, "all", nsigma=1e9, cap=0.125)
    lo2, pm2 = _formula(pp, x, psig2, 1e9, 0.125)
    assert np.array_equal(psig2, psig) and np.array_equal(b.path_margins(), pm2) and np.array_equal(b.thrust_margins()[1], lo2)
    _capped(pp, x, psig2, pm2, 0.125)
    assert np.all(lo2[:, 1:] == 0.125 * (pp.Tmax - pp.Tmin)) and not lo2[:, 0].any()
    if K == 50:
        assert np.all(pm2[:, 1:K, pr.TILT] == 0.125 * _consts(pp)[1]) and np.all(pm2[:, 1:K, pr.RATE] == 0.125 * pp.omMax)
        assert np.all(pm2[:, 1:, pr.MASS] == 0.125 * (pp.mwet - pp.mdry)) and np.all(pm2[:, 1:K, pr.GLIDE] == 0.125 * (x[:, 1:K, 1] * _consts(pp)[0]))
        assert not pm2[:, K, [pr.GLIDE, pr.TILT, pr.RATE]].any() and not pm2[:, 0].any()
    # an unselected constraint is left alone: tilt again at other settings, everything else as it was
    b.margins_from_cov(S0, ("tilt",), nsigma=2.0, cap=0.25)
    got = b.path_margins()
    assert np.array_equal(got[..., pr.TILT], _formula(pp, x, psig, 2.0, 0.25)[1][..., pr.TILT])
    assert np.array_equal(got[..., [pr.MASS, pr.GLIDE, pr.RATE]], pm2[..., [pr.MASS, pr.GLIDE, pr.RATE]]) and np.array_equal(b.thrust_margins()[0], lo2)
    # the thrust call keeps its behaviour and leaves the path back-offs alone
    b._margins_from_cov(S0, None, None, None, None, 3.0, 0.25, False)
    assert np.array_equal(b.thrust_margins()[0], lo) and np.array_equal(b.path_margins(), got)
    # a batch without path back-offs has zeros in the unselected columns
    b.set_path_margins()
    b.margins_from_cov(S0, ("rate",), nsigma=3.0, cap=0.25)
    assert np.array_equal(b.path_margins()[..., pr.RATE], pm[..., pr.RATE]) and not b.path_margins()[..., [pr.MASS, pr.GLIDE, pr.TILT]].any()
    # a trajectory whose sigma are NaN gets zeros in what is selected, and the other trajectory is what it was
    bad = S0.copy()
    bad[1, 3, 3] = np.nan
    pn = b.margins_from_cov(bad, ("mass", "tilt"), nsigma=3.0, cap=0.25)
    got = b.path_margins()
    assert np.isnan(pn[1]).all() and np.array_equal(pn[0], psig[0])
    assert not got[1][:, [pr.MASS, pr.TILT]].any() and np.array_equal(got[1][:, pr.RATE], pm[1][:, pr.RATE])
    assert np.array_equal(got[0][:, [pr.MASS, pr.TILT, pr.RATE]], pm[0][:, [pr.MASS, pr.TILT, pr.RATE]])
    b.close(), c.close()


def test_arguments_are_refused():
    import ctypes as C
    from successiveconvexification_amd import _lib, sample_problems as sp
    from successiveconvexification_amd.batch import ScvxBatch, _p
    from successiveconvexification_amd.dynamics import IntegratorCache
    p = sp.base_prob_scaled
    c = IntegratorCache(p, npts=10)
    b = ScvxBatch(c, 2)
    K = p.K
    sqcm = pr.consts(p)[1]
    with pytest.raises(_lib.ScvxError, match="scvx_batch_init first"):
        b.set_path_margins(tilt=0.1)
    b.init(None)
    L, h = c._L, b.handle
    err = lambda: L.scvx_last_error(c.handle).decode()   # noqa: E731

    def one(k, col, v):
        a = np.zeros((2, K + 1, 4))
        a[1, k, col] = v
        return a

    for col in range(4):
        for v in (-1e-9, np.nan, np.inf):
            assert L.scvx_batch_set_path_margins(h, _p(one(7, col, v))) == -1 and "finite" in err(), (col, v)
    for col, v in ((pr.TILT, sqcm), (pr.RATE, p.omMax), (pr.MASS, p.mwet - p.mdry), (pr.TILT, 2.0), (pr.RATE, 1e3)):
        assert L.scvx_batch_set_path_margins(h, _p(one(7, col, v))) == -1 and "must hold" in err(), (col, v)
    for k, col in ((K, pr.GLIDE), (K, pr.TILT), (K, pr.RATE), (0, pr.MASS)):
        assert L.scvx_batch_set_path_margins(h, _p(one(k, col, 1e-6))) == -1 and "without a row" in err(), (k, col)
    for col in (pr.GLIDE, pr.RATE):
        assert L.scvx_batch_set_path_margins(h, _p(one(0, col, 1e-6))) == -1 and "node 0" in err(), col
    assert not b.path_margins().any()                            # nothing was set
    ok = one(0, pr.TILT, 0.5 * sqcm)                             # tilt at node 0 is allowed: q_0 is free
    ok[1, 7] = [0.5 * (p.mwet - p.mdry), 123.0, 0.9 * sqcm, 0.9 * p.omMax]
    ok[0, K, pr.MASS] = 1e-5
    assert L.scvx_batch_set_path_margins(h, _p(ok)) == 0 and np.array_equal(b.path_margins(), ok)
    assert L.scvx_batch_get_path_margins(h, None) == -1 and "null" in err()
    q, r, qf = np.ones(14), np.ones(3), np.full(14, 100.0)
    S0 = np.ascontiguousarray(np.broadcast_to(1e-6 * np.eye(14), (2, 14, 14)))
    call = lambda S, w, ns, cap, which: L.scvx_batch_margins_from_cov(h, _p(q), _p(r), _p(qf), S, w, C.c_double(ns), C.c_double(cap),   # noqa: E731
                                                                      C.c_uint(which), None)
    assert call(None, None, 3.0, 0.25, 31) == -1 and "null" in err()
    for ns in (-1.0, np.nan, np.inf):
        assert call(_p(S0), None, ns, 0.25, 31) == -1 and "nsigma" in err(), ns
    for cap in (0.0, 0.5, -0.1, np.nan):
        assert call(_p(S0), None, 3.0, cap, 31) == -1 and "cap" in err(), cap
    for which in (0, 32, 64 + 8):
        assert call(_p(S0), None, 3.0, 0.25, which) == -1 and "which" in err(), which
    bad_w = np.zeros(14)
    bad_w[3] = -1.0
    assert call(_p(S0), _p(bad_w), 3.0, 0.25, 31) == -1 and "w must be" in err()
    assert np.array_equal(b.path_margins(), ok) and not b.thrust_margins()[0].any()   # the refused calls left everything alone
    with pytest.raises(ValueError):
        b.robustify(S0, constraints=("gimbal",))
    b.close(), c.close()
