"""Back-offs taken from the navigation analysis on the MI355X (scvx_nav_path_sigma_f64, scvx_batch_margins_from_nav, robustify(nav=...);
include/scvx.h) against the independent CPU reference (tests/nav_margin_reference.py; fixture tests/golden/oracle_nav_margin_runs.npz)
and against the properties that define the feature.

Bounds, none of them taken from the device:
  * path sigma: the rule of test_gpu_margins.py on the joint -- with e_ref the largest difference between the float64 and the
    longdouble reference of a column, the device must be within max(16 e_ref, K N 2^-52 max|column|) of the longdouble reference,
    N = n + 14 the depth of the joint's inner products;
  * the reports of the path-sigma launch, the back-offs against the numpy formula, the batch form against the one-shot form, the
    isolation of a poisoned trajectory: bit for bit;
  * robustify(nav=...): CONVERGED, the oracle's 3 steps on plan 0, N_TMIN and N_TMAX of the NAVIGATION report >= 2 afterwards (the
    oracle: 2.76 and 2.99 on plan 0; the slack is for s_T moving with the plan, as in test_gpu_margins.py) while the twin backed off by
    the covariance analysis keeps less than 2 on plan 0 (the oracle: 1.33); final mass of plan 0 within 1e-4 of the oracle's replan
    (the project's contract for a complete run);
  * flights on sampled estimates: fewer commanded node controls outside the band after navigation back-offs than after covariance
    ones, fewer after those than on the base plan (first order on plan 0: 13 < 201 < 3,935 over 256 flights x 51 nodes).
Every comparison prints its figures before it asserts.
"""
import ctypes as C
import os

import numpy as np
import pytest

import cov_reference as cr
import margin_reference as mr
import nav_margin_reference as nm
import track_reference as tr
from conftest import GOLDEN
from test_gpu_flight import _case, _flyable
from test_gpu_nav import _model

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
WEIGHTS = ((1.0, 1.0, 100.0), (1.0, 1e-2, 1e4))
NOISE = np.random.default_rng(5).uniform(0.0, 1e-8, 14)
_ROB = {}


def _fixture():
    return np.load(os.path.join(GOLDEN, "oracle_nav_margin_runs.npz"))


def _s0(x):
    return np.stack([cr.handover_s0(x[b, 0], 0, 1e-3)[0] for b in range(x.shape[0])])


def _nav_model(m, x0):
    """(H, rm): m = 0 none, 3 the fixture's position-only model, 6 test_gpu_nav.py's position and velocity"""
    return nm.position_model(x0) if m == 3 else _model(m, x0)


def _check_psig(tag, po, K, N, got, p64, pld):
    from successiveconvexification_amd import _lib
    assert got.shape == p64.shape == (got.shape[0], K + 1, _lib.PSIG_N) and np.isfinite(got).all() and not got[:, 0].any()
    for i, name in enumerate(_lib.PSIG_COLUMNS):
        e_ref = float(np.abs(p64[..., i] - pld[..., i]).max())
        bound = max(16.0 * e_ref, K * N * EPS * float(np.abs(pld[..., i]).max()))
        e = float(np.abs(got[..., i] - pld[..., i]).max())
        print("%s %-6s: device-vs-longdouble %.3e (float64 reference %.3e, bound %.3e), max %.3e" % (tag, name, e, e_ref, bound, float(np.abs(pld[..., i]).max())))
        assert e <= bound, (tag, name, e, bound)


def _parity(tag, c, po, x, u, d):
    """the one-shot call on the plans x, u with the tiles d: every m, w and weight set against the longdouble reference; the reports of
    the same launch are scvx_nav_cov_f64's bit for bit"""
    from successiveconvexification_amd import _lib
    from successiveconvexification_amd.dynamics import nav_cov_batch, nav_path_sigma_batch
    K, N = po.K, 28 + c.nu
    S0 = _s0(x)
    N0 = S0.copy()
    for w in WEIGHTS:
        L, _ = tr.gains(d, K, *w)                                # the REFERENCE's gains, fed to both sides
        for m in (0, 3, 6):
            H, rm = _nav_model(m, x[0, 0])
            for nz in (None, NOISE):
                p64 = nm.path_sigma(po, x, u, d, K, L, S0, N0, H, rm, nz)
                pld = nm.path_sigma(po, x, u, d, K, L, S0, N0, H, rm, nz, dtype=np.longdouble)
                rep, got = nav_path_sigma_batch(c, x, u, d, L, S0, N0, H, rm, nz)
                _check_psig("%s weights %s m = %d w %s" % (tag, w, m, "0" if nz is None else "> 0"), po, K, N, got, p64, pld)
                plain = nav_cov_batch(c, x, u, d, L, S0, N0, H, rm, nz)
                assert np.array_equal(rep.raw, plain.raw, equal_nan=True) and np.array_equal(rep.navraw, plain.navraw, equal_nan=True)
                assert np.array_equal(got[:, :, _lib.PSIG_INDEX["THRUST"]].max(axis=1), plain.S_THRUST)


def test_path_sigma_golden_plans_against_the_longdouble_reference():
    from successiveconvexification_amd.dynamics import IntegratorCache, cov_path_sigma_batch, linearize_batch, nav_path_sigma_batch
    g = np.load(os.path.join(GOLDEN, "oracle_flight_runs.npz"))
    pp, po = _flyable()
    x, u, s = g["x"], g["u"], g["sigma"]
    K = po.K
    c = IntegratorCache(pp, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (K + 1))
    _parity("golden", c, po, x, u, d)
    # the fixture's own arrays, through the device
    f = _fixture()
    L, _ = tr.gains(d, K)
    got = nav_path_sigma_batch(c, x, u, d, L, f["S0"], f["N0"], f["H"], f["rm"])[1]
    pld = nm.path_sigma(po, x, u, d, K, L, f["S0"], f["N0"], f["H"], f["rm"], dtype=np.longdouble)
    _check_psig("fixture", po, K, 31, got, nm.path_sigma(po, x, u, d, K, L, f["S0"], f["N0"], f["H"], f["rm"]), pld)
    # N0 = 0 and w = 0 (process noise is missed by the estimate, so it alone makes eps): the estimate never errs, and psig is the
    # covariance launch's to the same bound (both against the covariance reference)
    for w in WEIGHTS:
        L, _ = tr.gains(d, K, *w)
        S0 = _s0(x)
        p64 = mr.path_sigma(po, x, u, cr.propagate(d, K, L, S0))
        pld = mr.path_sigma(po, x, u, cr.propagate(d, K, L, S0, None, np.longdouble), np.longdouble)
        for m in (0, 3):
            H, rm = _nav_model(m, x[0, 0])
            got = nav_path_sigma_batch(c, x, u, d, L, S0, np.zeros((14, 14)), H, rm)[1]
            _check_psig("N0 = 0, weights %s m = %d vs covariance reference" % (w, m), po, K, 31, got, p64, pld)
            cv = cov_path_sigma_batch(c, x, u, d, L, S0)[1]
            print("   navigation launch vs covariance launch: %.3e" % np.abs(got - cv).max())
    c.close()


def test_path_sigma_unconverged_fin_plans_against_the_longdouble_reference(aero_tables):
    from successiveconvexification_amd.dynamics import IntegratorCache, linearize_batch
    pp, po, dyn, par, x, u, s = _case("aero+fins", aero_tables)
    x, u, s = x[:2], u[:2], s[:2]
    c = IntegratorCache(pp, npts=10)
    assert c.nu == 5
    _, d = linearize_batch(c, x, u, s, 1.0 / (po.K + 1))
    _parity("fins", c, po, x, u, d)
    c.close()


@pytest.mark.parametrize("tiles", ["double", "float"])
def test_batch_call_is_the_formula_and_the_one_shot_call_on_its_own_tiles(tiles):
    _batch_call_is_the_formula(tiles, 50)


@pytest.mark.parametrize("tiles", ["double", "float"])
@pytest.mark.parametrize("K", [64, 100])
def test_batch_call_is_the_formula_where_the_node_loop_takes_a_second_lap(K, tiles):
    """K + 1 = 65 puts one node, K + 1 = 101 puts 37 nodes into the second lap of margins_from_psig_kernel's node-strided loop; the
    plans are test_gpu_path_margins._plans' (a dispersed flyable batch after three solve_steps), the navigation model the fixture's
    kind (nav_margin_reference.position_model) with N0 = S0 as in _parity"""
    _batch_call_is_the_formula(tiles, K)


def _batch_call_is_the_formula(tiles, K):
    from dataclasses import replace
    from successiveconvexification_amd import _lib
    from successiveconvexification_amd.dynamics import nav_path_sigma_batch
    from test_gpu_path_margins import _capped, _formula, _plans
    import path_margin_reference as pr
    pp, c, b, x, u, s = _plans(K, tiles == "float")
    po = replace(_flyable()[1], K=K)
    if K == 50:
        f = _fixture()
        S0, N0, H, rm = f["S0"], f["N0"], f["H"], f["rm"]
    else:
        S0 = _s0(x)
        N0 = S0.copy()
        H, rm = nm.position_model(x[0, 0])
    state = lambda: (b.trajectory_record(),) + b.scalars() + b.flags()   # noqa: E731
    before = state()
    d = b.linearization()[1]                                    # float tiles: widened on the host
    for w in WEIGHTS:
        # the batch's launch (its own tiles, double or float, and gains) against the one-shot launch on the same: bit for bit
        ps = b.margins_from_nav(S0, N0, H, rm, "all", 3.0, 0.25, NOISE, *w)
        one = nav_path_sigma_batch(c, x, u, d, b.track_gains(*w), S0, N0, H, rm, NOISE)[1]
        assert np.array_equal(ps, one)
        assert np.array_equal(b.path_sigma(S0, NOISE, *w, nav=(N0, H, rm)), one)
        # and against the longdouble reference on those tiles and gains
        L = b.track_gains(*w)
        _check_psig("%s tiles, batch, weights %s" % (tiles, w), po, K, 31, ps, nm.path_sigma(po, x, u, d, K, L, S0, N0, H, rm, NOISE),
                    nm.path_sigma(po, x, u, d, K, L, S0, N0, H, rm, NOISE, dtype=np.longdouble))
    psig = b.margins_from_nav(S0, N0, H, rm)
    lo, pm = _formula(pp, x, psig, 3.0, 0.25)
    for name, got, want in (("thrust lo", b.thrust_margins()[0], lo), ("thrust hi", b.thrust_margins()[1], lo), ("path", b.path_margins(), pm)):
        print("%s tiles, all: %s largest %.3e, differs in %d entries" % (tiles, name, want.max(), int((got != want).sum())))
        assert np.array_equal(got, want), name
    assert psig.shape == (2, K + 1, 5) and not psig[:, 0].any()
    assert (pm[:, 1:K, [pr.MASS, pr.TILT, pr.RATE]] > 0).all() and (lo[:, 1:] > 0).all()
    assert not pm[:, K, [pr.GLIDE, pr.TILT, pr.RATE]].any() and not pm[:, 0, [pr.MASS, pr.GLIDE, pr.RATE]].any() and not lo[:, 0].any()
    if K == 50:          # the oracle's converged plans
        assert (pm[:, 1:K] > 0).all() and (lo[:, 1:] > 0).all()
        assert (psig[:, 2:, 4] > b.path_sigma(S0)[:, 2:, 4]).all()                  # navigation errors widen s_T at every node
    # every entry capped, as it follows from the formula on the plan in use
    pcap = b.margins_from_nav(S0, N0, H, rm, "all", nsigma=1e9, cap=0.125)
    locap, pmcap = _formula(pp, x, pcap, 1e9, 0.125)
    assert np.array_equal(pcap, psig) and np.array_equal(b.path_margins(), pmcap) and np.array_equal(b.thrust_margins()[0], locap)
    _capped(pp, x, pcap, pmcap, 0.125)
    assert np.all(locap[:, 1:] == 0.125 * (pp.Tmax - pp.Tmin))
    assert np.array_equal(b.margins_from_nav(S0, N0, H, rm), psig)                  # ... and back to the settings of above
    # psig = NULL: nothing returns, the same back-offs
    b.set_thrust_margins(None, None).set_path_margins()
    assert b._margins_from_nav(S0, (N0, H, rm), None, None, None, None, 3.0, 0.25, False, _lib.MARGIN_BITS["thrust"] | 30) is None
    assert np.array_equal(b.thrust_margins()[0], lo) and np.array_equal(b.thrust_margins()[1], lo) and np.array_equal(b.path_margins(), pm)
    # a subset: the others keep what they had
    mine = np.full((2, K + 1), 1.25e-3)
    b.set_thrust_margins(mine, 2 * mine)
    p2 = b.margins_from_nav(S0, N0, H, rm, ("tilt", "rate"), nsigma=2.0, cap=0.125)
    lo2, pm2 = _formula(pp, x, p2, 2.0, 0.125)
    got = b.path_margins()
    assert np.array_equal(p2, psig)
    assert np.array_equal(got[..., [pr.TILT, pr.RATE]], pm2[..., [pr.TILT, pr.RATE]]) and np.array_equal(got[..., [pr.MASS, pr.GLIDE]], pm[..., [pr.MASS, pr.GLIDE]])
    assert np.array_equal(b.thrust_margins()[0], mine) and np.array_equal(b.thrust_margins()[1], 2 * mine)
    b.margins_from_nav(S0, N0, H, rm, ("thrust",))
    assert np.array_equal(b.thrust_margins()[0], lo) and np.array_equal(b.thrust_margins()[1], lo) and np.array_equal(b.path_margins(), got)
    # a batch without path back-offs has zeros in the unselected columns
    b.set_path_margins()
    b.margins_from_nav(S0, N0, H, rm, ("rate",))
    assert np.array_equal(b.path_margins()[..., pr.RATE], pm[..., pr.RATE]) and not b.path_margins()[..., [pr.MASS, pr.GLIDE, pr.TILT]].any()
    # nsigma * NaN: zeros for that trajectory in what is selected, the other trajectory is what it was
    bad = N0.copy()
    bad[1, 3, 3] = np.nan
    pn = b.margins_from_nav(S0, bad, H, rm, ("thrust", "tilt"))
    assert np.isnan(pn[1]).all() and np.array_equal(pn[0], psig[0])
    got = b.path_margins()
    assert not got[1][:, pr.TILT].any() and not b.thrust_margins()[0][1].any() and not b.thrust_margins()[1][1].any()
    assert np.array_equal(got[1][:, pr.RATE], pm[1][:, pr.RATE])
    assert np.array_equal(got[0][:, [pr.TILT, pr.RATE]], pm[0][:, [pr.TILT, pr.RATE]]) and np.array_equal(b.thrust_margins()[0][0], lo[0])
    for a0, a1 in zip(before, state()):
        assert np.array_equal(a0, a1, equal_nan=True)
    b.close(), c.close()


def test_a_poisoned_trajectory_disturbs_no_other():
    from successiveconvexification_amd.dynamics import IntegratorCache, linearize_batch, nav_path_sigma_batch
    g = np.load(os.path.join(GOLDEN, "oracle_flight_runs.npz"))
    f = _fixture()
    pp, po = _flyable()
    K = po.K
    x, u, s = g["x"], g["u"], g["sigma"]
    c = IntegratorCache(pp, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (K + 1))
    L, _ = tr.gains(d, K)
    S0, N0 = f["S0"], f["N0"]
    for m in (0, 3):
        H, rm = _nav_model(m, x[0, 0])
        good = nav_path_sigma_batch(c, x, u, d, L, S0, N0, H, rm)[1]
        assert np.isfinite(good).all()
        for what in ("tile", "gain", "S0", "N0"):
            for t in (0, 1):
                dn, gn, sn, nn = d.copy(), L.copy(), S0.copy(), N0.copy()
                if what == "tile":
                    dn.reshape(2, K, -1, 14)[t, 30, 2, 5] = np.nan
                elif what == "gain":
                    gn[t, 12, 1, 4] = np.inf
                elif what == "S0":
                    sn[t, 3, 3] = np.nan
                else:
                    nn[t, 3, 5] = np.nan
                rep, bad = nav_path_sigma_batch(c, x, u, dn, gn, sn, nn, H, rm)
                assert np.isnan(bad[t]).all(), (m, what, t)
                assert np.array_equal(bad[1 - t], good[1 - t]), (m, what, t)
                assert np.isnan(rep.raw[t]).all() and np.isnan(rep.navraw[t]).all() and np.isfinite(rep.navraw[1 - t]).all()
    c.close()


def _robustified():
    """(cache, base batch, batch robustified by the covariance analysis, batch robustified by the navigation analysis, the returns of
    the two robustify calls) on the fixture's starts and model, from the device's own converged plans; made once"""
    if not _ROB:
        from successiveconvexification_amd.batch import ScvxBatch
        from successiveconvexification_amd.dynamics import IntegratorCache
        f = _fixture()
        pp, po = _flyable()
        c = IntegratorCache(pp, npts=10)
        base, cov, nav = (ScvxBatch(c, f["ic"].shape[0]).init(f["ic"]) for _ in range(3))
        for b in (base, cov, nav):
            st0 = b.solve()[0]
            assert np.all(st0 == 0), st0
        rc = cov.robustify(f["S0"], nsigma=3, rounds=1)
        rn = nav.robustify(f["S0"], nsigma=3, rounds=1, nav=(f["N0"], f["H"], f["rm"]))
        _ROB["v"] = (c, base, cov, nav, rc, rn)
    return _ROB["v"]


def test_robustify_on_the_navigation_analysis_keeps_the_headroom_the_covariance_one_loses():
    from successiveconvexification_amd import _lib
    f = _fixture()
    pp, po = _flyable()
    c, base, cov, nav, rc, (st, it, nu, dj, lo, hi) = _robustified()
    S0, N0, H, rm = f["S0"], f["N0"], f["H"], f["rm"]
    band = pp.Tmax - pp.Tmin
    r0, r1, r2 = (b.navigation(S0, N0, H, rm) for b in (base, cov, nav))
    c2 = nav.covariance(S0)
    x0, xc, xn = (b.trajectory()[0] for b in (base, cov, nav))
    steps = [int((r >= 0).sum()) for r in f["nav_accepted"]]
    print("navigation back-offs: status %s in %s steps (oracle, plans %s: %s); covariance back-offs: status %s in %s steps"
          % (st, it, list(f["plans"]), steps, rc[0], rc[1]))
    print("final mass: base %s, covariance back-offs %s (oracle %s), navigation back-offs %s (oracle %s)"
          % (x0[:, -1, 0], xc[:, -1, 0], f["cov_x"][:, -1, 0], xn[:, -1, 0], f["nav_x"][:, -1, 0]))
    print("navigation report: N_TMIN base %s, covariance back-offs %s (oracle %s), navigation back-offs %s (oracle %s)"
          % (r0.N_TMIN, r1.N_TMIN, f["cov_navrep_cov"][:, cr.IDX["N_TMIN"]], r2.N_TMIN, f["nav_navrep_cov"][:, cr.IDX["N_TMIN"]]))
    print("navigation report: N_TMAX base %s, covariance back-offs %s (oracle %s), navigation back-offs %s (oracle %s)"
          % (r0.N_TMAX, r1.N_TMAX, f["cov_navrep_cov"][:, cr.IDX["N_TMAX"]], r2.N_TMAX, f["nav_navrep_cov"][:, cr.IDX["N_TMAX"]]))
    print("covariance report of the navigation-robustified plans: N_TMIN %s N_TMAX %s; back-offs up to %s (covariance ones %s)"
          % (c2.N_TMIN, c2.N_TMAX, lo.max(axis=1), rc[4].max(axis=1)))
    assert np.all(st == 0), (st, it)
    assert np.all(rc[0] == 0), rc[:2]
    assert int(it[0]) == steps[0] == 3
    assert np.array_equal(lo, hi) and (lo[:, 1:] > 0).all() and (lo <= 0.25 * band).all() and (lo[:, 2:] > rc[4][:, 2:]).all()
    assert np.all(r2.N_TMIN >= 2.0) and np.all(r2.N_TMAX >= 2.0)
    assert min(r1.N_TMIN[0], r1.N_TMAX[0]) < 2.0
    assert abs(xn[0, -1, 0] - f["nav_x"][0, -1, 0]) < 1e-4
    # the replanned trajectories hold the band they were given, and restarted from create_initial's scalars
    un = np.linalg.norm(nav.trajectory()[1][..., :3], axis=-1)
    assert (un >= pp.Tmin + lo - 1e-6).all() and (un <= pp.Tmax - hi + 1e-6).all()
    assert np.all(it < pp.imax - 1) and np.all(nav.scalars()[2] == it)
    assert len(_lib.PSIG_COLUMNS) == 5


def test_commanded_controls_on_sampled_estimates_leave_the_band_least_often_after_navigation_backoffs():
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.montecarlo import gaussian_handover, nav_error_samples
    f = _fixture()
    pp, po = _flyable()
    c, base, cov, nav, _, _ = _robustified()
    S0, N0, H, rm = f["S0"], f["N0"], f["H"], f["rm"]
    N, P = 256, S0.shape[0]
    counts, expect = {}, {}
    fleet = ScvxBatch(c, N * P).init(np.repeat(f["ic"], N, axis=0))
    dx0 = np.concatenate([gaussian_handover(S0[i], 0, N, 20261018) for i in range(P)])
    for name, b in (("base", base), ("covariance", cov), ("navigation", nav)):
        x, u, s = b.trajectory()
        kf = b.navigation(S0, N0, H, rm, dense=("kf",)).kf
        d = b.linearization()[1]
        fed = np.concatenate([nav_error_samples(d[i], kf[i], H, rm, N0[i], 0, N, 20261019)[0] for i in range(P)])
        fleet.set_trajectory(cr.rep(x, N), cr.rep(u, N), cr.rep(s, N))
        r = fleet.track(dx0, nav=fed, dense=True)
        t = np.linalg.norm(r.ufly[:, :, :3], axis=-1).reshape(P, N, -1)
        counts[name] = ((t < pp.Tmin) | (t > pp.Tmax)).sum(axis=(1, 2))
        ps = b.path_sigma(S0, nav=(N0, H, rm))
        expect[name] = np.array([nm.outside_band(po, u[i], ps[i], N) for i in range(P)])
    print("commanded node controls outside [Tmin, Tmax], %d flights on sampled estimates per plan x %d nodes:" % (N, pp.K + 1))
    for name in counts:
        print("   %-10s %s (first order from the device's per-node sigma: %s)" % (name, counts[name], np.round(expect[name], 1)))
    print("   the oracle's first-order figures on plan 0: base %.0f, covariance %.0f, navigation %.0f"
          % (f["base_outside"][0], f["cov_outside"][0], f["nav_outside"][0]))
    assert np.all(counts["navigation"] < counts["covariance"]) and np.all(counts["covariance"] < counts["base"]), counts
    fleet.close()


def test_rocketland_robustify_takes_the_navigation_model():
    from successiveconvexification_amd import rocketland as rl
    from successiveconvexification_amd.dynamics import IntegratorCache
    f = _fixture()
    pp, po = _flyable()
    from dataclasses import replace
    p = replace(pp, rIi=f["ic"][0, :3], vIi=f["ic"][0, 3:])       # plan 0's start as the problem's own
    c = IntegratorCache(p, npts=10)
    ip, cnu, cdel = rl.solve_problem(p, c)
    assert cnu <= p.nuTol and cdel <= p.delTol
    S0, N0, H, rm = f["S0"][0], f["N0"][0], f["H"], f["rm"]
    ip2, lo, hi = rl.robustify(ip, c, S0, nav=(N0, H, rm))
    rep = rl.navigation(ip2, c, S0, N0, H, rm)
    print("rocketland.robustify(nav=...): back-offs up to %.3g, final mass %.6f (oracle %.6f), navigation report N_TMIN %.2f N_TMAX %.2f"
          % (lo.max(), ip2.about[-1].state[0], f["nav_x"][0, -1, 0], rep.N_TMIN[0], rep.N_TMAX[0]))
    assert lo.shape == (p.K + 1,) and np.array_equal(lo, hi) and lo[0] == 0 and (lo[1:] > 0).all()
    assert rep.N_TMIN[0] >= 2.0 and rep.N_TMAX[0] >= 2.0
    with pytest.raises(ValueError):
        rl.robustify(ip2, c, S0, nav=(N0, H))
    c.close()


def test_arguments_are_refused():
    from successiveconvexification_amd import _lib, sample_problems as sp
    from successiveconvexification_amd.batch import ScvxBatch, _p
    from successiveconvexification_amd.dynamics import IntegratorCache, linearize_batch, track_gains_batch
    p = sp.base_prob_scaled
    c = IntegratorCache(p, npts=10)
    b = ScvxBatch(c, 2).init(None)
    K = p.K
    L, h, bh = c._L, c.handle, b.handle
    err = lambda: L.scvx_last_error(h).decode()   # noqa: E731
    x, u, s = b.trajectory()
    _, d = linearize_batch(c, x, u, s, 1.0 / (K + 1))
    gain = track_gains_batch(c, d)
    S0 = np.ascontiguousarray(np.broadcast_to(1e-6 * np.eye(14), (2, 14, 14)))
    N0 = S0.copy()
    H = np.ascontiguousarray(np.eye(14)[1:4])
    rm = np.full(3, 1e-10)
    rep, navrep, psig = np.full((2, 16), 7.0), np.full((2, 8), 7.0), np.full((2, K + 1, 5), 7.0)
    dev = lambda v: C.c_void_p(1) if v is not None else None   # noqa: E731  the checks come before any device pointer is used

    def bad(a, v):
        a = np.array(a, float)
        a.flat[2] = v
        return a

    Hbig = np.ascontiguousarray(np.eye(14)[[0] * 15])
    cases = [(dict(psig=None), "psig"), (dict(N0=None), "N0"), (dict(m=15, H=Hbig, rm=np.full(15, 1e-10)), "m must be"),
             (dict(rm=bad(rm, 0.0)), "rm must be"), (dict(H=bad(H, np.inf)), "H must be"), (dict(H=bad(H, np.nan)), "H must be"),
             (dict(navrep=None), "null"), (dict(S0=None), "null"), (dict(K=K - 1), "K must equal"), (dict(w=bad(np.zeros(14), -1.0)), "w must be")]
    for kw, word in cases:
        v = dict(B=2, K=K, x=x, u=u, d=d, gain=gain, S0=S0, N0=N0, m=3, H=H, rm=rm, w=None, rep=rep, navrep=navrep, psig=psig)
        v.update(kw)
        ptr = lambda n: None if v[n] is None else _p(np.ascontiguousarray(v[n]))   # noqa: E731
        hostp = [ptr("H"), ptr("rm"), ptr("w")]
        a_host = [v["B"], v["K"], ptr("x"), ptr("u"), ptr("d"), ptr("gain"), ptr("S0"), ptr("N0"), v["m"]] + hostp + [ptr("rep"), ptr("navrep"), ptr("psig")]
        a_dev = ([v["B"], v["K"]] + [dev(v[n]) for n in ("x", "u", "d", "gain", "S0", "N0")] + [v["m"]] + hostp
                 + [dev(v["rep"]), dev(v["navrep"]), dev(v["psig"])])
        for fn, a in ((L.scvx_nav_path_sigma_f64_host, a_host), (L.scvx_nav_path_sigma_f64, a_dev)):
            assert fn(h, *a) == -1, (kw, fn)
            assert word in err(), (kw, err())
    assert np.all(rep == 7.0) and np.all(navrep == 7.0) and np.all(psig == 7.0)       # nothing ran
    # the batch call: every refusal leaves the back-offs and the batch as they were
    lo = np.full((2, K + 1), 0.1 * (p.Tmax - p.Tmin))
    pm = np.zeros((2, K + 1, 4))
    pm[:, 1:K, 2] = 1e-3
    b.set_thrust_margins(lo, 2 * lo)
    L.scvx_batch_set_path_margins(bh, _p(pm))
    before = (b.trajectory_record(),) + b.scalars() + b.flags()
    q, r, qf = np.ones(14), np.ones(3), np.full(14, 100.0)

    def call(**kw):
        v = dict(S0=_p(S0), N0=_p(N0), m=3, H=_p(H), rm=_p(rm), w=None, ns=3.0, cap=0.25, which=31, r=_p(r))
        v.update(kw)
        return L.scvx_batch_margins_from_nav(bh, _p(q), v["r"], _p(qf), v["S0"], v["N0"], v["m"], v["H"], v["rm"], v["w"], C.c_double(v["ns"]),
                                             C.c_double(v["cap"]), C.c_uint(v["which"]), _p(psig))

    assert call(N0=None) == -1 and "N0" in err()
    assert call(S0=None) == -1 and "S0" in err()
    assert call(m=15, H=_p(Hbig), rm=_p(np.full(15, 1e-10))) == -1 and "m must be" in err()
    assert call(m=-1) == -1 and "m must be" in err()
    assert call(rm=_p(bad(rm, 0.0))) == -1 and "rm must be" in err()
    assert call(rm=_p(bad(rm, np.nan))) == -1 and "rm must be" in err()
    assert call(H=_p(bad(H, np.inf))) == -1 and "H must be" in err()
    assert call(H=None) == -1 and "needs H" in err()
    for ns in (-1.0, np.nan, np.inf):
        assert call(ns=ns) == -1 and "nsigma" in err(), ns
    for cap in (0.0, 0.5, -0.1, np.nan):
        assert call(cap=cap) == -1 and "cap" in err(), cap
    for which in (0, 32, 64 + 8):
        assert call(which=which) == -1 and "which" in err(), which
    assert call(w=_p(bad(np.zeros(14), -1.0))) == -1 and "w must be" in err()
    assert call(r=_p(np.zeros(3))) == -1
    assert np.all(psig == 7.0)
    assert np.array_equal(b.thrust_margins()[0], lo) and np.array_equal(b.thrust_margins()[1], 2 * lo) and np.array_equal(b.path_margins(), pm)
    for a0, a1 in zip(before, (b.trajectory_record(),) + b.scalars() + b.flags()):
        assert np.array_equal(a0, a1, equal_nan=True)
    # the host layer refuses a malformed model itself
    with pytest.raises(ValueError):
        b.robustify(S0, nav=(N0, H, 0.0))
    with pytest.raises(ValueError):
        b.margins_from_nav(S0, N0, H[:, :13], rm)
    # and a good call goes through: m = 0 (no measurement) included
    assert call(m=0, H=None, rm=None, which=1) == 0 and np.isfinite(psig).all() and not psig[:, 0].any()
    b.close(), c.close()
