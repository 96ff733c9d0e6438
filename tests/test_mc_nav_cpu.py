"""Sampled closed-loop dispersion flown on a navigation estimate, without a GPU: the three bindings of the new calls (header,
_lib.SIGNATURES, julia/ScvxAMD.jl) against each other, the draws (montecarlo.mc_nav_draws), dynamics.McNavReport, the reference's error
recursion (tests/mc_nav_reference.py) against montecarlo.nav_error_samples where the two models coincide (w = 0), and the statistical
check of the W term of the navigation analysis: the C oracle's closed loop flown on an estimate whose error receives the process noise
the truth receives, against Xi_K of tests/nav_reference.py WITH w -- the first comparison of that term with a nonlinear flight.

Data: the two plans the oracle converges on (tests/golden/oracle_flight_runs.npz), tiles from oracle.dynamics.linearize."""
import os
import re

import numpy as np
import pytest

import cov_reference as cr
import mc_nav_reference as mn
import mc_reference as mr
import nav_reference as nr
import track_reference as tr
from conftest import ROOT
from test_cov_cpu import _data
from test_nav_cpu import pv_model

NAV_SAMPLES = 8192      # the C oracle flies them in well under a minute
NAV_SEED = 20261019


def test_header_binding_and_julia_carry_the_new_symbols():
    from successiveconvexification_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "scvx.h")).read()
    jl = open(os.path.join(ROOT, "julia", "ScvxAMD.jl")).read()
    nargs = {"scvx_track_mc_nav_f64": 34, "scvx_track_mc_nav_f64_host": 34, "scvx_batch_track_mc_nav": 30}
    for sym, n in nargs.items():
        m = re.search(r"\bint %s\(([^;]*?)\);" % sym, hdr, flags=re.S)
        assert m, sym
        assert len(m.group(1).split(",")) == n, sym
        assert len(_lib.SIGNATURES[sym][1]) == n, sym
        j = re.search(r"ccall\(\(:%s, LIB\), Cint,\s*\(([^)]*)\)" % sym, jl, flags=re.S)
        assert j, sym
        assert len([a for a in j.group(1).split(",") if a.strip()]) == n, sym
    # the old calls keep their argument lists and their reserved argument: the estimate is a call of its own
    assert len(_lib.SIGNATURES["scvx_track_mc_f64"][1]) == 22 and len(_lib.SIGNATURES["scvx_batch_track_mc"][1]) == 19
    assert "const void *reserved" in re.search(r"\bint scvx_track_mc_f64\(([^;]*?)\);", hdr, flags=re.S).group(1)
    assert int(re.search(r"#define SCVX_MCNAV_MAX_FED (\d+)", hdr).group(1)) == 5 == _lib.MCNAV_INDEX["MAX_FED"] == mn.MCNAV_IDX["MAX_FED"]
    assert int(re.search(r"const MCNAV_MAX_FED = (\d+)", jl).group(1)) == 5
    assert _lib.MCNAV_COLUMNS == mn.MCNAV_COLUMNS and len(_lib.MCNAV_COLUMNS) == _lib.NAV_NREP
    assert [n for n in _lib.MCNAV_COLUMNS if n != "MAX_FED"] == [n for n in _lib.NAV_COLUMNS if n != "NAV_PEAK"]
    assert int(re.search(r"#define SCVX_ABI_VERSION (\d+)", hdr).group(1)) == 4 == _lib.ABI_VERSION    # no struct, no old signature changed
    # outside install!(): that function's body is pinned to the reference's by test_abi_harness.py
    assert jl.index("function track_mc_nav(b::Batch") < jl.index("function install!")
    assert "track_mc_nav" not in jl[jl.index("function install!"):]
    # the header states the model's limits, and the old call points at the new one
    for word in ("not an EKF re-linearised on the flown state", "the gains are the analysis's gains", "no measurement at node K",
                 "the clamp acts on the command formed from the estimate", "scvx_track_mc_nav_f64 below"):
        assert word in hdr, word


def test_mc_nav_draws_rows_are_shard_independent_and_their_own():
    from successiveconvexification_amd.montecarlo import mc_draws, mc_nav_draws, nav_error_samples
    K, m, seed = 7, 6, 11
    xin, nud = mc_nav_draws(10, K, m, seed)
    assert xin.shape == (10, 14) and nud.shape == (10, K, m)
    again = mc_nav_draws(10, K, m, seed)
    assert np.array_equal(again[0], xin) and np.array_equal(again[1], nud)                   # reproducible
    xs, ns = mc_nav_draws(4, K, m, seed, lo=3)
    assert np.array_equal(xs, xin[3:7]) and np.array_equal(ns, nud[3:7])                   # a shard is the rows of the whole set
    x0, none = mc_nav_draws(10, K, 0, seed)
    assert none is None and np.array_equal(x0, xin)                                        # the start draws do not depend on m
    assert not np.array_equal(mc_nav_draws(10, K, m, seed + 1)[0], xin)
    mine = np.concatenate([xin.reshape(-1), nud.reshape(-1)])
    assert len(np.unique(mine)) == mine.size
    # not the draws of mc_draws or nav_error_samples for the same seed (identity factors: the latter's output IS its draws)
    xi0, eta = mc_draws(10, K, seed, noise=True)
    _, before = nav_error_samples(np.zeros((K, 21, 14)), None, None, None, np.eye(14), 0, 10, seed)
    for other in (xi0, eta, before[:, 0]):
        assert not np.isin(mine, other.reshape(-1)).any()
    big = mc_nav_draws(4096, 2, 3, 3)
    z = np.concatenate([big[0].reshape(-1), big[1].reshape(-1)])
    assert abs(z.mean()) < 6.0 / np.sqrt(z.size) and abs(z.var() - 1.0) < 6.0 * np.sqrt(2.0 / z.size)


def test_mc_nav_report_and_summary():
    from successiveconvexification_amd import _lib
    from successiveconvexification_amd._calls import MC_NAV_DENSE, MC_NAV_REDUCED, dense_names, mc_outputs
    from successiveconvexification_amd.dynamics import McNavReport, McReport, _mc_nav_inputs
    from successiveconvexification_amd.montecarlo import mc_summary
    rng = np.random.default_rng(0)
    raw = rng.uniform(0.0, 1.0, (3, 48))
    raw[:, 45], raw[:, 44] = 64, [0, 2, 0]
    nav = 100.0 + np.arange(24.0).reshape(3, 8)
    rep = McNavReport(raw, np.zeros((3, 14)), np.zeros((3, 14, 14)), np.zeros((3, 28)), np.zeros((3, 28, 28)), nav, navK=np.ones((3, 64, 14)))
    assert isinstance(rep, McReport) and len(rep) == 3 and rep.navfed is None and rep.flights is None and rep.navK.shape == (3, 64, 14)
    for n, i in _lib.MC_INDEX.items():
        assert np.array_equal(getattr(rep, n), raw[:, i])
    for n, i in _lib.MCNAV_INDEX.items():
        assert np.array_equal(getattr(rep, n), nav[:, i])
    assert np.array_equal(rep.MAX_FED, nav[:, 5]) and not hasattr(rep, "NAV_PEAK")
    s = mc_summary(rep, np.zeros(3, int))                                                   # reads it unchanged
    assert s["converged"] == 3 and s["samples"] == 64 and s["plans_with_bad_flights"] == 1 and s["stats"]["P_ANY"]["max"] == raw[:, 41].max()
    assert dense_names(True, MC_NAV_DENSE) == {"flights", "xland", "dx0", "navfed", "navK"} and dense_names((), MC_NAV_DENSE) == set()
    assert dense_names("navK", MC_NAV_DENSE) == {"navK"}
    with pytest.raises(ValueError):
        dense_names(("navfed", "ufly"), MC_NAV_DENSE)
    out = mc_outputs(2, 3, 5, dense_names(("navfed",), MC_NAV_DENSE) | set(MC_NAV_REDUCED))
    red, dn = [out[k] for k in MC_NAV_REDUCED], [out[k] for k in MC_NAV_DENSE]
    assert [a.shape for a in red] == [(2, 48), (2, 14), (2, 14, 14), (2, 28), (2, 28, 28), (2, 8)]
    assert [None if a is None else a.shape for a in dn] == [None, None, None, (2, 5, 3, 14), None]
    c0, cn, n0, xi0, eta, xin, nud, wv = _mc_nav_inputs(np.full(14, 2.0), np.full(14, 0.5), 2, 3, 6, 5, 1, 1e-8, None)
    assert np.array_equal(c0[1], 2.0 * np.eye(14)) and np.array_equal(cn[0], 0.5 * np.eye(14)) and np.array_equal(n0[0], 0.25 * np.eye(14))
    assert xi0.shape == (5, 14) and eta.shape == (5, 3, 14) and xin.shape == (5, 14) and nud.shape == (5, 3, 6) and np.all(wv == 1e-8)
    assert _mc_nav_inputs(np.ones(14), np.ones(14), 1, 3, 0, 5, 1, None, None)[4:7:2] == (None, None)     # no eta, no nud
    with pytest.raises(ValueError):
        _mc_nav_inputs(np.ones(14), np.ones(14), 1, 3, 6, 5, 1, None, (xi0, None, xin, nud[:, :2]))
    with pytest.raises(ValueError):
        _mc_nav_inputs(np.ones(14), np.ones(14), 1, 3, 6, 5, 1, None, (xi0, None))


def test_reference_recursion_is_nav_error_samples_without_process_noise():
    """w = 0: the reference's recursion on the draws nav_error_samples makes is that helper's recursion; with w the two differ from
    node 1 on and only through sqrt(w) eta"""
    from successiveconvexification_amd.montecarlo import handover_factor, nav_error_samples
    p, par, x, u, s, d = _data()
    K, N, seed = p.K, 40, 12
    L, _ = tr.gains(d, K)
    S0, _ = cr.handover_s0(x[0, 0], scale=0.1)
    N0 = 0.25 * S0
    H, rm = pv_model(x[0, 0])
    m = H.shape[0]
    kf = nr.propagate(d[:1], K, L[:1], S0[None], N0[None], H, rm)[1][0]
    fed0, before0 = nav_error_samples(d[0], kf, H, rm, N0, 0, N, seed)
    xi = np.stack([np.random.Generator(np.random.Philox(key=seed, counter=[3, 0, 0, b])).standard_normal(14 + K * m) for b in range(N)])
    xin, nud = np.ascontiguousarray(xi[:, :14]), np.ascontiguousarray(xi[:, 14:].reshape(N, K, m))
    CN = handover_factor(N0)
    for w, eta in ((None, None), (np.zeros(14), np.ones((N, K, 14))), (np.full(14, 1e-9), None)):
        fed, before = mn.eps_recursion(d[0], kf, H, rm, CN, xin, nud, w, eta)
        scale = np.abs(before0).max()
        print("w %s: fed bitwise %s, before bitwise %s, largest difference / max|eps| %.3e"
              % (None if w is None else w[0], np.array_equal(fed, fed0), np.array_equal(before, before0), np.abs(before - before0).max() / scale))
        assert np.abs(fed - fed0).max() <= 64 * 2.0 ** -52 * scale and np.abs(before - before0).max() <= 64 * 2.0 ** -52 * scale
    w = np.full(14, 1e-9)
    eta = np.random.default_rng(1).standard_normal((N, K, 14))
    fed, before = mn.eps_recursion(d[0], kf, H, rm, CN, xin, nud, w, eta)
    assert np.array_equal(fed[:, 0], mn.eps_recursion(d[0], kf, H, rm, CN, xin, nud)[0][:, 0]) and not np.allclose(before[:, 1], before0[:, 1], rtol=1e-6, atol=0)
    # m = 0: no update, the transport alone; longdouble agrees with float64 to rounding
    f0, b0 = mn.eps_recursion(d[0], None, None, None, CN, xin, None)
    assert np.array_equal(f0, b0[:, :K])
    fl, bl = mn.eps_recursion(d[0], kf, H, rm, CN, xin, nud, w, eta, dtype=np.longdouble)
    assert fl.dtype == np.longdouble and np.abs(bl.astype(float) - before).max() <= 1e-9 * np.abs(before).max()


def nav_case():
    """The inputs of the statistical check, shared with tests/test_gpu_mc_nav.py: plan 0 of the golden runs, S0 of
    cov_reference.handover_s0(x0, scale=0.1), N0 = 0.25 S0, r and v measured at every node (test_nav_cpu.pv_model), the default
    weights' reference gains, and w = alpha diag(S0) with alpha such that in the truth block of the navigation propagation the landing
    covariance from w alone has the trace of the one from the handover alone.
    (p, par, x, u, s, d, L, S0, N0, H, rm, w, Xi_K [N][N] with w, kf [K][14][m])"""
    p, par, x, u, s, d = _data()
    sl = slice(0, 1)
    L, _ = tr.gains(d, p.K)
    S0, _ = cr.handover_s0(x[0, 0], scale=0.1)
    H, rm = pv_model(x[0, 0])
    prop = lambda S, w: nr.propagate(d[sl], p.K, L[sl], S[None], 0.25 * S[None], H, rm, w)[0][0, -1]   # noqa: E731
    w, t0, t1 = mr.noise_for_equal_share(prop, S0)
    print("truth block of Xi_K: trace from the handover alone %.4e, from w alone %.4e (ratio %.3f)" % (t0, t1, t1 / t0))
    assert 0.5 <= t1 / t0 <= 2.0
    joint, kf, _ = nr.propagate(d[sl], p.K, L[sl], S0[None], 0.25 * S0[None], H, rm, w)
    return p, par, x, u, s, d, L, S0, 0.25 * S0, H, rm, w, joint[0, -1], kf[0]


def test_navigation_process_noise_against_the_recursion_within_six_standard_errors():
    """S = 8,192 flights of plan 0 through the C oracle's closed loop, fed an estimate whose error follows the reference recursion WITH
    the impulses sqrt(w) eta that the truth receives, against the rows and columns 0:14 and n:n+14 of Xi_K of nav_reference.propagate
    with W: every one of the 28 x 28 entries of the sample covariance of [e; eps_K] within six standard errors (mc_reference.se_check's
    bound), entries over six: 0.  Figures of this run: see the print, and README.md."""
    from oracle import dynamics as od
    from successiveconvexification_amd.montecarlo import handover_factor, mc_draws, mc_nav_draws
    p, par, x, u, s, d, L, S0, N0, H, rm, w, XiK, kf = nav_case()
    N, K, n = NAV_SAMPLES, p.K, 14 + u.shape[-1]
    xi0, eta = mc_draws(N, K, NAV_SEED, noise=True)
    xin, nud = mc_nav_draws(N, K, H.shape[0], NAV_SEED)
    dx0 = xi0 @ handover_factor(S0).T
    CN = handover_factor(N0)
    imp = eta * np.sqrt(w)
    fed, before = mn.eps_recursion(d[0], kf, H, rm, CN, xin, nud, w, eta)
    _, xf, _, _ = mn.fly_plan(od, p, x[0], u[0], s[0], L[0], dx0, fed, 10, 0, imp, par)
    _, jcov, nav = mn.reduce(xf[:, -1] - x[0, -1], before[:, -1], fed)
    worst, over = mn.se_check(jcov, XiK, n, N)
    ref = nr.nav_report(XiK[None, None], n)[0]
    print("C oracle, plan 0, S = %d, seed %d: worst entry of the 28 x 28 joint covariance %.2f standard errors, %d entries over 6; "
          "sampled NAV_R %.3e EST_R %.3e MAX_FED %.3e, analysis NAV_R %.3e EST_R %.3e"
          % (N, NAV_SEED, worst, over, nav[1], nav[6], nav[5], ref[nr.NAV_IDX["NAV_R"]], ref[nr.NAV_IDX["EST_R"]]))
    assert over == 0, (worst, over)
    # the same flights with eps generated WITHOUT process noise -- what montecarlo.nav_error_samples covers today: printed, not asserted
    fed0, before0 = mn.eps_recursion(d[0], kf, H, rm, CN, xin, nud)
    _, xf0, _, _ = mn.fly_plan(od, p, x[0], u[0], s[0], L[0], dx0, fed0, 10, 0, imp, par)
    worst0, over0 = mn.se_check(mn.reduce(xf0[:, -1] - x[0, -1], before0[:, -1], fed0)[1], XiK, n, N)
    print("the same flights with eps generated without process noise against the same Xi_K: worst %.2f standard errors, %d entries over 6"
          % (worst0, over0))
