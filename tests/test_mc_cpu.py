"""Sampled closed-loop dispersion without a GPU: the draws (montecarlo.mc_draws), the three bindings of the new calls (header,
_lib.SIGNATURES, julia/ScvxAMD.jl) against each other, dynamics.McReport / montecarlo.mc_summary, the reference's own impulse and
reduction (tests/mc_reference.py), and the statistical check of the process noise w: the C oracle's closed loop with impulses against
the covariance recursion of tests/cov_reference.py WITH w -- the first comparison of the analyses' w term with a nonlinear flight.

Data: the two plans the oracle converges on (tests/golden/oracle_flight_runs.npz), tiles from oracle.dynamics.linearize."""
import os
import re

import numpy as np
import pytest

import cov_reference as cr
import mc_reference as mr
import track_reference as tr
from conftest import ROOT
from test_cov_cpu import _data

W_SAMPLES = 8192      # the C oracle flies them in well under a minute
W_SEED = 20261019


def test_mc_draws_rows_are_shard_independent_and_their_own():
    from successiveconvexification_amd.montecarlo import gaussian_handover, mc_draws, nav_error_samples
    K, seed = 7, 11
    xi, eta = mc_draws(10, K, seed, noise=True)
    assert xi.shape == (10, 14) and eta.shape == (10, K, 14)
    xi_s, eta_s = mc_draws(4, K, seed, noise=True, lo=3)
    assert np.array_equal(xi_s, xi[3:7]) and np.array_equal(eta_s, eta[3:7])
    xi_n, none = mc_draws(10, K, seed)
    assert none is None and np.array_equal(xi_n, xi)              # the start draws do not depend on the noise
    assert not np.array_equal(mc_draws(10, K, seed + 1)[0], xi)
    assert len(np.unique(np.concatenate([xi.reshape(-1), eta.reshape(-1)]))) == xi.size + eta.size
    # not the draws of the other samplers for the same seed (identity factors: their outputs ARE their draws)
    g = gaussian_handover(np.ones(14), 0, 10, seed)
    _, before = nav_error_samples(np.zeros((K, 21, 14)), None, None, None, np.eye(14), 0, 10, seed)
    assert not np.isin(xi.reshape(-1), g.reshape(-1)).any() and not np.isin(xi.reshape(-1), before[:, 0].reshape(-1)).any()
    big = mc_draws(4096, 1, 3, noise=True)
    z = np.concatenate([big[0].reshape(-1), big[1].reshape(-1)])
    assert abs(z.mean()) < 6.0 / np.sqrt(z.size) and abs(z.var() - 1.0) < 6.0 * np.sqrt(2.0 / z.size)


def test_header_binding_and_julia_carry_the_new_symbols():
    from successiveconvexification_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "scvx.h")).read()
    jl = open(os.path.join(ROOT, "julia", "ScvxAMD.jl")).read()
    nargs = {"scvx_track_mc_f64": 22, "scvx_track_mc_f64_host": 22, "scvx_batch_track_mc": 19}
    for sym, n in nargs.items():
        m = re.search(r"\bint %s\(([^;]*?)\);" % sym, hdr, flags=re.S)
        assert m, sym
        assert len(m.group(1).split(",")) == n, sym
        assert len(_lib.SIGNATURES[sym][1]) == n, sym
        j = re.search(r"ccall\(\(:%s, LIB\), Cint,\s*\(([^)]*)\)" % sym, jl, flags=re.S)
        assert j, sym
        assert len([a for a in j.group(1).split(",") if a.strip()]) == n, sym
    mac = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define SCVX_MC_([A-Z_]+) (\d+)", hdr)}
    assert mac.pop("NREP") == 48 == _lib.MC_NREP == mr.NREP
    assert _lib.MC_COLUMNS == mr.COLUMNS and len(_lib.MC_COLUMNS) == 46
    I = _lib.MC_INDEX
    assert mac == {"MAX": I["MAX_GAP"], "MEAN": I["MEAN_GAP"], "P_MASS": I["P_MASS"], "P_ANY": I["P_ANY"], "OUT_LO": I["OUT_LO"],
                   "OUT_HI": I["OUT_HI"], "N_BAD": I["N_BAD"], "S": I["S"]}
    assert (I["MAX_QNORM"], I["MEAN_QNORM"], I["P_FIN"]) == (15, 31, 40)
    assert int(re.search(r"#define SCVX_ABI_VERSION (\d+)", hdr).group(1)) == 4 == _lib.ABI_VERSION
    assert int(re.search(r"const MC_NREP = (\d+)", jl).group(1)) == 48
    # outside install!(): that function's body is pinned to the reference's by test_abi_harness.py
    assert jl.index("function track_mc(b::Batch") < jl.index("function install!")
    assert "track_mc" not in jl[jl.index("function install!"):]


def test_mc_report_and_summary():
    from successiveconvexification_amd._calls import MC_DENSE, dense_names
    from successiveconvexification_amd.dynamics import FlightReport, McReport
    from successiveconvexification_amd.montecarlo import mc_summary
    rng = np.random.default_rng(0)
    raw = rng.uniform(0.0, 1.0, (6, 48))
    raw[:, 45] = 64
    raw[:, 44] = [0, 0, 3, 0, 0, 0]
    raw[:, [13, 29]] = -np.inf                                       # G_DP: not enforced by the model
    fl = rng.uniform(0.0, 1.0, (6, 64, 16))
    rep = McReport(raw, np.zeros((6, 14)), np.zeros((6, 14, 14)), flights=fl)
    assert len(rep) == 6 and np.array_equal(rep.P_ANY, raw[:, 41]) and np.array_equal(rep.MAX_G_TMIN, raw[:, 11])
    assert np.array_equal(rep.MEAN_MISS_R, raw[:, 17]) and np.array_equal(rep.OUT_LO, raw[:, 42]) and np.array_equal(rep.S, raw[:, 45])
    f = rep.flight(2)
    assert isinstance(f, FlightReport) and len(f) == 64 and np.array_equal(f.G_TMIN, fl[2, :, 11]) and f.mode == "track"
    with pytest.raises(ValueError):
        McReport(raw, None, None).flight(0)
    with pytest.raises(ValueError):
        dense_names(("flights", "ufly"), MC_DENSE)
    assert dense_names(True, MC_DENSE) == {"flights", "xland", "dx0"} and dense_names((), MC_DENSE) == set()
    assert dense_names("xland", MC_DENSE) == {"xland"}
    status = np.array([0, 0, 0, 1, 3, 0])
    s = mc_summary(rep, status)
    assert s["n"] == 6 and s["converged"] == 4 and s["samples"] == 64 and s["plans_with_bad_flights"] == 1
    assert s["counts"]["converged"] == 4 and s["counts"]["running"] == 1 and s["counts"]["solver"] == 1 and sum(s["counts"].values()) == 6
    conv = raw[status == 0]
    assert s["stats"]["P_ANY"]["max"] == conv[:, 41].max() and s["stats"]["MEAN_GAP"]["median"] == float(np.median(conv[:, 16]))
    assert s["stats"]["MAX_G_DP"]["max"] == -np.inf and "S" not in s["stats"]
    assert mc_summary(raw, np.full(6, 2))["stats"]["P_ANY"] is None
    with pytest.raises(ValueError):
        mc_summary(raw, status[:5])


def test_reference_impulses_and_reduction():
    """the extended chain: no impulses = track_reference.chain; an impulse moves the node and everything after it, never the sample
    before it; the reduction's columns on a hand-made set of flights"""
    from oracle import dynamics as od
    p, par, x, u, s, d = _data()
    L, _ = tr.gains(d, p.K)
    dx0 = np.zeros((2, 14))
    dx0[:, 1:7] = 1e-3
    S0_, US0, xf0, uf0, cmd0 = tr.chain(od, par, p, x, u, s, L, dx0, 2)
    S1, US1, xf1, uf1, cmd1 = mr.chain(od, par, p, x, u, s, L, dx0, 2)
    for a0, a1 in ((S0_, S1), (US0, US1), (xf0, xf1), (uf0, uf1), (cmd0, cmd1)):
        assert np.array_equal(a0, a1)
    imp = np.zeros((2, p.K, 14))
    imp[:, 9, 4] = 1e-4                                               # after segment 9: node 10
    S2, US2, xf2, uf2, cmd2 = mr.chain(od, par, p, x, u, s, L, dx0, 2, 0, imp)
    assert np.array_equal(S2[:, :10], S1[:, :10]) and np.array_equal(xf2[:, :10], xf1[:, :10]) and np.array_equal(uf2[:, :11], uf1[:, :11])
    assert np.array_equal(xf2[:, 10], S1[:, 9, -1] + imp[:, 9]) and np.array_equal(S2[:, 10, 0], xf2[:, 10])
    assert not np.array_equal(uf2[:, 11], uf1[:, 11]) and not np.array_equal(xf2[:, -1], xf1[:, -1])
    imp = np.zeros((2, p.K, 14))
    imp[:, -1, 2] = 1e-4                                              # the last impulse: the landing row only
    S3, _, xf3, uf3, _ = mr.chain(od, par, p, x, u, s, L, dx0, 2, 0, imp)
    assert np.array_equal(S3, S1) and np.array_equal(uf3, uf1) and np.array_equal(xf3[:, -1], xf1[:, -1] + imp[:, -1])
    # reduction
    fl = np.zeros((5, 16))
    fl[:, 0] = [1.0, 3.0, 2.0, 0.5, 0.1]
    fl[:, 13] = -np.inf
    fl[:, 11] = [-1.0, 0.2, 0.3, -0.1, 0.05]                          # G_TMIN
    fl[:, 6] = [0.2, -1.0, -1.0, -1.0, -1.0]                          # G_MASS
    e = np.arange(70.0).reshape(5, 14) ** 1.5
    r, xm, xc = mr.reduce(fl, e, 7, 3, 10, tol=0.1)
    I = mr.IDX
    assert r[I["MAX_GAP"]] == 3.0 and r[I["MEAN_GAP"]] == 6.6 / 5 and r[I["MAX_G_DP"]] == -np.inf and r[I["MEAN_G_DP"]] == -np.inf
    assert r[I["P_TMIN"]] == 0.4 and r[I["P_MASS"]] == 0.2 and r[I["P_ANY"]] == 0.6 and r[I["P_DP"]] == 0.0
    assert r[I["OUT_LO"]] == 7 / 50 and r[I["OUT_HI"]] == 3 / 50 and r[I["N_BAD"]] == 0 and r[I["S"]] == 5 and not r[46:].any()
    assert np.allclose(xm, e.mean(axis=0), rtol=1e-15) and np.allclose(xc, np.cov(e.T), rtol=1e-13)
    fl[3, 0] = np.nan
    r, _, _ = mr.reduce(fl, e, 0, 0, 10)
    assert np.isnan(r[I["MAX_GAP"]]) and np.isnan(r[I["MEAN_GAP"]]) and r[I["N_BAD"]] == 1 and r[I["MAX_G_TMIN"]] == 0.3
    assert mr.reduce(fl[:1], e[:1], 0, 0, 10)[2].shape == (14, 14) and not mr.reduce(fl[:1], e[:1], 0, 0, 10)[2].any()
    assert mr.out_counts(np.array([0.1, 0.5, np.nan, 0.9]), 0.3, 0.8) == (1, 1)
    assert mr.out_counts(np.array([0.1, 0.5, np.nan, 0.9]), 0.3, 0.8, tol=0.15) == (1, 0)


def w_case():
    """The inputs of the statistical check of w, shared with tests/test_gpu_mc.py: plan 0 of the golden runs, S0 of
    cov_reference.handover_s0(x0, scale=0.1), the default weights' reference gains, and w = alpha diag(S0) with alpha such that the
    landing covariance from w alone has the trace of the one from S0 alone.  (p, par, x, u, s, d, L, S0, w, Sigma_K [n][n] with w)"""
    p, par, x, u, s, d = _data()
    sl = slice(0, 1)
    L, _ = tr.gains(d, p.K)
    S0, _ = cr.handover_s0(x[0, 0], scale=0.1)
    prop = lambda S, w: cr.propagate(d[sl], p.K, L[sl], S[None], w)[0, -1]   # noqa: E731
    w, t0, t1 = mr.noise_for_equal_share(prop, S0)
    print("landing covariance trace from S0 alone %.4e, from w alone %.4e (ratio %.3f); w %s" % (t0, t1, t1 / t0, w))
    assert 0.5 <= t1 / t0 <= 2.0
    return p, par, x, u, s, d, L, S0, w, prop(S0, w)


def test_process_noise_against_the_recursion_within_six_standard_errors():
    """S = 8,192 flights of plan 0 through the C oracle's closed loop, Gaussian starts AND an impulse sqrt(w) eta at every node, against
    Sigma_K of the recursion with + diag(w): every entry of the sample landing covariance within six standard errors
    (cov_reference.mc_check's bound).  Without the impulses the same flights miss it: the check sees the w term."""
    from oracle import dynamics as od
    from successiveconvexification_amd.montecarlo import handover_factor, mc_draws
    p, par, x, u, s, d, L, S0, w, covK = w_case()
    N = W_SAMPLES
    xi0, eta = mc_draws(N, p.K, W_SEED, noise=True)
    dx0 = xi0 @ handover_factor(S0).T
    imp = eta * np.sqrt(w)
    _, xf, _, _ = mr.fly_plan(od, p, x[0], u[0], s[0], L[0], dx0, 10, 0, imp, par)
    e = xf[:, -1] - x[0, -1]
    _, _, xcov = mr.reduce(np.zeros((N, 16)), e, 0, 0, p.K)
    worst, over = mr.se_check(xcov, covK[:14, :14], N)
    print("C oracle, plan 0, S = %d, seed %d: worst entry of the landing covariance %.2f standard errors, %d entries over 6"
          % (N, W_SEED, worst, over))
    assert over == 0, (worst, over)
    _, xf0, _, _ = mr.fly_plan(od, p, x[0], u[0], s[0], L[0], dx0, 10, 0, None, par)
    e0 = xf0[:, -1] - x[0, -1]
    worst0, over0 = mr.se_check(mr.reduce(np.zeros((N, 16)), e0, 0, 0, p.K)[2], covK[:14, :14], N)
    print("the same starts without impulses against the same Sigma_K: worst %.2f standard errors, %d entries over 6" % (worst0, over0))
    assert over0 > 0
