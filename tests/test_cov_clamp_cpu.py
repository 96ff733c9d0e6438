"""Clamp-aware covariance analysis without a GPU: the independent reference (tests/cov_clamp_reference.py: the recursion of
include/scvx.h "CLAMP-AWARE covariance analysis" in numpy with the full F, G, N, Mtilde) against quadrature of the clamp, against the
plain recursion where nobody reaches the band, and -- the anchor -- against 2,048 clamped flights of the C oracle per case; the three
bindings (header, _lib.SIGNATURES, julia/ScvxAMD.jl) against each other; dynamics.SatCovReport and montecarlo.clamp_summary.

Data: the two plans the oracle converges on (tests/golden/oracle_flight_runs.npz), tiles from oracle.dynamics.linearize
(test_cov_cpu._data)."""
import os
import re

import numpy as np
import pytest

import cov_clamp_reference as sl
import cov_reference as cr
import mc_reference as mr
import track_reference as tr
from conftest import ROOT
from test_cov_cpu import _data


def _quad(Tlo, Thi, That, s):
    """(E[sat(t)], E[sat(t) (t - That)] / s^2) for t ~ N(That, s^2) by quadrature at 30 digits, the three pieces of sat apart"""
    import mpmath as mp
    with mp.workdps(30):
        Tlo, Thi, That, s = (mp.mpf(float(v)) for v in (Tlo, Thi, That, s))
        pdf = lambda t: mp.exp(-((t - That) / s) ** 2 / 2) / (s * mp.sqrt(2 * mp.pi))   # noqa: E731
        sat = lambda t: min(max(t, Tlo), Thi)   # noqa: E731
        lo, hi = That - 40 * s, That + 40 * s
        pts = sorted({lo, hi} | {p for p in (Tlo, Thi, That) if lo < p < hi})
        E = mp.quad(lambda t: sat(t) * pdf(t), pts)
        gam = mp.quad(lambda t: sat(t) * (t - That) * pdf(t), pts) / (s * s)
        return float(E), float(gam)


def test_mean_and_gain_of_the_clamp_against_quadrature():
    """E and gamma of steps 4 and 5 for (That, s) inside, on and outside the band: 1e-12 of the band's scale"""
    Tlo, Thi = 0.3, 0.9
    worst = 0.0
    for That in (0.05, 0.29, 0.3, 0.31, 0.6, 0.89, 0.9, 0.92, 1.4):
        for s in (1e-3, 0.02, 0.3, 2.0):
            plo, phi, gam, E = sl.sat_scalars(That, s, Tlo, Thi)
            Eq, gq = _quad(Tlo, Thi, That, s)
            worst = max(worst, abs(E - Eq), abs(gam - gq))
            assert abs(E - Eq) <= 1e-12 and abs(gam - gq) <= 1e-12, (That, s, E, Eq, gam, gq)
            assert gam == 1.0 - plo - phi and -1e-15 <= gam <= 1.0 and Tlo - 1e-15 <= E <= Thi + 1e-15
    print("E and gamma against quadrature over 36 points: worst difference %.2e" % worst)
    # the longdouble form (mpmath's erfc and exp) agrees with the float64 form to float64 rounding
    for That, s in ((0.29, 0.02), (0.6, 0.3), (0.92, 1e-3)):
        f, g = sl.sat_scalars(That, s, Tlo, Thi), sl.sat_scalars(That, s, Tlo, Thi, np.longdouble)
        assert all(abs(float(a) - float(b)) <= 1e-14 for a, b in zip(f, g)), (f, g)
    # Thi = +inf is allowed: its term is dropped where nobody reaches it, and E is the mean of max(t, Tlo)
    plo, phi, gam, E = sl.sat_scalars(0.31, 0.02, Tlo, np.inf)
    assert phi == 0.0 and np.isfinite(E) and abs(E - _quad(Tlo, 1e6, 0.31, 0.02)[0]) <= 1e-12
    # Tlo == 0 is no lower clamp: whatever mass the Gaussian puts below 0, P_lo is 0 and the band (0, inf) leaves t alone
    assert sl.sat_scalars(0.31, 0.3, 0.0, np.inf) == (0.0, 0.0, 1.0, 0.31)
    plo, phi, gam, E = sl.sat_scalars(0.31, 0.3, 0.0, Thi)
    assert plo == 0.0 and abs(E - _quad(-1e6, Thi, 0.31, 0.3)[0]) <= 1e-12


def test_the_special_cases_of_the_contract():
    Tlo, Thi = 0.3, 0.9
    # s == 0: the indicator forms
    assert sl.sat_scalars(0.5, 0.0, Tlo, Thi) == (0.0, 0.0, 1.0, 0.5)
    assert sl.sat_scalars(0.3, 0.0, Tlo, Thi) == (0.0, 0.0, 1.0, 0.3) and sl.sat_scalars(0.9, 0.0, Tlo, Thi) == (0.0, 0.0, 1.0, 0.9)
    assert sl.sat_scalars(0.2, 0.0, Tlo, Thi) == (1.0, 0.0, 0.0, 0.3) and sl.sat_scalars(1.2, 0.0, Tlo, Thi) == (0.0, 1.0, 0.0, 0.9)
    # That == 0: the flight's clamp leaves a zero thrust alone
    assert sl.sat_scalars(0.0, 0.1, Tlo, Thi) == (0.0, 0.0, 1.0, 0.0) and sl.sat_scalars(0.0, 0.0, Tlo, Thi) == (0.0, 0.0, 1.0, 0.0)
    un = np.zeros((1, 3))
    assert not tr.clamp_control(_data()[0], un).any()
    # a zero mean command in the recursion (node 1: mu_0 = 0, so chat is the plan's control itself): unsaturated, whatever the band
    p, par, x, u, s, d = _data()
    L, _ = tr.gains(d, p.K)
    S0 = cr.handover_s0(x[0, 0])[0]
    u0 = u[:1].copy()
    u0[0, 1] = 0.0
    out = sl.propagate(u0, d[:1], p.K, L[:1], S0[None], (p.Tmin, p.Tmax))
    assert tuple(out["satk"][0, 0]) == (0.0, 0.0, 0.0, 0.0) and out["gamma"][0, 0] == 1.0
    # a NaN stays in its own trajectory
    dn = d.copy().reshape(2, p.K, -1, 14)
    dn[1, 20, 3, 2] = np.nan
    S2 = np.stack([cr.handover_s0(x[b, 0])[0] for b in range(2)])
    good, bad = sl.propagate(u, d, p.K, L, S2, (p.Tmin, p.Tmax)), sl.propagate(u, dn, p.K, L, S2, (p.Tmin, p.Tmax))
    good["satrep"], bad["satrep"] = sl.satrep(good), sl.satrep(bad)
    assert np.isnan(bad["satrep"][1]).all() and np.isfinite(good["satrep"]).all()
    for k in ("satrep", "mean", "cov", "satk"):
        assert np.array_equal(bad[k][0], good[k][0]), k


def test_a_band_nobody_reaches_reproduces_the_plain_recursion_exactly():
    p, par, x, u, s, d = _data()
    L, _ = tr.gains(d, p.K)
    S0 = np.stack([cr.handover_s0(x[b, 0])[0] for b in range(2)])
    w = np.random.default_rng(5).uniform(0.0, 1e-8, 14)
    for noise in (None, w):
        out = sl.propagate(u, d, p.K, L, S0, (0.0, np.inf), noise)
        assert np.array_equal(out["cov"], cr.propagate(d, p.K, L, S0, noise))
        assert not out["mean"].any() and not out["satk"][:, :, 2:].any() and np.all(out["gamma"] == 1.0)
    rep = sl.satrep(out)
    assert not rep[:, sl.IDX["BIAS_M"]:sl.IDX["BIAS_W"] + 1].any() and not rep[:, sl.IDX["BIAS_PEAK"]].any()
    assert np.all(rep[:, sl.IDX["GAIN_MIN"]] == 1.0) and not rep[:, sl.IDX["P_LO"]].any() and not rep[:, sl.IDX["P_HI"]].any()
    assert np.array_equal(rep[:, sl.IDX["RMS_R"]], rep[:, sl.IDX["SIG_R"]])
    full = sl.run(p, x, u, d, p.K, L, S0, (0.0, np.inf), w)
    assert np.array_equal(full["report"], cr.run(p, x, u, d, p.K, L, S0, w)[0])


def test_no_dispersion_on_a_plan_inside_the_band_stays_zero():
    """S0 = 0, w = 0, the plan's thrust moved 1 % inside the band: s == 0 at every node, nothing saturates, Sigma and mu stay 0"""
    p, par, x, u, s, d = _data()
    L, _ = tr.gains(d, p.K)
    t = np.linalg.norm(u[:, :, :3], axis=2)
    width = p.Tmax - p.Tmin
    u_in = u.copy()
    u_in[:, :, :3] *= (np.clip(t, p.Tmin + 0.01 * width, p.Tmax - 0.01 * width) / t)[:, :, None]
    out = sl.propagate(u_in, d, p.K, L, np.zeros((2, 14, 14)), (p.Tmin, p.Tmax))
    assert not out["cov"].any() and not out["mean"].any() and not out["satk"][:, :, 1:].any()
    # the plan as it is rides Tmin to rounding: a node a hair below the band has a bias even without dispersion
    print("the plan's own |u| - Tmin: min %.3e" % (t - p.Tmin).min())


def test_header_binding_and_julia_carry_the_same_symbols():
    from successiveconvexification_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "scvx.h")).read()
    jl = open(os.path.join(ROOT, "julia", "ScvxAMD.jl")).read()
    nargs = {"scvx_cov_clamp_f64": 17, "scvx_cov_clamp_f64_host": 17, "scvx_batch_cov_clamp": 14}
    for sym, n in nargs.items():
        m = re.search(r"\bint %s\(([^;]*?)\);" % sym, hdr, flags=re.S)
        assert m, sym
        assert len(m.group(1).split(",")) == n, sym
        assert len(_lib.SIGNATURES[sym][1]) == n, sym
        j = re.search(r"ccall\(\(:%s, LIB\), Cint,\s*\(([^)]*)\)" % sym, jl, flags=re.S)
        assert j, sym
        assert len([a for a in j.group(1).split(",") if a.strip()]) == n, sym
    mac = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define SCVX_SAT_([A-Z_]+) (\d+)", hdr)}
    assert mac.pop("NREP") == 16 == _lib.SAT_NREP == sl.NREP
    assert mac == _lib.SAT_INDEX == sl.IDX and _lib.SAT_COLUMNS == sl.COLUMNS
    for name, i in _lib.SAT_INDEX.items():
        assert int(re.search(r"const SAT_%s = (\d+)" % name, jl).group(1)) == i
    assert int(re.search(r"#define SCVX_ABI_VERSION (\d+)", hdr).group(1)) == 4 == _lib.ABI_VERSION
    # outside install!(): that function's body is pinned to the reference's by test_abi_harness.py
    assert jl.index("function cov_clamp(b::Batch") < jl.index("function install!")
    assert "cov_clamp" not in jl[jl.index("function install!"):]


def test_sat_cov_report_clamp_summary_and_the_argument_helpers():
    from successiveconvexification_amd import _lib
    from successiveconvexification_amd._calls import CLAMP_DENSE, dense_names
    from successiveconvexification_amd.dynamics import CovReport, SatCovReport, _cov_band
    from successiveconvexification_amd.montecarlo import clamp_summary
    raw, sat = np.arange(5 * 16, dtype=float).reshape(5, 16), 100.0 + np.arange(5 * 16, dtype=float).reshape(5, 16)
    r = SatCovReport(raw, sat, mean=np.zeros((5, 4, 17)))
    assert isinstance(r, CovReport) and len(r) == 5 and r.satk is None and r.mean.shape == (5, 4, 17)
    for n, i in _lib.COV_INDEX.items():
        assert np.array_equal(getattr(r, n), raw[:, i])
    for n, i in _lib.SAT_INDEX.items():
        if not n.startswith("SIG_"):
            assert np.array_equal(getattr(r, n), sat[:, i])
    status = np.array([0, 0, 3, 0, 1])
    sm = clamp_summary(r, status)
    assert sm["n"] == 5 and sm["converged"] == 3 and sm["counts"]["solver"] == 1 and sum(sm["counts"].values()) == 5
    col = sat[[0, 1, 3], _lib.SAT_INDEX["P_LO"]]
    assert sm["stats"]["P_LO"] == {"min": col.min(), "median": float(np.median(col)), "p99": float(np.percentile(col, 99)), "max": col.max()}
    assert set(sm["stats"]) == set(_lib.SAT_COLUMNS) and clamp_summary(sat, status) == sm
    assert clamp_summary(sat, np.ones(5, int))["stats"]["RMS_R"] is None
    with pytest.raises(ValueError):
        clamp_summary(sat, status[:4])
    assert _cov_band(None) is None and _cov_band((0.0, np.inf)).tolist() == [0.0, np.inf] and _cov_band((0.3, 0.3)).tolist() == [0.3, 0.3]
    for bad in ((-0.1, 1.0), (np.inf, np.inf), (0.5, 0.4), (0.1, np.nan), (np.nan, 1.0), (0.1, 0.2, 0.3)):
        with pytest.raises(ValueError):
            _cov_band(bad)
    assert dense_names(True, CLAMP_DENSE) == {"mean", "sig", "covK", "cov", "satk"} and dense_names("satk", CLAMP_DENSE) == {"satk"}
    with pytest.raises(ValueError):
        dense_names(["sens"], CLAMP_DENSE)


def test_anchor_against_sampled_clamped_flights_of_the_oracle():
    """THE ANCHOR.  Both golden plans, the handover factor scaled by 0.1, 0.3 and 1; 2,048 clamped flights of the C oracle per case
    (mc_reference.fly_plan, nsub = 10, the starts mc_draws(2048, K, 7) through handover_factor(S0)) against the statistical
    linearisation (SL) and the plain recursion (LIN), track_reference.gains at default weights.  Four conditions per case: the trace of
    the r and of the v block of the landing covariance, SL / sampled, within [1/6, 6], and LIN / sampled of the v block below 1/6;
    the cosine of the SL landing bias with the sampled mean of x_fly[K] - xbar[K] (14-vectors) >= 0.9; their norm ratio within
    [1/3, 3]; P_LO / OUT_LO and P_HI / OUT_HI within [0.8, 2]."""
    from oracle import dynamics as od
    from successiveconvexification_amd.montecarlo import handover_factor, mc_draws
    p, par, x, u, s, d = _data()
    L, _ = tr.gains(d, p.K)
    xi0, _ = mc_draws(2048, p.K, 7, noise=False)
    for b in range(2):
        for scale in (0.1, 0.3, 1.0):
            S0 = cr.handover_s0(x[b, 0], scale=scale)[0]
            dx0 = xi0 @ handover_factor(S0).T
            _, xf, _, cmd = mr.fly_plan(od, p, x[b], u[b], s[b], L[b], dx0, 10, tr.CLAMP, par=par)
            e = xf[:, -1] - x[b, -1]
            n_lo, n_hi = mr.out_counts(cmd, p.Tmin, p.Tmax)
            out = sl.run(p, x[b:b + 1], u[b:b + 1], d[b:b + 1], p.K, L[b:b + 1], S0[None])
            lin = cr.propagate(d[b:b + 1], p.K, L[b:b + 1], S0[None])[0, -1]
            f = sl.anchor_figures(out["covK"][0][:14, :14], out["mean"][0, -1, :14], out["satrep"][0, sl.IDX["P_LO"]],
                                  out["satrep"][0, sl.IDX["P_HI"]], lin[:14, :14], e.mean(axis=0), np.cov(e.T), n_lo / cmd.size,
                                  n_hi / cmd.size)
            sl.anchor_assert("plan %d scale %.1f" % (b, scale), f)
