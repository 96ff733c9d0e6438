"""The CPU references of the analysis family (track_reference, cov_reference, nav_reference, margin_reference, flight_reference) at the
horizons of tests/horizon_cases.py -- K = 1, 2, 3 and 100 -- on tiles from oracle.dynamics.linearize: they run, stay finite, and obey
the truncation identities that test_gpu_horizons.py then asks of the device.  No GPU.

A recursion sees only the tiles it has passed.  On the reference these identities hold EXACTLY (np.array_equal, every K and model):
  * gains: the backward recursion over the last tile alone gives the last gain of the K-horizon recursion (both start from qf);
  * covariance: the forward recursion over the first tile alone gives the first two nodes of the K-horizon covariance;
  * navigation: the same for the joint and for the filter gain of node 0 -- the stored node k is the joint BEFORE the update at k, so
    "no measurement at node K" never touches a stored node.
The float64-to-longdouble distances printed here are the e_ref of the device's bounds (16 e_ref, floored) at the same horizons.
"""
import numpy as np
import pytest

import cov_reference as cr
import flight_reference as fr
import horizon_cases as hc
import margin_reference as mr
import nav_reference as nr
import track_reference as tr
from test_gpu_nav import _model

WEIGHTS = (1.0, 1e-2, 1e4)
NPTS = 4
_TILES = {}


def _setup(model, K, aero_tables):
    """the case with its oracle tiles, reference gains, S0 and N0"""
    key = (model, K)
    if key not in _TILES:
        from oracle import dynamics as od
        pp, po, dyn, par, x, u, s = hc.case(model, K, aero_tables)
        _, d = od.linearize(par, x, u, s, 1.0 / (K + 1), NPTS)
        S0 = np.stack([cr.handover_s0(x[b, 0])[0] for b in range(x.shape[0])])
        _TILES[key] = (po, dyn, par, x, u, s, d, tr.gains(d, K)[0], S0, 0.25 * S0)
    return _TILES[key]


def _dist(a, b):
    return float(np.abs(np.asarray(a, np.longdouble) - np.asarray(b, np.longdouble)).max()) if np.size(a) else 0.0


@pytest.mark.parametrize("K", hc.HORIZONS)
@pytest.mark.parametrize("model", hc.MODELS)
def test_references_run_and_are_finite(model, K, aero_tables):
    po, dyn, par, x, u, s, d, L, S0, N0 = _setup(model, K, aero_tables)
    nu = u.shape[-1]
    n = 14 + nu
    assert d.shape == (hc.B, K, 15 + 2 * nu, 14) and np.isfinite(d).all()
    # gains, float64 and longdouble
    for w in ((), WEIGHTS):
        L64, P64 = tr.gains(d, K, *w)
        Lld, Pld = tr.gains(d, K, *w, dtype=np.longdouble)
        assert L64.shape == (hc.B, K, nu, n) and np.isfinite(L64).all() and np.isfinite(P64).all()
        assert np.isfinite(Lld.astype(float)).all() and np.isfinite(Pld.astype(float)).all()
        print("%s K = %d weights %s: gains float64-vs-longdouble %.3e (max|L| %.4g), P0 %.3e" % (model, K, w or "default", _dist(L64, Lld),
                                                                                              np.abs(L64).max(), _dist(P64, Pld)))
    # covariance, report and path sigma
    rep, cov, sig = cr.run(po, x, u, d, K, L, S0)
    cld = cr.propagate(d, K, L, S0, None, np.longdouble)
    rld = cr.report(po, x, u, cld, np.longdouble)
    fin = [cr.IDX[c] for c in cr.COLUMNS if c not in cr.MARGINS]           # a margin may be +inf by definition (no node had one)
    assert cov.shape == (hc.B, K + 1, n, n) and np.isfinite(cov).all() and np.isfinite(sig).all()
    assert np.isfinite(rep[:, fin]).all() and not np.isnan(rep).any() and not np.isnan(rld.astype(float)).any()
    ps, psld = mr.path_sigma(po, x, u, cov), mr.path_sigma(po, x, u, cld, np.longdouble)
    assert ps.shape == (hc.B, K + 1, 5) and np.isfinite(ps).all() and not ps[:, 0].any() and (ps[:, 1:, 4] > 0).all()
    print("%s K = %d: covariance float64-vs-longdouble %.3e (max %.3e), path sigma %.3e (max %.3e)"
          % (model, K, _dist(cov, cld), np.abs(cov).max(), _dist(ps, psld), ps.max()))
    # the ELL_ANG comparisons the rule ELL_A - ELL_B > 1e-6 ELL_A leaves out
    ea, eb = rld[:, cr.IDX["ELL_A"]], rld[:, cr.IDX["ELL_B"]]
    out = int((~np.asarray(ea - eb > 1e-6 * ea)).sum())
    print("%s K = %d: ELL_ANG left out %d of %d" % (model, K, out, hc.B))
    assert out <= 0.1 * hc.B
    # navigation
    for m in (0, 6, 14):
        H, rm = _model(m, x[0, 0])
        r64 = nr.run(po, x, u, d, K, L, S0, N0, H, rm)
        r80 = nr.run(po, x, u, d, K, L, S0, N0, H, rm, None, np.longdouble)
        assert r64["joint"].shape == (hc.B, K + 1, n + 14, n + 14) and r64["kf"].shape == (hc.B, K, 14, m)
        for name in ("joint", "sig", "navsig", "kf", "navrep"):
            assert np.isfinite(r64[name]).all(), (m, name)
        assert np.isfinite(r64["report"][:, fin]).all() and not np.isnan(r64["report"]).any()
        print("%s K = %d m = %d: joint float64-vs-longdouble %.3e (max %.3e), kf %.3e, cond(S) %.3e"
              % (model, K, m, _dist(r64["joint"], r80["joint"]), np.abs(r64["joint"]).max(), _dist(r64["kf"], r80["kf"]), r64["cond"].max()))
    # the open-loop and the closed-loop flight
    for mode in (fr.PLAN, fr.SHOOT):
        rf, xf = fr.fly(dyn, po, x, u, s, NPTS, mode, par)
        assert xf.shape == (hc.B, K + 1, 14) and np.isfinite(xf).all() and not np.isnan(rf).any() and not np.isposinf(rf).any()
        assert np.array_equal(xf[:, 0], x[:, 0])
    dx0 = 1e-3 * np.abs(x[:, 0]) * np.random.default_rng(K).uniform(-1.0, 1.0, (hc.B, 14))
    for flags in (0, tr.CLAMP):
        rt, xt, ut, cmd = tr.fly(dyn, po, x, u, s, L, dx0, NPTS, flags, par)
        assert np.isfinite(xt).all() and np.isfinite(ut).all() and cmd.shape == (hc.B, K) and not np.isnan(rt).any()
        assert np.array_equal(xt[:, 0], x[:, 0] + dx0) and np.array_equal(ut[:, 0], u[:, 0])


@pytest.mark.parametrize("K", hc.HORIZONS)
@pytest.mark.parametrize("model", hc.MODELS)
def test_truncation_identities_hold_exactly_on_the_reference(model, K, aero_tables):
    po, dyn, par, x, u, s, d, L, S0, N0 = _setup(model, K, aero_tables)
    for dtype in (np.float64, np.longdouble):
        for w in ((), WEIGHTS):
            assert np.array_equal(tr.gains(d[:, K - 1:], 1, *w, dtype=dtype)[0], tr.gains(d, K, *w, dtype=dtype)[0][:, K - 1:])
        assert np.array_equal(cr.propagate(d[:, :1], 1, L[:, :1], S0, None, dtype), cr.propagate(d, K, L, S0, None, dtype)[:, :2])
        for m in (0, 6):
            H, rm = _model(m, x[0, 0])
            j1, k1, _ = nr.propagate(d[:, :1], 1, L[:, :1], S0, N0, H, rm, None, dtype)
            jK, kK, _ = nr.propagate(d, K, L, S0, N0, H, rm, None, dtype)
            assert np.array_equal(j1, jK[:, :2]) and np.array_equal(k1, kK[:, :1])
