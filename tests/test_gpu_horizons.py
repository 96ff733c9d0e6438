"""The analysis calls on the MI355X at horizons other than the sample problem's K = 50: K = 1, 2, 3 (the kernels' prefetch of "the next
node" runs once or never, the first and the last trip of their node loops coincide or touch) and K = 100 (config 5), and the batch-level
calls at K = 64 and 100, where the node-strided loop of the back-off kernel takes a second lap.  The calls: the flight check, the LQR
gains, the closed-loop flight (on the state and on an estimate), the covariance and navigation analyses and their per-node sigma.

The cases are those of tests/horizon_cases.py (B = 3), the tiles the device's own linearize_batch, the gains the REFERENCE's, fed to
both sides.  No tolerance here is new: every comparison goes through the helper of the module that pins the call at K = 50
(test_gpu_flight._compare, test_gpu_track._check_gains / _closed_loop_parity, test_gpu_cov._check_parity, test_gpu_nav._check_parity /
_zero_nav_equals_cov, test_gpu_nav_margins._check_psig) with that module's rule -- 16 x the float64-versus-longdouble distance of
the reference of that very case, floored at K n 2^-52 max|.|; the margin floor 8 * 2^-52 * terms / s; K * 1e-12 * A -- all computed
from the reference, never from the device.  Every comparison prints its figures before it asserts.

Truncation on the device (the identities test_horizons_cpu.py finds exact on the reference): a recursion sees only the tiles it has
passed, so the K-horizon call contains the 1-horizon call on a slice of its tiles and gains.  Asserted within the parity bound of the
shorter case and -- they were bitwise equal on the first run on an MI355X, every model, horizon, weight set and m -- bit for bit.
"""
import ctypes as C
from dataclasses import replace

import numpy as np
import pytest

import cov_reference as cr
import flight_reference as fr
import horizon_cases as hc
import margin_reference as mr
import nav_margin_reference as nm
import nav_reference as nr
import path_margin_reference as pr
import test_gpu_cov as tgc
import test_gpu_nav as tgn
import track_reference as tr
from test_gpu_flight import _compare
from test_gpu_nav_margins import _check_psig
from test_gpu_track import WEIGHTS, _check_gains, _closed_loop_parity, _gain_bounds

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
# the two flight kernels: both models at nsub 1 and 4, and the torque model once per K (its reference is driven substep by substep in
# Python: one substep per segment at K = 100 keeps that case to seconds)
FLIGHT_CASES = ([(m, K, n) for m in hc.MODELS for K in hc.HORIZONS for n in (1, 4)]
                + [(hc.FLIGHT_ONLY_MODEL, K, 1 if K == hc.LONG else 4) for K in hc.HORIZONS])
NOISE = np.random.default_rng(5).uniform(0.0, 1e-8, 14)
_SETUP = {}
_ANG = {"compared": 0, "left_out": 0}


def _setup(model, K, aero_tables):
    """(pp, po, dyn, par, x, u, sigma, the device's tiles d [B][K][14+2nu+1][14], the reference's gains at the default weights)"""
    key = (model, K)
    if key not in _SETUP:
        from successiveconvexification_amd.dynamics import IntegratorCache, linearize_batch
        pp, po, dyn, par, x, u, s = hc.case(model, K, aero_tables, device=True)
        c = IntegratorCache(pp, npts=10)
        _, d = linearize_batch(c, x, u, s, 1.0 / (K + 1))
        c.close()
        assert np.isfinite(d).all()
        _SETUP[key] = (pp, po, dyn, par, x, u, s, d, tr.gains(d, K)[0])
    return _SETUP[key]


def _rows(B):
    return [slice(b, b + 1) for b in range(B)]


def _count_angles(fn, *a):
    """run a parity helper of test_gpu_cov / test_gpu_nav and keep this module's own tally of the ELL_ANG values it left out"""
    tally = tgc._ANG if fn is tgc._check_parity else tgn._ANG
    before = dict(tally)
    fn(*a)
    for k in _ANG:
        _ANG[k] += tally[k] - before[k]


@pytest.mark.parametrize("K", hc.HORIZONS)
@pytest.mark.parametrize("model", hc.MODELS)
def test_gains(model, K, aero_tables, monkeypatch):
    from successiveconvexification_amd.dynamics import IntegratorCache, track_gains_batch
    pp, po, dyn, par, x, u, s, d, _ = _setup(model, K, aero_tables)
    c = IntegratorCache(pp, npts=10)
    for w in WEIGHTS:
        got = {}
        for mfma in ("0", "1"):
            monkeypatch.setenv("SCVX_TRACK_MFMA", mfma)
            L, P0 = track_gains_batch(c, d, *w, cost=True)
            assert L.shape == (hc.B, K, c.nu, 14 + c.nu) and P0.shape == (hc.B, 14 + c.nu, 14 + c.nu)
            _check_gains("%s K = %d, SCVX_TRACK_MFMA=%s" % (model, K, mfma), d, K, w, L, P0)
            assert np.array_equal(track_gains_batch(c, d, *w), L)       # without the cost output: the same gains
            for r in _rows(hc.B):                                      # every row is what a launch of its own gives
                L1, P1 = track_gains_batch(c, d[r], *w, cost=True)
                assert np.array_equal(L1, L[r]) and np.array_equal(P1, P0[r]), (mfma, r)
            got[mfma] = (L, P0)
        assert np.array_equal(got["0"][0], got["1"][0]) and np.array_equal(got["0"][1], got["1"][1])   # the two forms: bit for bit
    c.close()


@pytest.mark.parametrize("model,K,nsub", FLIGHT_CASES)
def test_flight_check(model, K, nsub, aero_tables):
    from successiveconvexification_amd.dynamics import IntegratorCache, flight_check_batch, propagate_batch
    pp, po, dyn, par, x, u, s, d, _ = _setup(model, K, aero_tables)
    c = IntegratorCache(pp, npts=nsub)                                   # PLAN and scvx_propagate_f64 take the context's nsub
    tag = "%s K = %d nsub %d" % (model, K, nsub)
    plan = flight_check_batch(c, x, u, s, mode="plan", dense=True)
    xn = propagate_batch(c, x, u, s, 1.0 / (K + 1))
    k2 = float(np.abs(plan.xfly[:, 1:] - xn).max())
    ref, xref = fr.fly(dyn, po, x, u, s, nsub, fr.PLAN, par)
    dp = float(np.abs(plan.xfly - xref).max())
    print("%s PLAN: xfly vs scvx_propagate_f64 %.3e (bound 1e-13), bitwise %s; vs the reference %.3e (bound 1e-12)"
          % (tag, k2, np.array_equal(plan.xfly[:, 1:], xn), dp))
    assert plan.xfly.shape == (hc.B, K + 1, 14) and np.array_equal(plan.xfly[:, 0], x[:, 0])
    assert k2 <= 1e-13 and dp <= 1e-12
    _compare(tag + " PLAN", plan.raw, ref, 1e-12, po)
    shoot = flight_check_batch(c, x, u, s, nsub=nsub, mode="shoot", dense=True)
    ref, xref = fr.fly(dyn, po, x, u, s, nsub, fr.SHOOT, par)
    A = fr.sensitivity(dyn, po, x, u, s, nsub, 1e-9, par=par)
    bound = K * 1e-12 * A
    dx = float(np.abs(shoot.xfly - xref).max())
    print("%s SHOOT: A %.3f, bound %.3e, device's largest state difference %.3e" % (tag, A, bound, dx))
    assert np.array_equal(shoot.xfly[:, 0], x[:, 0])
    assert dx <= bound
    _compare(tag + " SHOOT", shoot.raw, ref, bound, po)
    for mode, rep in (("plan", plan), ("shoot", shoot)):
        assert np.array_equal(flight_check_batch(c, x, u, s, nsub=nsub, mode=mode).raw, rep.raw, equal_nan=True)   # without the dense output
        for r in _rows(hc.B):
            own = flight_check_batch(c, x[r], u[r], s[r], nsub=nsub, mode=mode, dense=True)
            assert np.array_equal(own.raw, rep.raw[r], equal_nan=True) and np.array_equal(own.xfly, rep.xfly[r]), (mode, r)
    c.close()


@pytest.mark.parametrize("model,K,nsub", FLIGHT_CASES)
def test_closed_loop_flight(model, K, nsub, aero_tables):
    from successiveconvexification_amd.dynamics import IntegratorCache, flight_check_batch, track_fly_batch
    from successiveconvexification_amd.montecarlo import disperse_handover
    pp, po, dyn, par, x, u, s, d, L = _setup(model, K, aero_tables)
    c = IntegratorCache(pp, npts=10)
    tag = "%s K = %d" % (model, K)
    dx0 = disperse_handover(x[:, 0], 0, hc.B, 20261016, frac_r=1e-3, frac_v=1e-3, rate=1e-3)
    for clamp in (False, True):
        dev, _ = _closed_loop_parity(tag, c, po, dyn, par, x, u, s, L, dx0, nsub, clamp)
        # nav = zeros is the call without nav, bit for bit
        zero = track_fly_batch(c, x, u, s, L, dx0, nsub=nsub, clamp=clamp, dense=True, nav=np.zeros((hc.B, K, 14)))
        assert np.array_equal(zero.raw, dev.raw, equal_nan=True) and np.array_equal(zero.xfly, dev.xfly) and np.array_equal(zero.ufly, dev.ufly)
        assert np.array_equal(track_fly_batch(c, x, u, s, L, dx0, nsub=nsub, clamp=clamp).raw, dev.raw, equal_nan=True)
        for r in _rows(hc.B):
            own = track_fly_batch(c, x[r], u[r], s[r], L[r], dx0[r], nsub=nsub, clamp=clamp, dense=True)
            assert np.array_equal(own.raw, dev.raw[r], equal_nan=True) and np.array_equal(own.xfly, dev.xfly[r]), (clamp, r)
            assert np.array_equal(own.ufly, dev.ufly[r]), (clamp, r)
    # all-zero gains: the SHOOT flight check, bit for bit
    t = track_fly_batch(c, x, u, s, np.zeros_like(L), nsub=nsub, dense=True)
    sh = flight_check_batch(c, x, u, s, nsub=nsub, mode="shoot", dense=True)
    print("%s nsub %d zero gains vs SHOOT: report bitwise %s, xfly bitwise %s, largest difference %.3e"
          % (tag, nsub, np.array_equal(t.raw, sh.raw, equal_nan=True), np.array_equal(t.xfly, sh.xfly), np.abs(t.xfly - sh.xfly).max()))
    assert t.mode == "track" and np.array_equal(t.ufly, u)
    assert np.array_equal(t.xfly, sh.xfly) and np.array_equal(t.raw, sh.raw, equal_nan=True)
    # a non-zero nav [B][K][14] against the oracle closed loop fed the same estimate
    nav = 1e-3 * np.abs(x[:, :1]) * np.random.default_rng(3).uniform(-1.0, 1.0, (hc.B, K, 14))
    dev = track_fly_batch(c, x, u, s, L, dx0, nsub=nsub, dense=True, nav=nav)
    xref, uref = nr.chain(dyn, par, po, x, u, s, L, dx0, nav, nsub)
    A = tr.sensitivity(dyn, po, x, u, s, L, dx0, nsub, 1e-9, 0, par=par)
    bound = K * 1e-12 * A
    bu = bound * max(1.0, float(np.abs(L).max()))
    dxs, dus = float(np.abs(dev.xfly - xref).max()), float(np.abs(dev.ufly - uref).max())
    plain = track_fly_batch(c, x, u, s, L, dx0, nsub=nsub, dense=True)
    print("%s nsub %d on an estimate: A_cl %.3f, bound %.3e, xfly %.3e, ufly %.3e (bound %.3e); the estimate moves the flight by %.3e"
          % (tag, nsub, A, bound, dxs, dus, bu, np.abs(dev.xfly - plain.xfly).max()))
    assert np.array_equal(dev.xfly[:, 0], x[:, 0] + dx0) and np.array_equal(dev.ufly[:, 0], u[:, 0])
    assert dxs <= bound and dus <= bu
    assert np.abs(dev.xfly - plain.xfly).max() > 1e3 * bound      # nothing cancels: the injected error is what is compared
    for r in _rows(hc.B):
        own = track_fly_batch(c, x[r], u[r], s[r], L[r], dx0[r], nsub=nsub, dense=True, nav=nav[r])
        assert np.array_equal(own.raw, dev.raw[r], equal_nan=True) and np.array_equal(own.xfly, dev.xfly[r]) and np.array_equal(own.ufly, dev.ufly[r])
    c.close()


def _s0(x):
    return np.stack([cr.handover_s0(x[b, 0])[0] for b in range(x.shape[0])])


@pytest.mark.parametrize("mfma", ["0", "1"])
@pytest.mark.parametrize("K", hc.HORIZONS)
@pytest.mark.parametrize("model", hc.MODELS)
def test_covariance(model, K, mfma, aero_tables, monkeypatch):
    from successiveconvexification_amd.dynamics import IntegratorCache, cov_path_sigma_batch, cov_propagate_batch
    monkeypatch.setenv("SCVX_COV_MFMA", mfma)
    pp, po, dyn, par, x, u, s, d, _ = _setup(model, K, aero_tables)
    c = IntegratorCache(pp, npts=10)
    n = 14 + c.nu
    S0 = _s0(x)
    for w in WEIGHTS[:2]:
        for nz in (None, NOISE):
            ref = tgc._reference(("horizons", model, K, w, nz is None), po, x, u, d, K, w, S0, nz)
            L = ref[0]
            dev = cov_propagate_batch(c, x, u, d, L, S0, nz, dense=True)
            assert dev.cov.shape == (hc.B, K + 1, n, n) and dev.sig.shape == (hc.B, K + 1, n) and dev.covK.shape == (hc.B, n, n)
            tag = "%s K = %d, weights %s, w %s, SCVX_COV_MFMA=%s" % (model, K, w, "0" if nz is None else "> 0", mfma)
            _count_angles(tgc._check_parity, tag, K, dev, ref)
            lean = cov_propagate_batch(c, x, u, d, L, S0, nz)                # without the dense outputs: the same report
            assert np.array_equal(lean.raw, dev.raw, equal_nan=True) and lean.sig is None and lean.cov is None
            # the per-node sigma of the same launch, by the rule of test_path_sigma_against_the_longdouble_reference
            rep, psig = cov_path_sigma_batch(c, x, u, d, L, S0, nz)
            p64, pld = mr.path_sigma(po, x, u, ref[2]), mr.path_sigma(po, x, u, ref[5], np.longdouble)
            _check_psig(tag, po, K, n, psig, p64, pld)                        # ... which also asserts that row 0 is exactly zero
            assert np.array_equal(rep.raw, dev.raw, equal_nan=True)
            for r in _rows(hc.B):
                own = cov_propagate_batch(c, x[r], u[r], d[r], L[r], S0[r], nz, dense=True)
                assert np.array_equal(own.raw, dev.raw[r], equal_nan=True) and np.array_equal(own.cov, dev.cov[r]), r
                assert np.array_equal(own.sig, dev.sig[r]) and np.array_equal(own.covK, dev.covK[r]), r
                assert np.array_equal(cov_path_sigma_batch(c, x[r], u[r], d[r], L[r], S0[r], nz)[1], psig[r]), r
    c.close()


@pytest.mark.parametrize("m", [0, 6, 14])
@pytest.mark.parametrize("K", hc.HORIZONS)
@pytest.mark.parametrize("model", hc.MODELS)
def test_navigation(model, K, m, aero_tables):
    from successiveconvexification_amd.dynamics import IntegratorCache, nav_cov_batch, nav_path_sigma_batch
    pp, po, dyn, par, x, u, s, d, L = _setup(model, K, aero_tables)
    c = IntegratorCache(pp, npts=10)
    N = 28 + c.nu
    S0 = _s0(x)
    N0 = 0.25 * S0
    H, rm = tgn._model(m, x[0, 0])
    tag = "%s K = %d, m = %d" % (model, K, m)
    ref = tgn._reference(("horizons", model, K, m), po, x, u, d, K, L, S0, N0, H, rm)
    dev = nav_cov_batch(c, x, u, d, L, S0, N0, H, rm, dense=True)
    assert dev.joint.shape == (hc.B, K + 1, N, N) and dev.kf.shape == (hc.B, K, 14, m) and dev.navsig.shape == (hc.B, K + 1, 14)
    assert dev.sig.shape == (hc.B, K + 1, N - 14)
    _count_angles(tgn._check_parity, tag, K, dev, ref)
    lean = nav_cov_batch(c, x, u, d, L, S0, N0, H, rm)
    assert np.array_equal(lean.raw, dev.raw, equal_nan=True) and np.array_equal(lean.navraw, dev.navraw, equal_nan=True) and lean.joint is None
    # the per-node sigma of the navigation launch, by the rule of test_gpu_nav_margins.py
    rep, psig = nav_path_sigma_batch(c, x, u, d, L, S0, N0, H, rm)
    _check_psig(tag, po, K, N, psig, nm.path_sigma(po, x, u, d, K, L, S0, N0, H, rm),
                nm.path_sigma(po, x, u, d, K, L, S0, N0, H, rm, dtype=np.longdouble))
    assert np.array_equal(rep.raw, dev.raw, equal_nan=True) and np.array_equal(rep.navraw, dev.navraw, equal_nan=True)
    for r in _rows(hc.B):
        own = nav_cov_batch(c, x[r], u[r], d[r], L[r], S0[r], N0[r], H, rm, dense=True)
        for nm_ in ("raw", "navraw", "sig", "navsig", "kf", "joint"):
            assert np.array_equal(getattr(own, nm_), getattr(dev, nm_)[r], equal_nan=True), (nm_, r)
        assert np.array_equal(nav_path_sigma_batch(c, x[r], u[r], d[r], L[r], S0[r], N0[r], H, rm)[1], psig[r]), r
    c.close()


@pytest.mark.parametrize("K", hc.HORIZONS)
@pytest.mark.parametrize("model", hc.MODELS)
def test_zero_navigation_error_equals_the_covariance_call(model, K, aero_tables):
    from successiveconvexification_amd.dynamics import IntegratorCache
    pp, po, dyn, par, x, u, s, d, _ = _setup(model, K, aero_tables)
    c = IntegratorCache(pp, npts=10)
    tgn._zero_nav_equals_cov("%s K = %d" % (model, K), c, po, x, u, d)
    c.close()


def test_angle_exclusions_stay_below_a_tenth():
    """runs after the parity tests of this module: the ELL_ANG values they left out"""
    print("ELL_ANG compared %d, left out %d" % (_ANG["compared"], _ANG["left_out"]))
    assert _ANG["compared"] > 0
    assert _ANG["left_out"] <= 0.1 * (_ANG["compared"] + _ANG["left_out"])


@pytest.mark.parametrize("K", [2, 3, hc.LONG])
@pytest.mark.parametrize("model", hc.MODELS)
def test_truncation_on_the_device(model, K, aero_tables):
    """contexts of the two horizons, fed slices of the same tiles and gains"""
    from successiveconvexification_amd.dynamics import IntegratorCache, cov_propagate_batch, nav_cov_batch, track_gains_batch
    pp, po, dyn, par, x, u, s, d, L = _setup(model, K, aero_tables)
    cK, c1 = IntegratorCache(pp, npts=10), IntegratorCache(replace(pp, K=1), npts=10)
    p1 = replace(po, K=1)
    n = 14 + cK.nu
    tag = "%s K = %d -> 1" % (model, K)
    # gains: the last tile alone
    dl = np.ascontiguousarray(d[:, K - 1:])
    for w in WEIGHTS:
        long_, short = track_gains_batch(cK, d, *w)[:, K - 1:], track_gains_batch(c1, dl, *w)
        bL = _gain_bounds(dl, 1, w)[2]
        e = float(np.abs(long_ - short).max())
        print("%s gains, weights %s: %.3e (bound %.3e), bitwise %s" % (tag, w, e, bL, np.array_equal(long_, short)))
        assert e <= bL and np.array_equal(long_, short)
    # covariance and navigation: the first tile alone
    x2, u2 = np.ascontiguousarray(x[:, :2]), np.ascontiguousarray(u[:, :2])
    d0, L0 = np.ascontiguousarray(d[:, :1]), np.ascontiguousarray(L[:, :1])
    S0 = _s0(x)
    N0 = 0.25 * S0
    c64, cld = cr.propagate(d0, 1, L0, S0), cr.propagate(d0, 1, L0, S0, None, np.longdouble)
    bound = max(16.0 * float(np.abs(c64 - cld).max()), 1 * n * EPS * float(np.abs(cld).max()))
    long_, short = cov_propagate_batch(cK, x, u, d, L, S0, dense=("cov",)).cov[:, :2], cov_propagate_batch(c1, x2, u2, d0, L0, S0, dense=("cov",)).cov
    e = float(np.abs(long_ - short).max())
    print("%s covariance: %.3e (bound %.3e), bitwise %s" % (tag, e, bound, np.array_equal(long_, short)))
    assert e <= bound and np.array_equal(long_, short)
    for m in (0, 6):
        H, rm = tgn._model(m, x[0, 0])
        r64, rld = nr.propagate(d0, 1, L0, S0, N0, H, rm), nr.propagate(d0, 1, L0, S0, N0, H, rm, None, np.longdouble)
        cond = float(rld[2].max())
        long_ = nav_cov_batch(cK, x, u, d, L, S0, N0, H, rm, dense=("joint", "kf"))
        short = nav_cov_batch(c1, x2, u2, d0, L0, S0, N0, H, rm, dense=("joint", "kf"))
        for name, a, b_, f64, fld in (("joint", long_.joint[:, :2], short.joint, r64[0], rld[0]), ("kf", long_.kf[:, :1], short.kf, r64[1], rld[1])):
            if fld.size == 0:
                assert a.size == 0 and b_.size == 0
                continue
            bnd = max(16.0 * float(np.abs(f64 - fld).max()), 1 * (n + 14) * EPS * float(np.abs(fld).max()) * cond)
            e = float(np.abs(a - b_).max())
            print("%s navigation m = %d %s: %.3e (bound %.3e), bitwise %s" % (tag, m, name, e, bnd, np.array_equal(a, b_)))
            assert e <= bnd and np.array_equal(a, b_)
    cK.close(), c1.close()


def test_a_horizon_other_than_the_contexts_is_refused_at_k1(aero_tables):
    """K = 2 arrays on a K = 1 context: every call refuses them with its "K must equal" message and writes nothing"""
    from successiveconvexification_amd.dynamics import IntegratorCache, _p
    pp, po, dyn, par, x, u, s, d, gain = _setup("exo", 2, aero_tables)          # arrays of the horizon that is passed: nothing could overrun
    c = IntegratorCache(replace(pp, K=1), npts=10)
    L, h, B, K = c._L, c.handle, hc.B, 2
    S0 = np.ascontiguousarray(_s0(x))
    N0 = np.ascontiguousarray(0.25 * S0)
    H, rm = tgn._model(6, x[0, 0])
    H, rm = np.ascontiguousarray(H), np.ascontiguousarray(rm)
    q, r, qf = np.ones(14), np.ones(3), np.full(14, 100.0)
    nav = np.zeros((B, K, 14))
    out = {k: np.full(shape, 7.0) for k, shape in (("rep", (B, 16)), ("navrep", (B, 8)), ("xfly", (B, K + 1, 14)), ("ufly", (B, K + 1, 3)),
                                                    ("gain", (B, K, 3, 17)), ("p0", (B, 17, 17)), ("sig", (B, K + 1, 17)), ("covK", (B, 17, 17)),
                                                    ("cov", (B, K + 1, 17, 17)), ("psig", (B, K + 1, 5)), ("navsig", (B, K + 1, 14)),
                                                    ("kf", (B, K, 14, 6)), ("joint", (B, K + 1, 31, 31)))}
    o = lambda k: _p(out[k])   # noqa: E731
    gn = np.ascontiguousarray(gain)
    calls = [("scvx_flight_check_f64_host", [_p(x), _p(u), _p(s), 4, 0, o("rep"), o("xfly")]),
             ("scvx_track_gains_f64_host", [_p(d), _p(q), _p(r), _p(qf), o("gain"), o("p0")]),
             ("scvx_track_fly_f64_host", [_p(x), _p(u), _p(s), _p(gn), None, 4, 0, o("rep"), o("xfly"), o("ufly")]),
             ("scvx_track_fly_nav_f64_host", [_p(x), _p(u), _p(s), _p(gn), None, _p(nav), 4, 0, o("rep"), o("xfly"), o("ufly")]),
             ("scvx_cov_propagate_f64_host", [_p(x), _p(u), _p(d), _p(gn), _p(S0), None, o("rep"), o("sig"), o("covK"), o("cov")]),
             ("scvx_cov_path_sigma_f64_host", [_p(x), _p(u), _p(d), _p(gn), _p(S0), None, o("rep"), o("psig")]),
             ("scvx_nav_cov_f64_host", [_p(x), _p(u), _p(d), _p(gn), _p(S0), _p(N0), 6, _p(H), _p(rm), None, o("rep"), o("navrep"), o("sig"),
                                        o("navsig"), o("kf"), o("joint")]),
             ("scvx_nav_path_sigma_f64_host", [_p(x), _p(u), _p(d), _p(gn), _p(S0), _p(N0), 6, _p(H), _p(rm), None, o("rep"), o("navrep"),
                                               o("psig")])]
    for name, a in calls:
        assert getattr(L, name)(h, B, K, *a) == -1, name
        assert "K must equal" in L.scvx_last_error(h).decode(), (name, L.scvx_last_error(h))
    dev = C.c_void_p(1)                                                   # the device forms: the check comes before any pointer is used
    assert L.scvx_flight_check_f64(h, B, K, dev, dev, dev, 4, 0, dev, None) == -1 and "K must equal" in L.scvx_last_error(h).decode()
    assert L.scvx_track_gains_f64(h, B, K, dev, _p(q), _p(r), _p(qf), dev, None) == -1 and "K must equal" in L.scvx_last_error(h).decode()
    assert L.scvx_cov_propagate_f64(h, B, K, dev, dev, dev, dev, dev, None, dev, None, None, None) == -1 and "K must equal" in L.scvx_last_error(h).decode()
    for k, v in out.items():
        assert np.all(v == 7.0), k                                        # nothing ran
    # the context still works at its own horizon
    from successiveconvexification_amd.dynamics import flight_check_batch
    assert np.isfinite(flight_check_batch(c, x[:, :2], u[:, :2], s).GAP).all()
    c.close()


# ---- batch-level calls where the node loop of the back-off kernel takes a second lap: K + 1 = 65 and 101 --------------------------
@pytest.mark.parametrize("K", [64, hc.LONG])
def test_batch_level_calls_are_the_one_shot_calls_on_the_batchs_own_tiles(K):
    from successiveconvexification_amd.dynamics import (cov_path_sigma_batch, cov_propagate_batch, flight_check_batch, nav_cov_batch,
                                                          nav_path_sigma_batch, track_fly_batch, track_gains_batch)
    from successiveconvexification_amd.montecarlo import disperse_handover
    c, b = hc.flyable_batch(K)
    state = lambda: (b.trajectory_record(),) + b.scalars() + b.flags() + b.linearization()   # noqa: E731
    before = state()
    x, u, s = b.trajectory()
    d = b.linearization()[1]
    S0 = np.stack([cr.handover_s0(x[i, 0], 0, 1e-3)[0] for i in range(2)])
    N0 = 0.25 * S0
    H, rm = tgn._model(6, x[0, 0])
    w = (1.0, 1e-2, 1e4)
    for wt in ((), w):
        L, P0 = b.track_gains(*wt, cost=True)
        Lh, Ph = track_gains_batch(c, d, *wt, cost=True)
        assert L.shape == (2, K, 3, 17) and np.array_equal(L, Lh) and np.array_equal(P0, Ph)
    L = b.track_gains()
    assert np.isfinite(L).all()
    assert np.array_equal(b.path_sigma(S0, NOISE), cov_path_sigma_batch(c, x, u, d, L, S0, NOISE)[1])
    assert np.array_equal(b.path_sigma(S0, NOISE, nav=(N0, H, rm)), nav_path_sigma_batch(c, x, u, d, L, S0, N0, H, rm, NOISE)[1])
    assert np.array_equal(b.margins_from_cov(S0, ("thrust",), w=NOISE), cov_path_sigma_batch(c, x, u, d, L, S0, NOISE)[1])    # the device-side psig
    assert np.array_equal(b.margins_from_nav(S0, N0, H, rm, ("thrust",), w=NOISE), nav_path_sigma_batch(c, x, u, d, L, S0, N0, H, rm, NOISE)[1])
    b.set_thrust_margins(None, None)
    rb, rh = b.covariance(S0, NOISE, dense=True), cov_propagate_batch(c, x, u, d, L, S0, NOISE, dense=True)
    for nm_ in ("raw", "sig", "covK", "cov"):
        assert np.array_equal(getattr(rb, nm_), getattr(rh, nm_), equal_nan=True), nm_
    assert rb.cov.shape == (2, K + 1, 17, 17) and np.isfinite(rb.cov).all()
    nb, nh = b.navigation(S0, N0, H, rm, NOISE, dense=True), nav_cov_batch(c, x, u, d, L, S0, N0, H, rm, NOISE, dense=True)
    for nm_ in ("raw", "navraw", "sig", "navsig", "kf", "joint"):
        assert np.array_equal(getattr(nb, nm_), getattr(nh, nm_), equal_nan=True), nm_
    assert nb.kf.shape == (2, K, 14, 6) and np.isfinite(nb.joint).all()
    dx0 = disperse_handover(x[:, 0], 0, 2, 5, frac_r=1e-3, frac_v=1e-3, rate=1e-3)
    navv = 1e-4 * np.random.default_rng(8).uniform(-1.0, 1.0, (2, K, 14))
    for clamp in (False, True):
        for nv in (None, navv):
            fb = b.track(dx0, nsub=4, clamp=clamp, dense=True, nav=nv)
            fh = track_fly_batch(c, x, u, s, L, dx0, nsub=4, clamp=clamp, dense=True, nav=nv)
            assert np.array_equal(fb.raw, fh.raw, equal_nan=True) and np.array_equal(fb.xfly, fh.xfly) and np.array_equal(fb.ufly, fh.ufly)
    for mode in ("shoot", "plan"):
        fb, fh = b.flight_check(nsub=4, mode=mode, dense=True), flight_check_batch(c, x, u, s, nsub=4, mode=mode, dense=True)
        assert np.array_equal(fb.raw, fh.raw, equal_nan=True) and np.array_equal(fb.xfly, fh.xfly)
    for a0, a1 in zip(before, state()):
        assert np.array_equal(a0, a1, equal_nan=True)
    b.close(), c.close()


def test_one_round_of_robustify_on_every_constraint_at_k100():
    """No reference of a K = 100 replan exists, so neither convergence nor a sigma level is asserted: the statuses, the contract of
    include/scvx.h on what comes back, and the node feasibility of the replanned trajectories against the cones they were given"""
    from test_gpu_flight import _flyable
    K = hc.LONG
    c, b = hc.flyable_batch(K)
    po = replace(_flyable()[1], K=K)
    x0 = b.trajectory()[0]
    S0 = np.stack([cr.handover_s0(x0[i, 0], 0, 1e-3)[0] for i in range(2)])
    st, it, nu, dj, lo, hi = b.robustify(S0, nsigma=3, rounds=1, constraints="all")
    pm = b.path_margins()
    x, u, s = b.trajectory()
    tggs, sqcm = pr.consts(po)
    band = po.Tmax - po.Tmin
    print("K = 100 robustify(all): status %s in %s steps, |nu| %s; back-offs up to: thrust %s, mass %s, glide %s, tilt %s, rate %s"
          % (st, it, nu, lo.max(axis=1), *(pm[..., i].max(axis=1) for i in range(4))))
    assert np.isin(st, (0, 1, 2)).all(), st
    # the contract: finite, >= 0, below their widths, the forced zeros in place
    assert lo.shape == (2, K + 1) and np.array_equal(lo, hi) and np.isfinite(lo).all() and (lo >= 0).all() and (lo <= 0.25 * band).all()
    assert np.isfinite(pm).all() and (pm >= 0).all()
    for t in range(2):
        pr.check_contract(po, pm[t])
    assert not pm[:, K, [pr.GLIDE, pr.TILT, pr.RATE]].any() and not pm[:, 0, [pr.MASS, pr.GLIDE, pr.RATE]].any() and not lo[:, 0].any()
    assert (pm[:, 1:K, pr.TILT] > 0).all() and (lo[:, 1:] > 0).all()      # ... and something was asked for: S0 > 0 reaches every later node
    # node feasibility at the nodes 1..K-1: the audit's tilt and thrust functions are at most minus the back-off plus 1e-7
    g_tilt = np.linalg.norm(x[:, 1:K, 9:11], axis=-1) - sqcm
    tn = np.linalg.norm(u[:, 1:K, :3], axis=-1)
    print("   largest g + back-off at the nodes 1..K-1: tilt %.3e, Tmax %.3e, Tmin %.3e"
          % ((g_tilt + pm[:, 1:K, pr.TILT]).max(), (tn - po.Tmax + hi[:, 1:K]).max(), (po.Tmin - tn + lo[:, 1:K]).max()))
    assert (g_tilt <= -pm[:, 1:K, pr.TILT] + 1e-7).all()
    # ... and the audit kernel's own G_TILT over those nodes (test_gpu_path_margins._audit_shows_the_headroom: mode "plan", a time scale
    # that keeps every sample on its node, node 0 replaced by node 1) is that function
    from successiveconvexification_amd.dynamics import flight_check_batch
    xs, us = x.copy(), u.copy()
    xs[:, 0], us[:, 0] = xs[:, 1], us[:, 1]
    nodes = flight_check_batch(c, xs, us, np.full(2, 1e-9), mode="plan")
    print("   G_TILT of the audit at the nodes 1..K-1: %s (formed here: %s)" % (nodes.G_TILT, g_tilt.max(axis=1)))
    assert np.abs(nodes.G_TILT - g_tilt.max(axis=1)).max() < 1e-8
    assert (tn - po.Tmax <= -hi[:, 1:K] + 1e-7).all() and (po.Tmin - tn <= -lo[:, 1:K] + 1e-7).all()
    b.close(), c.close()
