"""Covariance analysis (scvx_cov_propagate_f64 / scvx_batch_cov) on the MI355X against the independent CPU reference
(tests/cov_reference.py: the recursion of include/scvx.h in numpy with the full F, G, M, float64 and longdouble) and against the
device's own closed-loop flight.

Bounds, none of them taken from the device:
  * parity (reference gains fed to both sides): with e_ref = the largest difference between the float64 and the longdouble reference
    of the case, the device must be within max(16 e_ref, K n 2^-52 max|Sigma|) of the longdouble reference -- the rule of
    test_gpu_track.py's _gain_bounds: one more decimal digit than numpy's own rounding on the same data for the device's other
    summation order and fma contraction, floored at the textbook forward error of K chained n-term dot products.  The same for sig,
    covK and, column by column, the report.  A margin N = -g / s adds the rounding of g itself, a small difference of terms of size
    t (|ubar| - Tmin is ~1e-9 on plans that sit on the bound): its floor is 8 * 2^-52 * t / s at the node that attains the minimum.
    ELL_ANG is compared only where ELL_A - ELL_B > 1e-6 ELL_A (a circular ellipse has no angle); at most 10 % may be left out.
  * device against device: the finite-difference window [13, 20] about (2 / 0.5)^2 = 16 and the six-standard-error bound of
    test_cov_cpu.py, with scvx_track_fly_f64 as the flyer and the device's own gains.
Every comparison prints its figures before it asserts.
"""
import os

import numpy as np
import pytest

import cov_reference as cr
import track_reference as tr
from conftest import GOLDEN
from test_gpu_flight import _case, _flyable, _problems  # noqa: F401

pytestmark = pytest.mark.gpu

MODELS = ["exo", "aero", "aero+fins", "aero+fins+torque"]
WEIGHTS = [(1.0, 1.0, 100.0), (1.0, 1e-2, 1e4), (10.0, 1.0, 1e6)]
EPS = 2.0 ** -52
_REF = {}
_ANG = {"compared": 0, "left_out": 0}


def _s0(x):
    return np.stack([cr.handover_s0(x[b, 0])[0] for b in range(x.shape[0])])


def _reference(key, po, x, u, d, K, w, S0, noise=None):
    """float64 and longdouble reference of a case under the REFERENCE's gains: (L, rep64, cov64, sig64, repld, covld, sigld, detail)"""
    if key not in _REF:
        L, _ = tr.gains(d, K, *w)
        r64, c64, s64 = cr.run(po, x, u, d, K, L, S0, noise)
        cld = cr.propagate(d, K, L, S0, noise, np.longdouble)
        rld, det = cr.report(po, x, u, cld, np.longdouble, detail=True)
        dg = np.diagonal(cld, axis1=-2, axis2=-1)
        sld = np.where(dg > 0, np.sqrt(np.where(dg > 0, dg, 0)), 0)
        _REF[key] = (L, r64, c64, s64, rld, cld, sld, det)
    return _REF[key]


def _check_parity(tag, K, dev, ref):
    L, r64, c64, s64, rld, cld, sld, det = ref
    n = c64.shape[-1]
    for name, got, f64, fld in (("cov", dev.cov, c64, cld), ("sig", dev.sig, s64, sld), ("covK", dev.covK, c64[:, -1], cld[:, -1])):
        e_ref = float(np.abs(f64 - fld).max())
        bound = max(16.0 * e_ref, K * n * EPS * float(np.abs(fld).max()))
        e = float(np.abs(got - fld).max())
        print("%s %s: device-vs-longdouble %.3e (float64 reference %.3e, bound %.3e), max %.3e" % (tag, name, e, e_ref, bound, np.abs(fld).max()))
        assert np.isfinite(got).all()
        assert e <= bound, (tag, name, e, bound)
    assert np.array_equal(dev.cov, np.swapaxes(dev.cov, -1, -2))          # symmetrised: each pair from both triangles
    assert np.array_equal(dev.cov[:, -1], dev.covK)
    for name in cr.COLUMNS:
        i = cr.IDX[name]
        g, f64, fld = dev.raw[:, i], r64[:, i], rld[:, i]
        inf = np.isposinf(fld.astype(np.float64))
        assert np.array_equal(inf, np.isposinf(g)), (tag, name, g, fld)
        keep = ~inf
        if name == "ELL_ANG":
            ea, eb = rld[:, cr.IDX["ELL_A"]], rld[:, cr.IDX["ELL_B"]]
            keep = keep & np.asarray(ea - eb > 1e-6 * ea)
            _ANG["compared"] += int(keep.sum())
            _ANG["left_out"] += int((~keep).sum())
        if not keep.any():
            continue
        e_ref = float(np.abs(f64 - fld)[keep].max())
        floor = np.full(g.shape[0], K * n * EPS * float(np.abs(fld[keep]).max()))
        if name in cr.MARGINS:
            m = cr.MARGINS.index(name)
            for b in range(g.shape[0]):
                if det[b][m] is not None:
                    _, terms, s = det[b][m]
                    floor[b] = max(floor[b], 8.0 * EPS * terms / s)
        bound = np.maximum(16.0 * e_ref, floor)
        e = np.abs(g - fld).astype(np.float64)
        print("%s %-8s: device-vs-longdouble %.3e (float64 reference %.3e, bound %.3e .. %.3e), values %.4g .. %.4g"
              % (tag, name, e[keep].max(), e_ref, bound[keep].min(), bound[keep].max(), float(fld[keep].min()), float(fld[keep].max())))
        assert np.all(e[keep] <= bound[keep]), (tag, name, e, bound)


@pytest.mark.parametrize("mfma", ["0", "1"])
@pytest.mark.parametrize("model", MODELS)
def test_parity_unconverged_plans(model, mfma, aero_tables, monkeypatch):
    """both forms of the kernel's n-deep products (SCVX_COV_MFMA, read at every launch), whichever is the default"""
    from successiveconvexification_amd.dynamics import IntegratorCache, cov_propagate_batch, linearize_batch
    monkeypatch.setenv("SCVX_COV_MFMA", mfma)
    pp, po, dyn, par, x, u, s = _case(model, aero_tables)
    c = IntegratorCache(pp, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (po.K + 1))
    S0 = _s0(x)
    for w in WEIGHTS:
        ref = _reference((model, w), po, x, u, d, po.K, w, S0)
        dev = cov_propagate_batch(c, x, u, d, ref[0], S0, dense=True)
        assert dev.cov.shape == (5, po.K + 1, 14 + c.nu, 14 + c.nu) and dev.sig.shape == (5, po.K + 1, 14 + c.nu)
        _check_parity("%s B = 5 unconverged, weights %s, SCVX_COV_MFMA=%s" % (model, w, mfma), po.K, dev, ref)
        lean = cov_propagate_batch(c, x, u, d, ref[0], S0)             # without the dense outputs: the same report
        assert np.array_equal(lean.raw, dev.raw) and lean.sig is None and lean.cov is None
        only = cov_propagate_batch(c, x, u, d, ref[0], S0, dense=("sig",))
        assert np.array_equal(only.sig, dev.sig) and only.covK is None
    c.close()


@pytest.mark.parametrize("mfma", ["0", "1"])
def test_parity_golden_plans_with_process_noise(mfma, monkeypatch):
    """the oracle's converged plans (they ride Tmin: the margins are small differences), with and without w"""
    from successiveconvexification_amd.dynamics import IntegratorCache, cov_propagate_batch, linearize_batch
    monkeypatch.setenv("SCVX_COV_MFMA", mfma)
    g = np.load(os.path.join(GOLDEN, "oracle_flight_runs.npz"))
    pp, po = _flyable()
    x, u, s = g["x"], g["u"], g["sigma"]
    c = IntegratorCache(pp, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (po.K + 1))
    S0 = _s0(x)
    noise = np.random.default_rng(5).uniform(0.0, 1e-8, 14)
    for w in WEIGHTS:
        for nz in (None, noise):
            ref = _reference(("golden", w, nz is None), po, x, u, d, po.K, w, S0, nz)
            dev = cov_propagate_batch(c, x, u, d, ref[0], S0, nz, dense=True)
            _check_parity("golden plans, weights %s, w %s, SCVX_COV_MFMA=%s" % (w, "0" if nz is None else "> 0", mfma), po.K, dev, ref)
    # what it shows: the closed loop shrinks the landing dispersion, and the plans have no thrust headroom
    L = ref[0]
    closed = cov_propagate_batch(c, x, u, d, tr.gains(d, po.K)[0], S0)
    opened = cov_propagate_batch(c, x, u, d, np.zeros_like(L), S0)
    print("SIG_R start %s closed %s open %s; S_THRUST %s N_TMIN %s" % (np.sqrt(np.trace(S0[:, 1:4, 1:4], axis1=1, axis2=2)), closed.SIG_R,
                                                                     opened.SIG_R, closed.S_THRUST, closed.N_TMIN))
    assert np.all(closed.SIG_R < opened.SIG_R) and np.all(np.isposinf(opened.N_TMIN)) and np.all(opened.S_THRUST == 0.0)
    c.close()


def test_angle_exclusions_stay_below_a_tenth():
    """runs after the parity tests of this module: the ELL_ANG values they left out"""
    print("ELL_ANG compared %d, left out %d" % (_ANG["compared"], _ANG["left_out"]))
    assert _ANG["compared"] > 0
    assert _ANG["left_out"] <= 0.1 * (_ANG["compared"] + _ANG["left_out"])


def test_device_recursion_against_the_device_closed_loop_finite_differences():
    """test_cov_cpu.py's second-order check with scvx_track_fly_f64 as the flyer and the device's own gains and covariance"""
    from successiveconvexification_amd.dynamics import IntegratorCache, cov_propagate_batch, linearize_batch, track_fly_batch, track_gains_batch
    g = np.load(os.path.join(GOLDEN, "oracle_flight_runs.npz"))
    pp, po = _flyable()
    x, u, s = g["x"], g["u"], g["sigma"]
    c = IntegratorCache(pp, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (po.K + 1))
    fly = lambda X, U, S, L, dx0: track_fly_batch(c, X, U, S, L, dx0, nsub=10, dense=True).xfly   # noqa: E731
    for wi, w in enumerate(WEIGHTS):
        L = track_gains_batch(c, d, *w)
        for b in range(2):
            S0, C = cr.handover_s0(x[b, 0])
            sl = slice(b, b + 1)
            cov = cov_propagate_batch(c, x[sl], u[sl], d[sl], L[sl], S0[None], dense=("cov",)).cov[0]
            err = cr.fd_errors(fly, x[sl], u[sl], s[sl], L[sl], cov, C, (2.0, 1.0, 0.5, 0.1))
            ratio = err[2.0] / err[0.5]
            print("device, weights %s plan %d: error at eps 2 / 1 / 0.5 / 0.1 = %.2e / %.2e / %.2e / %.2e, ratio(2 : 0.5) %.2f"
                  % (w, b, err[2.0], err[1.0], err[0.5], err[0.1], ratio))
            if wi < 2:
                assert 13.0 <= ratio <= 20.0, (w, b, ratio)
                assert err[0.5] < 1e-5, (w, b, err[0.5])
    c.close()


@pytest.mark.parametrize("b", [0, 1])
def test_device_monte_carlo_within_six_standard_errors(b):
    """N = 8,192 Gaussian starts in ONE scvx_track_fly_f64 launch against the device's covariance: every entry of every node"""
    from successiveconvexification_amd.dynamics import IntegratorCache, cov_propagate_batch, linearize_batch, track_fly_batch, track_gains_batch
    from successiveconvexification_amd.montecarlo import gaussian_handover
    g = np.load(os.path.join(GOLDEN, "oracle_flight_runs.npz"))
    pp, po = _flyable()
    x, u, s = g["x"], g["u"], g["sigma"]
    c = IntegratorCache(pp, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (po.K + 1))
    L = track_gains_batch(c, d)
    N = 8192
    sl = slice(b, b + 1)
    S0, _ = cr.handover_s0(x[b, 0], scale=0.1)
    dx0 = gaussian_handover(S0, 0, N, 11)
    r = track_fly_batch(c, cr.rep(x[sl], N), cr.rep(u[sl], N), cr.rep(s[sl], N), cr.rep(L[sl], N), dx0, nsub=10, dense=True)
    cov = cov_propagate_batch(c, x[sl], u[sl], d[sl], L[sl], S0[None], dense=("cov",)).cov[0]
    worst, worstK, over = cr.mc_check(r.xfly, r.ufly, x[b], u[b], cov)
    print("device, plan %d: worst entry %.2f standard errors (%.2f at node K), %d entries over 6" % (b, worst, worstK, over))
    assert over == 0, (worst, over)
    c.close()


def test_batch_level_covariance_and_the_batch_is_untouched():
    import bench
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache, cov_propagate_batch, linearize_batch
    pp, po = _flyable()
    B, K = 8, po.K
    ic = bench.disperse_ics(pp, 0, B, 7)
    c = IntegratorCache(pp, npts=10)
    b = ScvxBatch(c, B).init(ic)
    twin = ScvxBatch(c, B).init(ic)
    st, it, nu, dj = b.solve()
    twin.solve()
    assert np.all(st == 0), (st, it)
    before = (b.trajectory_record(),) + b.scalars() + b.flags() + b.linearization()
    x, u, s = b.trajectory()
    S0 = _s0(x)
    noise = np.full(14, 1e-9)
    _, d = linearize_batch(c, x, u, s, 1.0 / (K + 1))
    print("batch tiles vs a fresh linearisation of its iterate: bitwise %s" % np.array_equal(d.reshape(-1), before[-1].reshape(-1)))
    for w in (tr.DEFAULT_WEIGHTS, (1.0, 1e-2, 1e4)):
        rb = b.covariance(S0, noise, *w, dense=True)
        rh = cov_propagate_batch(c, x, u, d, b.track_gains(*w), S0, noise, dense=True)
        for a0, a1 in ((rb.raw, rh.raw), (rb.sig, rh.sig), (rb.covK, rh.covK), (rb.cov, rh.cov)):
            assert np.array_equal(a0, a1, equal_nan=True)
    lean = b.covariance(S0, noise)
    assert np.array_equal(lean.raw, b.covariance(S0, noise, dense=True).raw) and lean.sig is None
    assert np.array_equal(b.covariance(S0[0]).raw[0], b.covariance(S0).raw[0])          # one S0 for all
    sd = np.sqrt(np.diag(S0[0]))
    assert np.array_equal(b.covariance(sd).raw, b.covariance(np.diag(sd * sd)).raw)      # a vector of standard deviations
    print("batch: SIG_R %s S_THRUST %s N_TMIN %s" % (rb.SIG_R, rb.S_THRUST, rb.N_TMIN))
    after = (b.trajectory_record(),) + b.scalars() + b.flags() + b.linearization()
    for a0, a1 in zip(before, after):
        assert np.array_equal(a0, a1, equal_nan=True)
    # float tiles: widened on load; the same tiles, widened on the host, through the context-level call: bit for bit
    b.set_linearization_f32(True)
    d32 = b.linearization()[1]
    assert np.array_equal(d32, d32.astype(np.float32).astype(np.float64)) and not np.array_equal(d32.reshape(-1), d.reshape(-1))
    r32 = b.covariance(S0, noise, dense=True)
    h32 = cov_propagate_batch(c, x, u, d32, b.track_gains(), S0, noise, dense=True)
    for a0, a1 in ((r32.raw, h32.raw), (r32.sig, h32.sig), (r32.covK, h32.covK), (r32.cov, h32.cov)):
        assert np.array_equal(a0, a1, equal_nan=True)
    assert not np.array_equal(r32.raw, rb.raw)
    b.set_linearization_f32(False)
    assert np.array_equal(b.linearization()[1], before[-1])
    # a following solve_step equals, bit for bit, that of a twin batch never analysed
    r1, r2 = b.solve_step(), twin.solve_step()
    for a0, a1 in zip(r1 + (b.trajectory_record(),) + b.scalars(), r2 + (twin.trajectory_record(),) + twin.scalars()):
        assert np.array_equal(a0, a1, equal_nan=True)
    b.close(), twin.close(), c.close()


def test_at_size_rows_equal_a_launch_of_their_own():
    import bench
    from oracle import model as om
    from successiveconvexification_amd import montecarlo as mc, sample_problems as sp
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache, cov_propagate_batch
    pp, po = sp.base_prob_scaled, om.base_prob_scaled()
    B, K = 8192, pp.K
    c = IntegratorCache(pp, npts=10)
    b = ScvxBatch(c, B).init(bench.disperse_ics(pp, 0, B, 20261004))
    for _ in range(2):
        b.solve_step_async()
    status, _, _ = b.flags()
    x, u, s = b.trajectory()
    d = b.linearization()[1].reshape(B, K, -1, 14)
    sd = np.zeros(14)
    sd[1:] = 1e-3
    L = b.track_gains()
    big = b.covariance(sd, dense=("sig", "covK"))
    fine = np.isfinite(big.raw[:, :10]).all(axis=1)
    print("B = 8192: %d rows with a finite report" % fine.sum())
    assert fine.sum() >= 16
    rows = np.random.default_rng(20261016).choice(np.flatnonzero(fine), 16, replace=False)
    own = cov_propagate_batch(c, x[rows], u[rows], d[rows], L[rows], sd, dense=("sig", "covK"))
    assert np.array_equal(own.raw, big.raw[rows]) and np.array_equal(own.sig, big.sig[rows]) and np.array_equal(own.covK, big.covK[rows])
    ref = _reference(("at size",), po, x[rows], u[rows], d[rows], K, tr.DEFAULT_WEIGHTS, cr.s0_full(sd, 16))
    dev = cov_propagate_batch(c, x[rows], u[rows], d[rows], ref[0], sd, dense=True)
    _check_parity("B = 8192 rows %s" % rows.tolist(), K, dev, ref)
    summ = mc.dispersion_summary(big, status)
    assert sum(summ["counts"].values()) == B == summ["n"]
    b.close(), c.close()


def test_arguments_are_checked_and_a_nan_poisons_only_its_row():
    import ctypes as C
    from oracle import model as om
    from successiveconvexification_amd import _lib, sample_problems as sp
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache, _p, cov_propagate_batch, linearize_batch, track_gains_batch
    pp, po = sp.base_prob_scaled, om.base_prob_scaled()
    c = IntegratorCache(pp, npts=10)
    b = ScvxBatch(c, 5).init(om.disperse_ics(po, 5, 20261004))
    b.solve_step()
    x, u, s = b.trajectory()
    _, d = linearize_batch(c, x, u, s, 1.0 / (po.K + 1))
    gain = track_gains_batch(c, d)
    L, h, K = c._L, c.handle, pp.K
    S0 = np.ascontiguousarray(_s0(x))
    rep = np.full((5, 16), 7.0)
    err = lambda: L.scvx_last_error(h).decode()   # noqa: E731
    dev = lambda v: C.c_void_p(1) if v is not None else None   # noqa: E731  the checks come before any device pointer is used

    def bad_w(v):
        a = np.zeros(14)
        a[3] = v
        return a

    cases = [(dict(B=0), "B >= 1"), (dict(K=K - 1), "K must equal"), (dict(x=None), "null"), (dict(u=None), "null"), (dict(d=None), "null"),
             (dict(gain=None), "null"), (dict(S0=None), "null"), (dict(rep=None), "null"), (dict(w=bad_w(-1.0)), "w must be"),
             (dict(w=bad_w(np.nan)), "w must be"), (dict(w=bad_w(np.inf)), "w must be")]
    for kw, word in cases:
        v = dict(B=5, K=K, x=x, u=u, d=d, gain=gain, S0=S0, w=None, rep=rep)
        v.update(kw)
        pw = None if v["w"] is None else _p(np.ascontiguousarray(v["w"]))
        ptr = lambda n: None if v[n] is None else _p(v[n])   # noqa: E731
        a_host = [v["B"], v["K"], ptr("x"), ptr("u"), ptr("d"), ptr("gain"), ptr("S0"), pw, ptr("rep"), None, None, None]
        a_dev = [v["B"], v["K"]] + [dev(v[n]) for n in ("x", "u", "d", "gain", "S0")] + [pw, dev(v["rep"]), None, None, None]
        for fn, a in ((L.scvx_cov_propagate_f64_host, a_host), (L.scvx_cov_propagate_f64, a_dev)):
            assert fn(h, *a) == -1, (kw, fn)
            assert word in err(), (kw, err())
    assert np.all(rep == 7.0)                                    # nothing ran
    bh = b.handle
    q, r, qf = np.ones(14), np.ones(3), np.full(14, 100.0)
    assert L.scvx_batch_cov(bh, _p(q), _p(r), _p(qf), None, None, _p(rep), None, None, None) == -1 and "null" in err()
    assert L.scvx_batch_cov(bh, _p(q), _p(r), _p(qf), _p(S0), _p(bad_w(-1.0)), _p(rep), None, None, None) == -1 and "w must be" in err()
    assert L.scvx_batch_cov(bh, _p(q), _p(np.zeros(3)), _p(qf), _p(S0), None, _p(rep), None, None, None) == -1 and "r must be" in err()
    assert L.scvx_batch_cov(bh, None, _p(r), _p(qf), _p(S0), None, _p(rep), None, None, None) == -1 and "null" in err()
    assert np.all(rep == 7.0)
    with pytest.raises(_lib.ScvxError, match="w must be"):
        b.covariance(S0, w=-1.0)
    with pytest.raises(ValueError):
        b.covariance(S0[:4])
    with pytest.raises(ValueError):
        cov_propagate_batch(c, x, u, d, gain[:, :, :, :16], S0)
    with pytest.raises(ValueError):
        cov_propagate_batch(c, x, u, d[:, :, :20], gain, S0)
    # every output of the batch form may be left out; the batch form equals the context form on the batch's own gains
    assert L.scvx_batch_cov(bh, _p(q), _p(r), _p(qf), _p(S0), None, None, None, None, None) == 0
    good = cov_propagate_batch(c, x, u, d, gain, S0, dense=True)
    assert np.array_equal(b.covariance(S0).raw, cov_propagate_batch(c, x, u, d, b.track_gains(), S0).raw)
    # a NaN in one trajectory's tile (an Inf in another's gain, a NaN in a third's S0) poisons that row only
    dn, gn, sn = d.copy(), gain.copy(), S0.copy()
    dn.reshape(5, K, -1, 14)[1, 30, 2, 5] = np.nan
    gn[3, 12, 1, 4] = np.inf
    sn[4, 2, 2] = np.nan
    for mf in ("0", "1"):
        os.environ["SCVX_COV_MFMA"] = mf
        try:
            pois = cov_propagate_batch(c, x, u, dn, gn, sn, dense=True)
        finally:
            del os.environ["SCVX_COV_MFMA"]
        assert np.isnan(pois.raw[[1, 3, 4]]).all(), pois.raw[[1, 3, 4]]
        assert np.array_equal(pois.raw[[0, 2]], good.raw[[0, 2]]) and np.array_equal(pois.cov[[0, 2]], good.cov[[0, 2]])
        assert np.array_equal(pois.cov[1, :31], good.cov[1, :31]) and np.isnan(pois.cov[1, 31]).any()
    b.close(), c.close()


def test_rocketland_covariance_single_problem():
    from successiveconvexification_amd import rocketland as rl, sample_problems as sp
    from successiveconvexification_amd.dynamics import IntegratorCache
    p = sp.base_prob_scaled
    c = IntegratorCache(p, npts=10)
    ip = rl.create_initial(p, c)
    ip, _, _ = rl.solve_step(ip, c)
    sd = np.zeros(14)
    sd[1:7] = 1e-3
    r = rl.covariance(ip, c, sd, dense=True)
    assert len(r) == 1 and r.sig.shape == (1, p.K + 1, 17) and r.cov.shape == (1, p.K + 1, 17, 17) and np.isfinite(r.raw[:, :10]).all()
    rb = ip.model.covariance(sd, dense=True)
    assert np.array_equal(r.raw, rb.raw) and np.array_equal(r.cov, rb.cov)
    with pytest.raises(ValueError):
        rl.covariance(ip, c)
    c.close()
