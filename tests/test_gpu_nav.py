"""Navigation-error (LQG) covariance analysis and the closed loop flown on estimates (scvx_nav_cov_f64 / scvx_track_fly_nav_f64 /
scvx_batch_nav_cov / scvx_batch_track_fly_nav) on the MI355X against the independent CPU reference (tests/nav_reference.py: the
recursion of include/scvx.h in numpy with the full T, U and Xi, float64 and longdouble; the closed loop driven through the C oracle)
and against the device's own calls that it must contain.

Bounds, none of them taken from the device:
  * parity (reference gains fed to both sides): with e_ref = the largest difference between the float64 and the longdouble reference
    of the case, the device must be within max(16 e_ref, K N 2^-52 max|.| c) of the longdouble reference, N = 14 + nu + 14 and c the
    largest cond(S_k) of the case as the reference computes it -- the rule of test_gpu_cov.py with the joint's longer dot products
    and the conditioning of the solve with S.  For joint, sig, navsig, kf and, column by column, both reports; the N_* columns with
    test_gpu_cov._check_parity's floor 8 * 2^-52 * t / s; ELL_ANG only where ELL_A - ELL_B > 1e-6 ELL_A, at most 10 % left out.
  * N0 = 0: the z block and the report against cov_propagate_batch, to the same bound (c = 1: the filter gain is zero).
  * nav = zeros: scvx_track_fly_f64 bit for bit.  nav != 0: nav_reference's oracle closed loop within K * 1e-12 * A_cl, the rule of
    test_gpu_track.py.
  * sampled: 8,192 closed loops in one launch per plan against the device's joint: no entry over six standard errors.
Every comparison prints its figures before it asserts.
"""
import ctypes as C
import os

import numpy as np
import pytest

import cov_reference as cr
import nav_reference as nr
import track_reference as tr
from conftest import GOLDEN
from test_gpu_flight import _case, _compare, _flyable, _problems  # noqa: F401

pytestmark = pytest.mark.gpu

MODELS = ["exo", "aero", "aero+fins", "aero+fins+torque"]
EPS = 2.0 ** -52
_ANG = {"compared": 0, "left_out": 0}
_REF = {}


def _s0(x):
    return np.stack([cr.handover_s0(x[b, 0])[0] for b in range(x.shape[0])])


def _model(m, x0):
    """(H, rm) of the parity cases: m = 0 none; 1 the altitude; 6 position and velocity; 14 identity plus a fixed seeded perturbation.
    1 sigma: 3e-5 of the largest |r| / |v| component of x0 on r and v rows, 1e-4 on the others"""
    if m == 0:
        return None, None
    sd = np.full(14, 1e-4)
    sd[1:4], sd[4:7] = 3e-5 * np.abs(x0[1:4]).max(), 3e-5 * np.abs(x0[4:7]).max()
    if m == 1:
        return np.eye(14)[1:2], sd[1:2] ** 2
    if m == 6:
        return np.eye(14)[1:7], sd[1:7] ** 2
    assert m == 14
    return np.eye(14) + 0.1 * np.random.default_rng(14).standard_normal((14, 14)), sd ** 2


def _reference(key, po, x, u, d, K, L, S0, N0, H, rm, noise=None):
    """float64 and longdouble reference of a case: (run64, runld)"""
    if key not in _REF:
        _REF[key] = (nr.run(po, x, u, d, K, L, S0, N0, H, rm, noise), nr.run(po, x, u, d, K, L, S0, N0, H, rm, noise, np.longdouble, detail=True))
    return _REF[key]


def _check_parity(tag, K, dev, ref):
    r64, rld = ref
    N = rld["joint"].shape[-1]
    c = float(rld["cond"].max())
    for name, got in (("joint", dev.joint), ("sig", dev.sig), ("navsig", dev.navsig), ("kf", dev.kf)):
        f64, fld = r64[name], rld[name]
        if fld.size == 0:
            assert got.size == 0
            continue
        e_ref = float(np.abs(f64 - fld).max())
        bound = max(16.0 * e_ref, K * N * EPS * float(np.abs(fld).max()) * c)
        e = float(np.abs(got - fld).max())
        print("%s %s: device-vs-longdouble %.3e (float64 reference %.3e, bound %.3e), max %.3e, cond(S) %.3e"
              % (tag, name, e, e_ref, bound, np.abs(fld).max(), c))
        assert np.isfinite(got).all()
        assert e <= bound, (tag, name, e, bound)
    assert np.array_equal(dev.joint, np.swapaxes(dev.joint, -1, -2))          # symmetrised: each pair from both triangles
    det = rld["detail"]
    for rname, raw, cols, idx in (("report", dev.raw, cr.COLUMNS, cr.IDX), ("navrep", dev.navraw, nr.NAV_COLUMNS, nr.NAV_IDX)):
        for name in cols:
            i = idx[name]
            g, f64, fld = raw[:, i], r64[rname][:, i], rld[rname][:, i]
            inf = np.isposinf(fld.astype(np.float64))
            assert np.array_equal(inf, np.isposinf(g)), (tag, name, g, fld)
            keep = ~inf
            if name == "ELL_ANG":
                ea, eb = rld[rname][:, cr.IDX["ELL_A"]], rld[rname][:, cr.IDX["ELL_B"]]
                keep = keep & np.asarray(ea - eb > 1e-6 * ea)
                _ANG["compared"] += int(keep.sum())
                _ANG["left_out"] += int((~keep).sum())
            if not keep.any():
                continue
            e_ref = float(np.abs(f64 - fld)[keep].max())
            floor = np.full(g.shape[0], K * N * EPS * float(np.abs(fld[keep]).max()) * c)
            if name in cr.MARGINS:
                mi = cr.MARGINS.index(name)
                for b in range(g.shape[0]):
                    if det[b][mi] is not None:
                        _, terms, s = det[b][mi]
                        floor[b] = max(floor[b], 8.0 * EPS * terms / s)
            bound = np.maximum(16.0 * e_ref, floor)
            e = np.abs(g - fld).astype(np.float64)
            print("%s %-8s: device-vs-longdouble %.3e (float64 reference %.3e, bound %.3e .. %.3e), values %.4g .. %.4g"
                  % (tag, name, e[keep].max(), e_ref, bound[keep].min(), bound[keep].max(), float(fld[keep].min()), float(fld[keep].max())))
            assert np.all(e[keep] <= bound[keep]), (tag, name, e, bound)


@pytest.mark.parametrize("m", [0, 1, 6, 14])
@pytest.mark.parametrize("model", MODELS)
def test_parity_unconverged_plans(model, m, aero_tables):
    from successiveconvexification_amd.dynamics import IntegratorCache, linearize_batch, nav_cov_batch
    pp, po, dyn, par, x, u, s = _case(model, aero_tables)
    c = IntegratorCache(pp, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (po.K + 1))
    S0 = _s0(x)
    N0 = 0.25 * S0
    H, rm = _model(m, x[0, 0])
    L, _ = tr.gains(d, po.K)                                   # the REFERENCE's gains, fed to both sides
    ref = _reference((model, m), po, x, u, d, po.K, L, S0, N0, H, rm)
    dev = nav_cov_batch(c, x, u, d, L, S0, N0, H, rm, dense=True)
    N = 28 + c.nu
    assert dev.joint.shape == (5, po.K + 1, N, N) and dev.kf.shape == (5, po.K, 14, m) and dev.navsig.shape == (5, po.K + 1, 14)
    _check_parity("%s B = 5 unconverged, m = %d" % (model, m), po.K, dev, ref)
    c.close()


@pytest.mark.parametrize("m", [0, 1, 6, 14])
def test_parity_golden_plans_with_process_noise(m):
    """the oracle's converged plans (they ride Tmin: the margins are small differences), with the process noise of test_gpu_cov.py"""
    from successiveconvexification_amd.dynamics import IntegratorCache, linearize_batch, nav_cov_batch
    g = np.load(os.path.join(GOLDEN, "oracle_flight_runs.npz"))
    pp, po = _flyable()
    x, u, s = g["x"], g["u"], g["sigma"]
    c = IntegratorCache(pp, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (po.K + 1))
    S0 = _s0(x)
    N0 = 0.25 * S0
    H, rm = _model(m, x[0, 0])
    noise = np.random.default_rng(5).uniform(0.0, 1e-8, 14)
    L, _ = tr.gains(d, po.K)
    ref = _reference(("golden", m), po, x, u, d, po.K, L, S0, N0, H, rm, noise)
    dev = nav_cov_batch(c, x, u, d, L, S0, N0, H, rm, noise, dense=True)
    _check_parity("golden plans, m = %d, w > 0" % m, po.K, dev, ref)
    c.close()


def test_angle_exclusions_stay_below_a_tenth():
    """runs after the parity tests of this module: the ELL_ANG values they left out"""
    print("ELL_ANG compared %d, left out %d" % (_ANG["compared"], _ANG["left_out"]))
    assert _ANG["compared"] > 0
    assert _ANG["left_out"] <= 0.1 * (_ANG["compared"] + _ANG["left_out"])


def _zero_nav_equals_cov(model, c, po, x, u, d):
    """N0 = 0 on the device (the plans x, u with the tiles d on the context c): the z block and the report are cov_propagate_batch's,
    with and without a measurement model"""
    from successiveconvexification_amd.dynamics import cov_propagate_batch, nav_cov_batch
    K, n, B = po.K, 14 + c.nu, x.shape[0]
    S0 = _s0(x)
    L, _ = tr.gains(d, K)
    cov = cov_propagate_batch(c, x, u, d, L, S0, dense=True)
    c64, cld = cr.propagate(d, K, L, S0), cr.propagate(d, K, L, S0, dtype=np.longdouble)
    bound = max(16.0 * float(np.abs(c64 - cld).max()), K * (n + 14) * EPS * float(np.abs(cld).max()))
    rld, det = cr.report(po, x, u, cld, np.longdouble, detail=True)
    r64 = cr.report(po, x, u, c64)
    for m in (0, 6):
        H, rm = _model(m, x[0, 0])
        nav = nav_cov_batch(c, x, u, d, L, S0, np.zeros((14, 14)), H, rm, dense=True)
        e = float(np.abs(nav.joint[:, :, :n, :n] - cov.cov).max())
        print("%s m = %d: z block vs cov_propagate_batch %.3e (bound %.3e), bitwise %s; report bitwise %s"
              % (model, m, e, bound, np.array_equal(nav.joint[:, :, :n, :n], cov.cov), np.array_equal(nav.raw, cov.raw)))
        assert e <= bound
        assert not nav.joint[:, :, n:, :].any() and not nav.joint[:, :, :, n:].any() and not nav.kf.any()
        assert np.abs(nav.sig - cov.sig).max() <= bound and not nav.navsig.any() and not nav.navraw[:, :6].any()
        for name in cr.COLUMNS:
            i = cr.IDX[name]
            inf = np.isposinf(cov.raw[:, i])
            assert np.array_equal(inf, np.isposinf(nav.raw[:, i]))
            if name == "ELL_ANG" or inf.all():
                continue
            floor = np.full(B, K * (n + 14) * EPS * float(np.abs(rld[~inf, i]).max()))
            if name in cr.MARGINS:
                for b in range(B):
                    if det[b][cr.MARGINS.index(name)] is not None:
                        _, terms, sd = det[b][cr.MARGINS.index(name)]
                        floor[b] = max(floor[b], 8.0 * EPS * terms / sd)
            bnd = np.maximum(16.0 * float(np.abs(r64[:, i] - rld[:, i])[~inf].max()), floor)
            assert np.all(np.abs(nav.raw[:, i] - cov.raw[:, i])[~inf] <= bnd[~inf]), (name, nav.raw[:, i], cov.raw[:, i], bnd)


@pytest.mark.parametrize("model", ["exo", "aero+fins"])
def test_zero_navigation_error_equals_the_covariance_call(model, aero_tables):
    from successiveconvexification_amd.dynamics import IntegratorCache, linearize_batch
    pp, po, dyn, par, x, u, s = _case(model, aero_tables)
    c = IntegratorCache(pp, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (po.K + 1))
    _zero_nav_equals_cov(model, c, po, x, u, d)
    c.close()


@pytest.mark.parametrize("B", [1, 64, 65])
@pytest.mark.parametrize("model", ["exo", "aero+fins"])
def test_zero_nav_reproduces_the_flight_without_it_bit_for_bit(model, B, aero_tables):
    """the flyer is lane-per-trajectory: one lane, a full wavefront, a wavefront and a lane; nu = 3 and 5"""
    from successiveconvexification_amd.dynamics import IntegratorCache, linearize_batch, track_fly_batch
    from successiveconvexification_amd.montecarlo import disperse_handover
    pp, po, dyn, par, x, u, s = _case(model, aero_tables)
    c = IntegratorCache(pp, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (po.K + 1))
    L, _ = tr.gains(d, po.K)
    rows = np.arange(B) % 5
    X, U, S, G = x[rows], u[rows], s[rows], L[rows]
    dx0 = disperse_handover(X[:, 0], 0, B, 20261017, frac_r=1e-3, frac_v=1e-3, rate=1e-3)
    for clamp in (False, True):
        old = track_fly_batch(c, X, U, S, G, dx0, nsub=4, clamp=clamp, dense=True)
        new = track_fly_batch(c, X, U, S, G, dx0, nsub=4, clamp=clamp, dense=True, nav=np.zeros((B, po.K, 14)))
        assert np.array_equal(old.raw, new.raw, equal_nan=True) and np.array_equal(old.xfly, new.xfly) and np.array_equal(old.ufly, new.ufly)
    other = track_fly_batch(c, X, U, S, G, dx0, nsub=4, clamp=True, dense=True, nav=np.full((B, po.K, 14), 1e-4))
    assert not np.array_equal(other.ufly, old.ufly)
    assert np.array_equal(track_fly_batch(c, X, U, S, G, dx0, nsub=4, clamp=True, nav=np.full((B, po.K, 14), 1e-4)).raw, other.raw,
                          equal_nan=True)                            # without the dense outputs: the same report
    c.close()


@pytest.mark.parametrize("model", MODELS)
def test_flight_on_an_estimate_against_the_oracle_closed_loop(model, aero_tables):
    from successiveconvexification_amd.dynamics import IntegratorCache, linearize_batch, track_fly_batch
    from successiveconvexification_amd.montecarlo import disperse_handover
    pp, po, dyn, par, x, u, s = _case(model, aero_tables)
    c = IntegratorCache(pp, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (po.K + 1))
    L, _ = tr.gains(d, po.K)
    dx0 = disperse_handover(x[:, 0], 0, 5, 20261016, frac_r=1e-3, frac_v=1e-3, rate=1e-3)
    nav = 1e-3 * np.abs(x[:, :1]) * np.random.default_rng(3).uniform(-1.0, 1.0, (5, po.K, 14))
    dev = track_fly_batch(c, x, u, s, L, dx0, nsub=10, dense=True, nav=nav)
    xref, uref = nr.chain(dyn, par, po, x, u, s, L, dx0, nav, 10)
    A = tr.sensitivity(dyn, po, x, u, s, L, dx0, 10, 1e-9, 0, par=par)
    bound = po.K * 1e-12 * A
    bu = bound * max(1.0, float(np.abs(L).max()))
    dxs, dus = float(np.abs(dev.xfly - xref).max()), float(np.abs(dev.ufly - uref).max())
    plain = track_fly_batch(c, x, u, s, L, dx0, nsub=10, dense=True)
    print("%s: A_cl %.3f, bound %.3e, xfly %.3e, ufly %.3e (bound %.3e); the estimate moves the flight by %.3e"
          % (model, A, bound, dxs, dus, bu, np.abs(dev.xfly - plain.xfly).max()))
    assert np.array_equal(dev.xfly[:, 0], x[:, 0] + dx0) and np.array_equal(dev.ufly[:, 0], u[:, 0])
    assert dxs <= bound and dus <= bu
    assert np.abs(dev.xfly - plain.xfly).max() > 1e3 * bound      # nothing cancels: the injected error is what is compared
    c.close()


@pytest.mark.parametrize("b", [0, 1])
def test_device_monte_carlo_of_the_joint_within_six_standard_errors(b):
    """N = 8,192 closed loops flown on sampled estimates in ONE scvx_track_fly_nav_f64 launch, the filter gains and the joint
    covariance from the device: every entry of every node (inputs: test_nav_cpu.py's)"""
    from successiveconvexification_amd.dynamics import (IntegratorCache, cov_propagate_batch, linearize_batch, nav_cov_batch,
                                                          track_fly_batch, track_gains_batch)
    from successiveconvexification_amd.montecarlo import gaussian_handover, measurement_rows, nav_error_samples
    g = np.load(os.path.join(GOLDEN, "oracle_flight_runs.npz"))
    pp, po = _flyable()
    x, u, s = g["x"], g["u"], g["sigma"]
    c = IntegratorCache(pp, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (po.K + 1))
    L = track_gains_batch(c, d)
    N = 8192
    sl = slice(b, b + 1)
    S0, _ = cr.handover_s0(x[b, 0], scale=0.1)
    N0 = 0.25 * S0
    H = measurement_rows("rv")
    sd = np.repeat([3e-5 * np.abs(x[b, 0, 1:4]).max(), 3e-5 * np.abs(x[b, 0, 4:7]).max()], 3)
    rm = sd * sd
    an = nav_cov_batch(c, x[sl], u[sl], d[sl], L[sl], S0[None], N0[None], H, rm, dense=("kf", "joint"))
    base = cov_propagate_batch(c, x[sl], u[sl], d[sl], L[sl], S0[None])
    dx0 = gaussian_handover(S0, 0, N, 11)
    fed, before = nav_error_samples(d[b], an.kf[0], H, rm, N0, 0, N, 12)
    r = track_fly_batch(c, cr.rep(x[sl], N), cr.rep(u[sl], N), cr.rep(s[sl], N), cr.rep(L[sl], N), dx0, nsub=10, dense=True, nav=fed)
    worst, worstK, over = nr.mc_check(r.xfly, r.ufly, before, x[b], u[b], an.joint[0])
    print("device, plan %d: worst entry %.2f standard errors (%.2f at node K), %d entries over 6; landing position 1 sigma %.3g without, "
          "%.3g with the navigation term (NAV_R %.3g, EST_R %.3g)" % (b, worst, worstK, over, base.SIG_R[0], an.SIG_R[0], an.NAV_R[0], an.EST_R[0]))
    assert over == 0, (worst, over)
    assert an.SIG_R[0] > base.SIG_R[0]
    c.close()


def test_batch_level_calls_and_the_batch_is_untouched():
    import bench
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache, linearize_batch, nav_cov_batch, track_fly_batch
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
    N0 = 0.25 * S0
    H, rm = _model(6, x[0, 0])
    noise = np.full(14, 1e-9)
    _, d = linearize_batch(c, x, u, s, 1.0 / (K + 1))
    names = ("raw", "navraw", "sig", "navsig", "kf", "joint")
    for w in (tr.DEFAULT_WEIGHTS, (1.0, 1e-2, 1e4)):
        rb = b.navigation(S0, N0, H, rm, noise, *w, dense=True)
        rh = nav_cov_batch(c, x, u, d, b.track_gains(*w), S0, N0, H, rm, noise, dense=True)
        for nm in names:
            assert np.array_equal(getattr(rb, nm), getattr(rh, nm), equal_nan=True), nm
    lean = b.navigation(S0, N0, H, rm, noise)
    assert np.array_equal(lean.raw, b.navigation(S0, N0, H, rm, noise, dense=True).raw) and lean.joint is None and lean.kf is None
    assert np.array_equal(b.navigation(S0[0], N0[0], H, rm).navraw[0], b.navigation(S0, N0, H, rm).navraw[0])   # one S0 / N0 for all
    blind = b.navigation(S0, N0, None, None)
    print("batch: SIG_R %s NAV_R %s EST_R %s; inertial only: SIG_R %s NAV_R %s" % (rb.SIG_R, rb.NAV_R, rb.EST_R, blind.SIG_R, blind.NAV_R))
    assert np.all(rb.NAV_R < blind.NAV_R)
    nav = 1e-4 * np.random.default_rng(8).uniform(-1.0, 1.0, (B, K, 14))
    fb = b.track(nav=nav, dense=True)
    fh = track_fly_batch(c, x, u, s, b.track_gains(), dense=True, nav=nav)
    assert np.array_equal(fb.raw, fh.raw, equal_nan=True) and np.array_equal(fb.xfly, fh.xfly) and np.array_equal(fb.ufly, fh.ufly)
    assert np.array_equal(b.track(nav=np.zeros((B, K, 14)), dense=True).ufly, b.track(dense=True).ufly)
    after = (b.trajectory_record(),) + b.scalars() + b.flags() + b.linearization()
    for a0, a1 in zip(before, after):
        assert np.array_equal(a0, a1, equal_nan=True)
    # float tiles: widened on load; the same tiles, widened on the host, through the context-level call: bit for bit
    b.set_linearization_f32(True)
    d32 = b.linearization()[1]
    r32 = b.navigation(S0, N0, H, rm, noise, dense=True)
    h32 = nav_cov_batch(c, x, u, d32, b.track_gains(), S0, N0, H, rm, noise, dense=True)
    for nm in names:
        assert np.array_equal(getattr(r32, nm), getattr(h32, nm), equal_nan=True), nm
    assert not np.array_equal(r32.raw, rb.raw)
    b.set_linearization_f32(False)
    assert np.array_equal(b.linearization()[1], before[-1])
    # a following solve_step equals, bit for bit, that of a twin batch never analysed
    r1, r2 = b.solve_step(), twin.solve_step()
    for a0, a1 in zip(r1 + (b.trajectory_record(),) + b.scalars(), r2 + (twin.trajectory_record(),) + twin.scalars()):
        assert np.array_equal(a0, a1, equal_nan=True)
    b.close(), twin.close(), c.close()


def test_arguments_dense_outputs_and_nan_poisoning():
    from oracle import model as om
    from successiveconvexification_amd import _lib, sample_problems as sp
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache, _p, linearize_batch, nav_cov_batch, track_fly_batch, track_gains_batch
    pp, po = sp.base_prob_scaled, om.base_prob_scaled()
    c = IntegratorCache(pp, npts=10)
    b = ScvxBatch(c, 5).init(om.disperse_ics(po, 5, 20261004))
    b.solve_step()
    x, u, s = b.trajectory()
    _, d = linearize_batch(c, x, u, s, 1.0 / (po.K + 1))
    gain = track_gains_batch(c, d)
    L, h, K = c._L, c.handle, pp.K
    S0 = np.ascontiguousarray(_s0(x))
    N0 = np.ascontiguousarray(0.25 * S0)
    H, rm = _model(6, x[0, 0])
    H = np.ascontiguousarray(H)
    rep, navrep = np.full((5, 16), 7.0), np.full((5, 8), 7.0)
    err = lambda: L.scvx_last_error(h).decode()   # noqa: E731
    dev = lambda v: C.c_void_p(1) if v is not None else None   # noqa: E731  the checks come before any device pointer is used

    def bad(a, v):
        a = np.array(a, float)
        a.flat[2] = v
        return a

    cases = [(dict(m=15), "m must be"), (dict(m=-1), "m must be"), (dict(rm=bad(rm, 0.0)), "rm must be"), (dict(rm=bad(rm, np.nan)), "rm must be"),
             (dict(rm=bad(rm, -1.0)), "rm must be"), (dict(N0=None), "null"), (dict(navrep=None), "null"), (dict(H=None), "needs H"),
             (dict(rm=None), "needs H"), (dict(H=bad(H, np.inf)), "H must be"), (dict(S0=None), "null"), (dict(B=0), "B >= 1"),
             (dict(K=K - 1), "K must equal"), (dict(w=bad(np.zeros(14), -1.0)), "w must be")]
    for kw, word in cases:
        v = dict(B=5, K=K, x=x, u=u, d=d, gain=gain, S0=S0, N0=N0, m=6, H=H, rm=rm, w=None, rep=rep, navrep=navrep)
        v.update(kw)
        ptr = lambda n: None if v[n] is None else _p(np.ascontiguousarray(v[n]))   # noqa: E731
        hostp = [ptr("H"), ptr("rm"), ptr("w")]
        a_host = [v["B"], v["K"], ptr("x"), ptr("u"), ptr("d"), ptr("gain"), ptr("S0"), ptr("N0"), v["m"]] + hostp + [ptr("rep"), ptr("navrep")] + [None] * 4
        a_dev = ([v["B"], v["K"]] + [dev(v[n]) for n in ("x", "u", "d", "gain", "S0", "N0")] + [v["m"]] + hostp
                 + [dev(v["rep"]), dev(v["navrep"])] + [None] * 4)
        for fn, a in ((L.scvx_nav_cov_f64_host, a_host), (L.scvx_nav_cov_f64, a_dev)):
            assert fn(h, *a) == -1, (kw, fn)
            assert word in err(), (kw, err())
    assert np.all(rep == 7.0) and np.all(navrep == 7.0)                               # nothing ran
    bh = b.handle
    q, r, qf = np.ones(14), np.ones(3), np.full(14, 100.0)
    args = lambda **kw: [bh, _p(q), _p(r), _p(qf), kw.get("S0", _p(S0)), kw.get("N0", _p(N0)), kw.get("m", 6), _p(H), kw.get("rm", _p(rm)), None,   # noqa: E731
                         _p(rep), _p(navrep), None, None, None, None]
    assert L.scvx_batch_nav_cov(*args(N0=None)) == -1 and "null" in err()
    assert L.scvx_batch_nav_cov(*args(m=15)) == -1 and "m must be" in err()
    assert L.scvx_batch_nav_cov(*args(rm=_p(bad(rm, 0.0)))) == -1 and "rm must be" in err()
    assert np.all(rep == 7.0) and np.all(navrep == 7.0)
    nav = np.zeros((5, K, 14))
    fa = [5, K, _p(x), _p(u), _p(s), _p(gain), None, None, 10, 0, _p(rep), None, None]
    assert L.scvx_track_fly_nav_f64_host(h, *fa) == -1 and "null nav" in err()
    assert L.scvx_track_fly_nav_f64(h, *([5, K] + [dev(1)] * 4 + [None, None, 10, 0, dev(1), None, None])) == -1 and "null nav" in err()
    assert L.scvx_batch_track_fly_nav(bh, _p(q), _p(r), _p(qf), None, None, 0, 0, _p(rep), None, None) == -1 and "null nav" in err()
    assert np.all(rep == 7.0)
    with pytest.raises(_lib.ScvxError, match="rm must be"):
        b.navigation(S0, N0, H, 0.0)
    with pytest.raises(_lib.ScvxError, match="m must be"):
        nav_cov_batch(c, x, u, d, gain, S0, N0, np.ones((15, 14)), 1.0)
    with pytest.raises(ValueError):
        nav_cov_batch(c, x, u, d, gain, S0, N0[:4], H, rm)
    with pytest.raises(ValueError):
        track_fly_batch(c, x, u, s, gain, nav=nav[:, :-1])
    with pytest.raises(ValueError):
        b.track(nav=nav[:4])
    # every output of the batch form may be left out
    assert L.scvx_batch_nav_cov(bh, _p(q), _p(r), _p(qf), _p(S0), _p(N0), 6, _p(H), _p(rm), None, None, None, None, None, None, None) == 0
    # dense outputs: each on its own gives what all together give, and the reports do not depend on them
    good = nav_cov_batch(c, x, u, d, gain, S0, N0, H, rm, dense=True)
    lean = nav_cov_batch(c, x, u, d, gain, S0, N0, H, rm)
    assert np.array_equal(lean.raw, good.raw) and np.array_equal(lean.navraw, good.navraw)
    assert lean.sig is None and lean.navsig is None and lean.kf is None and lean.joint is None
    for nm in ("sig", "navsig", "kf", "joint"):
        only = nav_cov_batch(c, x, u, d, gain, S0, N0, H, rm, dense=(nm,))
        assert np.array_equal(getattr(only, nm), getattr(good, nm)), nm
        assert all(getattr(only, o) is None for o in ("sig", "navsig", "kf", "joint") if o != nm)
        assert np.array_equal(only.raw, good.raw) and np.array_equal(only.navraw, good.navraw)
    # a NaN in one trajectory's N0 (an Inf in another's gain, a NaN in a third's tile) poisons both reports of that row only
    for m_ in (0, 6):
        Hm, rmm = (H, rm) if m_ else (None, None)
        ok = nav_cov_batch(c, x, u, d, gain, S0, N0, Hm, rmm, dense=True)
        dn, gn, nn = d.copy(), gain.copy(), N0.copy()
        nn[2, 3, 5] = np.nan
        gn[3, 12, 1, 4] = np.inf
        dn.reshape(5, K, -1, 14)[1, 30, 2, 5] = np.nan
        pois = nav_cov_batch(c, x, u, dn, gn, S0, nn, Hm, rmm, dense=True)
        assert np.isnan(pois.raw[[1, 2, 3]]).all() and np.isnan(pois.navraw[[1, 2, 3]]).all(), (pois.raw, pois.navraw)
        assert np.array_equal(pois.raw[[0, 4]], ok.raw[[0, 4]]) and np.array_equal(pois.navraw[[0, 4]], ok.navraw[[0, 4]])
        assert np.array_equal(pois.joint[[0, 4]], ok.joint[[0, 4]])
        assert np.array_equal(pois.joint[1, :31], ok.joint[1, :31]) and np.isnan(pois.joint[1, 31]).any()
    b.close(), c.close()


def test_rocketland_navigation_single_problem():
    from successiveconvexification_amd import rocketland as rl, sample_problems as sp
    from successiveconvexification_amd.dynamics import IntegratorCache
    from successiveconvexification_amd.montecarlo import measurement_rows
    p = sp.base_prob_scaled
    c = IntegratorCache(p, npts=10)
    ip = rl.create_initial(p, c)
    ip, _, _ = rl.solve_step(ip, c)
    sd = np.zeros(14)
    sd[1:7] = 1e-3
    H = measurement_rows("r")
    r = rl.navigation(ip, c, sd, 0.5 * sd, H, 1e-8, dense=True)
    assert len(r) == 1 and r.joint.shape == (1, p.K + 1, 31, 31) and r.kf.shape == (1, p.K, 14, 3) and np.isfinite(r.navraw).all()
    rb = ip.model.navigation(sd, 0.5 * sd, H, 1e-8, dense=True)
    assert np.array_equal(r.raw, rb.raw) and np.array_equal(r.navraw, rb.navraw) and np.array_equal(r.joint, rb.joint)
    with pytest.raises(ValueError):
        rl.navigation(ip, c, sd)
    c.close()
