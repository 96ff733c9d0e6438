"""Sampled closed-loop dispersion flown on a navigation estimate (scvx_track_mc_nav_f64 / scvx_batch_track_mc_nav) on the MI355X: bit
for bit against scvx_track_mc_f64 where the estimate never errs and against the flyer on estimates (scvx_track_fly_nav_f64) fed the
errors this call formed; the error recursion against its longdouble reference (tests/mc_nav_reference.py); flights with impulses against
the CPU chain driven through the C oracle; the reduction against numpy on the dense outputs of the same launch; and the statistics
against the device's own navigation analysis WITH w.

Bounds, none of them taken from the device:
  * no estimate error, and against the flyer on estimates: equality.
  * the error recursion: 8 x the distance of the float64 numpy recursion from the longdouble one (the summation orders differ) plus
    4 ulp of max|eps|.
  * impulses against the CPU chain: K * 1e-12 * A_cl, test_gpu_mc.py's bound, A_cl the sensitivity of the REFERENCE chain.
  * reduction: MAX_FED exact; jmean 2 S eps max|v|; jcov 4 S eps max|v|^2 (test_gpu_mc.py's summation bounds); the squares of the
    trace columns of mcnav: the number of entries of their trace times the jcov bound.
  * statistics: six standard errors per entry (mc_reference.se_check's bound).
Every comparison prints its figures before it asserts.
"""
import ctypes as C

import numpy as np
import pytest

import cov_reference as cr
import mc_nav_reference as mn
import mc_reference as mr
import track_reference as tr
from test_gpu_flight import _case, _compare, _flyable
from test_gpu_mc import _check_reduction, _golden, _same

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
REDUCED = ("raw", "xmean", "xcov", "jmean", "jcov", "navraw")
DENSE = ("flights", "xland", "dx0", "navfed", "navK")


def _model(m, x0):
    """(H, rm) of the cases: m = 0 none; 3 the position; 6 position and velocity; 14 identity plus a fixed seeded perturbation.  1 sigma:
    3e-5 of the largest |r| / |v| component of x0 on r and v rows, 1e-4 on the others"""
    if m == 0:
        return None, None
    sd = np.full(14, 1e-4)
    sd[1:4], sd[4:7] = 3e-5 * np.abs(x0[1:4]).max(), 3e-5 * np.abs(x0[4:7]).max()
    if m in (3, 6):
        return np.eye(14)[1:1 + m], sd[1:1 + m] ** 2
    assert m == 14
    return np.eye(14) + 0.1 * np.random.default_rng(14).standard_normal((14, 14)), sd ** 2


def _s0(x):
    return np.stack([cr.handover_s0(x[b, 0])[0] for b in range(x.shape[0])])


def _all_same(r0, r1, names=REDUCED + DENSE):
    return all(_same(getattr(r0, n), getattr(r1, n)) for n in names)


def _golden3(c):
    """B = 3: the two golden plans and plan 0 again with another S0; device tiles and gains"""
    from successiveconvexification_amd.dynamics import linearize_batch, track_gains_batch
    pp, po, x, u, s = _golden()
    x3, u3, s3 = x[[0, 1, 0]], u[[0, 1, 0]], s[[0, 1, 0]]
    _, d = linearize_batch(c, x3, u3, s3, 1.0 / (po.K + 1))
    S0 = np.stack([cr.handover_s0(x[0, 0])[0], cr.handover_s0(x[1, 0])[0], cr.handover_s0(x[0, 0], seed=1, size=3e-3)[0]])
    return po, x3, u3, s3, d, track_gains_batch(c, d), S0


def _no_error_is_the_old_call(tag, c, x, u, s, d, L, S0, S, seed, nsub):
    from successiveconvexification_amd.dynamics import track_mc_batch, track_mc_nav_batch
    for clamp in (False, True):
        old = track_mc_batch(c, x, u, s, L, S0, S, seed=seed, nsub=nsub, clamp=clamp, dense=True)
        new = track_mc_nav_batch(c, x, u, s, d, L, S0, np.zeros((14, 14)), None, None, S, seed=seed, nsub=nsub, clamp=clamp, dense=True)
        same = {n: _same(getattr(old, n), getattr(new, n)) for n in ("raw", "xmean", "xcov", "flights", "xland", "dx0")}
        print("%s S %d clamp %s: bitwise %s; eps rows of jcov max %.1e, MAX_FED %s" % (tag, S, clamp, same, np.abs(new.jcov[:, 14:]).max(), new.MAX_FED))
        assert all(same.values()), same
        assert not new.jcov[:, 14:, :].any() and not new.jcov[:, :, 14:].any() and not new.navfed.any() and not new.navK.any()
        assert _same(new.jcov[:, :14, :14], old.xcov) and _same(new.jmean[:, :14], old.xmean) and not new.navraw[:, :6].any()
        # the estimate is the truth: the miss the vehicle believes it has is the miss it has
        dg = np.diagonal(old.xcov, axis1=1, axis2=2)
        assert np.allclose(new.EST_R, np.sqrt(dg[:, 1:4].sum(axis=1)), rtol=8 * EPS, atol=0)
        assert np.allclose(new.EST_V, np.sqrt(dg[:, 4:7].sum(axis=1)), rtol=8 * EPS, atol=0)


def test_no_estimate_error_is_the_old_call_on_the_golden_plans():
    """CN = 0, m = 0, no eta; B = 3, S = 130: three blocks per plan, the last with two live lanes"""
    from successiveconvexification_amd.dynamics import IntegratorCache
    pp = _flyable()[0]
    c = IntegratorCache(pp, npts=10)
    po, x, u, s, d, L, S0 = _golden3(c)
    _no_error_is_the_old_call("golden plans", c, x, u, s, d, L, S0, 130, 5, 10)
    c.close()


@pytest.mark.parametrize("model", ["exo", "aero+fins"])
def test_no_estimate_error_is_the_old_call_at_a_short_horizon(model, aero_tables):
    import horizon_cases as hc
    from successiveconvexification_amd.dynamics import IntegratorCache, linearize_batch, track_gains_batch
    pp, po, dyn, par, x, u, s = hc.case(model, 3, aero_tables)
    c = IntegratorCache(pp, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (po.K + 1))
    _no_error_is_the_old_call("%s K = 3" % model, c, x, u, s, d, track_gains_batch(c, d), _s0(x), 5, 7, 2)
    c.close()


def _bitwise_against_the_flyer_on_estimates(tag, c, x, u, s, d, L, S0, m, S, seed, nsub=10):
    from successiveconvexification_amd.dynamics import track_fly_batch, track_mc_nav_batch
    B, K = x.shape[0], x.shape[1] - 1
    H, rm = _model(m, x[0, 0])
    for clamp in (False, True):
        r = track_mc_nav_batch(c, x, u, s, d, L, S0, 0.25 * S0, H, rm, S, seed=seed, nsub=nsub, clamp=clamp, dense=True)
        assert r.navfed.shape == (B, S, K, 14) and r.navK.shape == (B, S, 14) and r.navfed.any()
        t = track_fly_batch(c, cr.rep(x, S), cr.rep(u, S), cr.rep(s, S), cr.rep(L, S), r.dx0.reshape(B * S, 14), nsub=nsub, clamp=clamp,
                            dense=True, nav=r.navfed.reshape(B * S, K, 14))
        fl, xl = r.flights.reshape(B * S, 16), r.xland.reshape(B * S, 14)
        print("%s m %d S %d clamp %s: flights bitwise %s (largest difference %.3e), xland bitwise %s, finite flights %d of %d, MAX_FED %s"
              % (tag, m, S, clamp, _same(fl, t.raw), np.nanmax(np.abs(np.nan_to_num(fl - t.raw, posinf=0, neginf=0))), _same(xl, t.xfly[:, K]),
                 np.isfinite(fl[:, 0]).sum(), B * S, r.MAX_FED))
        assert _same(fl, t.raw)
        assert _same(xl, t.xfly[:, K])
        quiet = track_mc_nav_batch(c, x, u, s, d, L, S0, np.zeros((14, 14)), None, None, S, seed=seed, nsub=nsub, clamp=clamp, dense=True)
        assert not _same(quiet.xland, r.xland)                      # the estimate's error is felt


def test_bitwise_against_the_flyer_on_estimates_on_the_golden_plans():
    from successiveconvexification_amd.dynamics import IntegratorCache
    c = IntegratorCache(_flyable()[0], npts=10)
    po, x, u, s, d, L, S0 = _golden3(c)
    _bitwise_against_the_flyer_on_estimates("golden plans", c, x, u, s, d, L, S0, 6, 130, 5)
    c.close()


def test_bitwise_against_the_flyer_on_estimates_on_unconverged_torque_plans(aero_tables):
    from successiveconvexification_amd.dynamics import IntegratorCache, linearize_batch, track_gains_batch
    pp, po, dyn, par, x, u, s = _case("aero+fins+torque", aero_tables)
    c = IntegratorCache(pp, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (po.K + 1))
    _bitwise_against_the_flyer_on_estimates("aero+fins+torque B = 5 unconverged", c, x, u, s, d, track_gains_batch(c, d), _s0(x), 3, 130, 6)
    c.close()


def _recursion_against_the_reference(tag, c, x, u, s, d, L, S0, S, seed, nsub, ms=(0, 3, 6, 14)):
    """navfed and navK of the device against the longdouble recursion from the same draws, gains and tiles, over m and eta"""
    from successiveconvexification_amd.dynamics import nav_cov_batch, track_mc_nav_batch
    from successiveconvexification_amd.montecarlo import handover_factor, mc_draws, mc_nav_draws
    B, K = x.shape[0], x.shape[1] - 1
    N0 = 0.25 * S0
    w = np.full(14, 1e-8)
    w[0] = 0.0
    for m in ms:
        H, rm = _model(m, x[0, 0])
        xin, nud = mc_nav_draws(S, K, m, seed)
        for noise in (False, True):
            wv = w if noise else None
            kf = nav_cov_batch(c, x, u, d, L, np.zeros((B, 14, 14)), N0, H, rm, wv, dense=("kf",)).kf if m else None
            r = track_mc_nav_batch(c, x, u, s, d, L, S0, N0, H, rm, S, seed=seed, w=wv, kf=kf, nsub=nsub, dense=("navfed", "navK"))
            eta = mc_draws(S, K, seed, noise=True)[1] if noise else None
            for b in range(B):
                CN = handover_factor(N0[b])
                a = (d[b], None if kf is None else kf[b], H, rm, CN, xin, nud, wv, eta)
                f64, b64 = mn.eps_recursion(*a)
                fld, bld = mn.eps_recursion(*a, dtype=np.longdouble)
                own = float(max(np.abs(f64 - fld).max(), np.abs(b64 - bld).max()))
                big = float(np.abs(bld).max())
                bound = 8.0 * own + 4.0 * EPS * big
                dev = float(max(np.abs(r.navfed[b] - fld).max(), np.abs(r.navK[b] - bld[:, K]).max()))
                print("%s plan %d m %d eta %s: max|eps| %.3e, float64 numpy vs longdouble %.3e, device vs longdouble %.3e (bound %.3e)"
                      % (tag, b, m, noise, big, own, dev, bound))
                assert np.isfinite(r.navfed[b]).all() and dev <= bound, (tag, b, m, noise, dev, bound)
            if noise:
                assert not _same(r.navK, quiet_K)                   # the impulses reach the error
            quiet_K = r.navK


@pytest.mark.parametrize("model", ["exo", "aero+fins"])
def test_error_recursion_against_the_reference_at_a_short_horizon(model, aero_tables):
    import horizon_cases as hc
    from successiveconvexification_amd.dynamics import IntegratorCache, linearize_batch, track_gains_batch
    pp, po, dyn, par, x, u, s = hc.case(model, 3, aero_tables)
    c = IntegratorCache(pp, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (po.K + 1))
    _recursion_against_the_reference("%s K = 3" % model, c, x, u, s, d, track_gains_batch(c, d), _s0(x), 5, 21, 2)
    c.close()


def test_error_recursion_against_the_reference_on_the_golden_plans():
    from successiveconvexification_amd.dynamics import IntegratorCache
    c = IntegratorCache(_flyable()[0], npts=10)
    po, x, u, s, d, L, S0 = _golden3(c)
    _recursion_against_the_reference("golden plans K = 50", c, x, u, s, d, L, S0, 5, 22, 10)
    c.close()


def _impulse_parity(tag, c, po, dyn, par, x, u, s, m, nsub, S, seed):
    from successiveconvexification_amd.dynamics import linearize_batch, nav_cov_batch, track_mc_nav_batch
    from successiveconvexification_amd.montecarlo import handover_factor, mc_draws, mc_nav_draws
    B, K = x.shape[0], po.K
    _, d = linearize_batch(c, x, u, s, 1.0 / (K + 1))
    L, _ = tr.gains(d, K)                                          # the REFERENCE's gains, fed to both sides
    S0 = _s0(x)
    N0 = 0.25 * S0
    H, rm = _model(m, x[0, 0])
    w = np.full(14, 1e-8)
    w[0] = 0.0
    xi0, eta = mc_draws(S, K, seed, noise=True)
    xin, nud = mc_nav_draws(S, K, m, seed)
    kf = nav_cov_batch(c, x, u, d, L, np.zeros((B, 14, 14)), N0, H, rm, w, dense=("kf",)).kf
    dev = track_mc_nav_batch(c, x, u, s, d, L, S0, N0, H, rm, S, seed=seed, w=w, kf=kf, nsub=nsub, dense=True)
    imp = eta * np.sqrt(w)
    taken = []                                                     # per plan: was the count comparison below made
    for b in range(B):
        dx0 = xi0 @ handover_factor(S0[b]).T
        fed, before = mn.eps_recursion(d[b], kf[b], H, rm, handover_factor(N0[b]), xin, nud, w, eta)
        ref, xref, _, cmd = mn.fly_plan(dyn, po, x[b], u[b], s[b], L[b], dx0, fed, nsub, 0, imp, par)
        A = mn.sensitivity(dyn, po, x[b], u[b], s[b], L[b], dx0, fed, nsub, 1e-9, 0, imp, par=par)
        bound = K * 1e-12 * A
        dxl = float(np.abs(dev.xland[b] - xref[:, -1]).max())
        print("%s plan %d m %d nsub %d: A_cl %.3f, bound %.3e, xland %.3e, dx0 %.3e, navfed %.3e"
              % (tag, b, m, nsub, A, bound, dxl, np.abs(dev.dx0[b] - dx0).max(), np.abs(dev.navfed[b] - fed).max()))
        assert dxl <= bound
        _compare("%s plan %d nsub %d" % (tag, b, nsub), dev.flights[b], ref, bound, po)
        lo, hi = mr.out_counts(cmd, po.Tmin, po.Tmax)
        margin = float(np.minimum(np.abs(cmd - po.Tmin), np.abs(cmd - po.Tmax)).min())
        print("    commanded norms outside the band: reference %d / %d, device %.1f / %.1f (closest to a bound %.3e)"
              % (lo, hi, dev.OUT_LO[b] * S * K, dev.OUT_HI[b] * S * K, margin))
        taken.append(margin > bound * max(1.0, float(np.abs(L).max())))
        if taken[-1]:
            assert dev.OUT_LO[b] == lo / (S * K) and dev.OUT_HI[b] == hi / (S * K)
    return taken


@pytest.mark.parametrize("model,m", [("exo", 3), ("aero+fins", 14)])
def test_impulses_against_the_cpu_chain_at_a_short_horizon(model, m, aero_tables):
    import horizon_cases as hc
    from successiveconvexification_amd.dynamics import IntegratorCache
    pp, po, dyn, par, x, u, s = hc.case(model, 3, aero_tables)
    c = IntegratorCache(pp, npts=10)
    _impulse_parity("%s K = 3" % model, c, po, dyn, par, x, u, s, m, 2, 5, 31)
    c.close()


def test_impulses_against_the_cpu_chain_on_the_golden_plans():
    from oracle import dynamics as od
    from successiveconvexification_amd.dynamics import IntegratorCache
    pp, po, x, u, s = _golden()
    c = IntegratorCache(pp, npts=10)
    _impulse_parity("golden plans K = 50", c, po, od, od.Params(po), x, u, s, 6, 10, 5, 32)
    c.close()


def _check_nav_reduction(tag, x, rep):
    """jmean, jcov and mcnav of one launch against numpy on its own dense outputs"""
    B, S, K, _ = rep.navfed.shape
    I = mn.MCNAV_IDX
    for b in range(B):
        e = rep.xland[b] - x[b, -1]
        jm, jc, nav = mn.reduce(e, rep.navK[b], rep.navfed[b])
        v = np.concatenate([e, rep.navK[b]], axis=1)
        vmax = float(np.abs(v).max())
        em, ec = np.abs(rep.jmean[b] - jm), np.abs(rep.jcov[b] - jc)
        bc = 4 * S * EPS * vmax ** 2
        print("%s plan %d: jmean %.3e (bound %.3e), jcov %.3e (bound %.3e), mcnav device %s reference %s"
              % (tag, b, em.max(), 2 * S * EPS * vmax, ec.max(), bc, rep.navraw[b], nav))
        assert np.all(em <= 2 * S * EPS * np.abs(v).max(axis=0))
        assert ec.max() <= bc
        assert _same(rep.jcov[b], rep.jcov[b].T)
        assert rep.navraw[b, I["MAX_FED"]] == nav[I["MAX_FED"]] == np.abs(rep.navfed[b]).max()
        for name, terms in (("NAV_M", 1), ("NAV_R", 3), ("NAV_V", 3), ("NAV_Q", 4), ("NAV_W", 3), ("EST_R", 12), ("EST_V", 12)):
            dv, rf = rep.navraw[b, I[name]], nav[I[name]]
            assert abs(dv * dv - rf * rf) <= terms * bc + 8 * EPS * rf * rf, (tag, b, name, dv, rf)
    assert _same(rep.xcov, rep.jcov[:, :14, :14]) and _same(rep.xmean, rep.jmean[:, :14])


def test_reduction_against_numpy_on_the_dense_outputs():
    from successiveconvexification_amd.dynamics import IntegratorCache, track_mc_nav_batch
    c = IntegratorCache(_flyable()[0], npts=10)
    po, x, u, s, d, L, S0 = _golden3(c)
    N0 = 0.25 * S0
    H, rm = _model(6, x[0, 0])
    w = np.full(14, 1e-8)
    w[0] = 0.0
    S = 130
    for clamp, wv in ((False, None), (True, w)):
        kw = dict(seed=3, w=wv, nsub=10, clamp=clamp, tol=1e-6)
        base = track_mc_nav_batch(c, x, u, s, d, L, S0, N0, H, rm, S, dense=True, **kw)
        _check_reduction("golden plans, on an estimate, clamp %s, w %s" % (clamp, wv is not None), po, x, base, 1e-6)
        _check_nav_reduction("golden plans, clamp %s, w %s" % (clamp, wv is not None), x, base)
        again = track_mc_nav_batch(c, x, u, s, d, L, S0, N0, H, rm, S, dense=True, **kw)
        assert _all_same(base, again)                               # two launches: bit for bit
        lean = track_mc_nav_batch(c, x, u, s, d, L, S0, N0, H, rm, S, **kw)
        assert _all_same(base, lean, REDUCED) and all(getattr(lean, n) is None for n in DENSE)
    r64 = track_mc_nav_batch(c, x, u, s, d, L, S0, N0, H, rm, 64, seed=3, w=w, nsub=10, dense=True)
    r65 = track_mc_nav_batch(c, x, u, s, d, L, S0, N0, H, rm, 65, seed=3, w=w, nsub=10, dense=True)
    assert _all_same(r64, type("prefix", (), {n: getattr(r65, n)[:, :64] for n in DENSE}), DENSE)
    _check_nav_reduction("S = 64", x, r64)
    _check_nav_reduction("S = 65", x, r65)
    one = track_mc_nav_batch(c, x, u, s, d, L, S0, N0, H, rm, 1, seed=3, w=w, nsub=10, dense=True)
    assert not one.xcov.any() and not one.jcov.any() and np.all(one.S == 1) and not one.navraw[:, [0, 1, 2, 3, 4, 6, 7]].any()
    assert _same(one.jmean[:, 14:], one.navK[:, 0]) and _same(one.MAX_FED, np.abs(one.navfed).max(axis=(1, 2, 3))) and _same(one.navK[:, 0], r64.navK[:, 0])
    c.close()


def test_statistics_on_the_device_within_six_standard_errors():
    """the CPU check's inputs and S (test_mc_nav_cpu.nav_case): jcov from the device against the device's own navigation analysis with w"""
    from test_mc_nav_cpu import NAV_SAMPLES, NAV_SEED, nav_case
    from successiveconvexification_amd.dynamics import IntegratorCache, linearize_batch, nav_cov_batch, track_gains_batch, track_mc_nav_batch
    p, par, x, u, s, d_ref, L_ref, S0, N0, H, rm, w, XiK_ref, kf_ref = nav_case()
    pp, po = _flyable()
    c = IntegratorCache(pp, npts=10)
    sl = slice(0, 1)
    _, d = linearize_batch(c, x[sl], u[sl], s[sl], 1.0 / (po.K + 1))
    L = track_gains_batch(c, d)
    n = 14 + c.nu
    XiK = nav_cov_batch(c, x[sl], u[sl], d, L, S0[None], N0[None], H, rm, w, dense=("joint",)).joint[0, -1]
    r = track_mc_nav_batch(c, x[sl], u[sl], s[sl], d, L, S0, N0, H, rm, NAV_SAMPLES, seed=NAV_SEED, w=w, nsub=10)
    worst, over = mn.se_check(r.jcov[0], XiK, n, NAV_SAMPLES)
    quiet = track_mc_nav_batch(c, x[sl], u[sl], s[sl], d, L, S0, N0, H, rm, NAV_SAMPLES, seed=NAV_SEED, nsub=10)
    worst0, over0 = mn.se_check(quiet.jcov[0], XiK, n, NAV_SAMPLES)
    print("device, plan 0, S = %d: worst entry of jcov %.2f standard errors, %d over 6 (without process noise: %.2f, %d over 6); device Xi_K vs "
          "the reference's %.3e; NAV_R %.3e EST_R %.3e MAX_FED %.3e"
          % (NAV_SAMPLES, worst, over, worst0, over0, np.abs(XiK - XiK_ref).max(), r.NAV_R[0], r.EST_R[0], r.MAX_FED[0]))
    assert r.N_BAD[0] == 0 and r.S[0] == NAV_SAMPLES
    assert over == 0, (worst, over)
    c.close()


def _raw_call(c, x, u, s, d, L, c0, cn, xi0, xin, nud, m, H, rm, kf):
    """scvx_track_mc_nav_f64_host on explicit factors, every dense output: a McNavReport"""
    from successiveconvexification_amd import _calls
    from successiveconvexification_amd.dynamics import McNavReport
    B, K, S = x.shape[0], x.shape[1] - 1, xi0.shape[0]
    f = dict(x=x, u=u, sigma=s, gain=L, C0=c0, xi0=xi0, deriv=d, kf=kf, CN=cn, xin=xin, nud=nud, H=H, rm=rm)
    f = {k: np.ascontiguousarray(v, np.float64) for k, v in f.items()}
    f.update(_calls.mc_outputs(B, K, S, _calls.MC_NAV_REDUCED + _calls.MC_NAV_DENSE), handle=c.handle, B=B, K=K, S=S, eta=None, w14=None,
             m=m, nsub=10, flags=0, tol=0.0)
    _calls.call(c._L, c.handle, "scvx_track_mc_nav_f64_host", f)
    return McNavReport(*[f[k] for k in _calls.MC_NAV_REDUCED + _calls.MC_NAV_DENSE])


def test_a_nan_poisons_only_its_plan():
    from successiveconvexification_amd.dynamics import IntegratorCache, nav_cov_batch
    from successiveconvexification_amd.montecarlo import handover_factor, mc_draws, mc_nav_draws
    c = IntegratorCache(_flyable()[0], npts=10)
    po, x, u, s, d, L, S0 = _golden3(c)
    N0 = 0.25 * S0
    m, S, K = 6, 70, po.K
    H, rm = _model(m, x[0, 0])
    kf = nav_cov_batch(c, x, u, d, L, np.zeros((3, 14, 14)), N0, H, rm, dense=("kf",)).kf
    c0, cn = (np.stack([handover_factor(v[b]) for b in range(3)]) for v in (S0, N0))
    xi0, (xin, nud) = mc_draws(S, K, 9)[0], mc_nav_draws(S, K, m, 9)
    good = _raw_call(c, x, u, s, d, L, c0, cn, xi0, xin, nud, m, H, rm, kf)
    assert np.all(good.N_BAD == 0) and np.isfinite(good.jcov).all()
    kfn, dn, cnn = kf.copy(), d.copy(), cn.copy()
    kfn[1, 20, 3, 2] = np.nan
    dn[2, K - 1, 5, 3] = np.nan          # the state block of the LAST tile: only eps_K reads it
    cnn[0, 4, 4] = np.inf
    for tag, row, kw in (("kf", 1, dict(kf=kfn)), ("tile", 2, dict(d=dn)), ("CN", 0, dict(cn=cnn))):
        v = dict(d=d, cn=cn, kf=kf)
        v.update(kw)
        bad = _raw_call(c, x, u, s, v["d"], L, c0, v["cn"], xi0, xin, nud, m, H, rm, v["kf"])
        print("non-finite %s of plan %d: N_BAD %s, MAX_GAP %s, MAX_FED %s, NAV_R %s" % (tag, row, bad.N_BAD, bad.MAX_GAP, bad.MAX_FED, bad.NAV_R))
        assert bad.N_BAD[row] == S and np.isnan(bad.MAX_GAP[row]) and np.isnan(bad.MEAN_GAP[row]) and np.isnan(bad.flights[row, :, 0]).all()
        assert np.isnan(bad.xcov[row]).any() and np.isnan(bad.jcov[row, 14:, 14:]).any() and np.isnan(bad.jmean[row]).any()
        assert np.isnan(bad.NAV_R[row]) and bad.S[row] == S
        others = [b for b in range(3) if b != row]
        for nme in REDUCED + DENSE:
            assert _same(getattr(bad, nme)[others], getattr(good, nme)[others]), (tag, nme)
    c.close()


def test_batch_level_call_and_the_batch_is_untouched():
    import bench
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache, track_mc_nav_batch
    from successiveconvexification_amd.montecarlo import measurement_rows
    pp, po = _flyable()
    B = 4
    c = IntegratorCache(pp, npts=10)
    b = ScvxBatch(c, B).init(bench.disperse_ics(pp, 0, B, 7))
    st, it, _, _ = b.solve()
    print("statuses after scvx_solve %s" % st.tolist())
    before = (b.trajectory_record(),) + b.scalars() + b.flags() + b.linearization()
    x, u, s = b.trajectory()
    sd = np.zeros(14)
    sd[1:7] = 1e-3 * np.abs(x[0, 0, 1:7])
    sd[7:] = 1e-3
    w = np.full(14, 1e-9)
    H = measurement_rows("rv")
    rm = np.repeat([(3e-5 * np.abs(x[0, 0, 1:4]).max()) ** 2, (3e-5 * np.abs(x[0, 0, 4:7]).max()) ** 2], 3)
    nav = (0.5 * sd, H, rm)

    def host(**kw):
        kf = b.navigation(sd, 0.5 * sd, H, rm, w=kw.get("w"), dense=("kf",)).kf
        return track_mc_nav_batch(c, x, u, s, b.linearization()[1], b.track_gains(), sd, 0.5 * sd, H, rm, 70, seed=4, kf=kf, nsub=10, **kw)

    for clamp in (False, True):
        rb = b.track_mc(sd, samples=70, seed=4, w=w, clamp=clamp, tol=1e-6, dense=True, nav=nav)
        rh = host(w=w, clamp=clamp, tol=1e-6, dense=True)
        print("batch, clamp %s: bitwise %s" % (clamp, {n: _same(getattr(rb, n), getattr(rh, n)) for n in REDUCED + DENSE}))
        assert _all_same(rb, rh) and rb.navfed.shape == (B, 70, po.K, 14)
    print("batch: P_ANY %s NAV_R %s EST_R %s MAX_FED %s" % (rb.P_ANY, rb.NAV_R, rb.EST_R, rb.MAX_FED))
    lean = b.track_mc(sd, samples=70, seed=4, w=w, clamp=True, tol=1e-6, nav=nav)
    assert _all_same(lean, rb, REDUCED) and lean.navfed is None
    assert not _same(rb.raw, b.track_mc(sd, samples=70, seed=4, w=w, clamp=True, tol=1e-6).raw)      # nav=None: the call it was
    inertial = b.track_mc(sd, samples=70, seed=4, nav=(0.5 * sd, None, None), dense=True)
    assert _all_same(inertial, track_mc_nav_batch(c, x, u, s, b.linearization()[1], b.track_gains(), sd, 0.5 * sd, None, None, 70, seed=4,
                                                  nsub=10, dense=True))
    # float tiles: the gains, the filter gains and the error's transport come from the widened tiles
    b.set_linearization_f32(True)
    r32 = b.track_mc(sd, samples=70, seed=4, w=w, dense=True, nav=nav)
    h32 = host(w=w, dense=True)
    print("float tiles: bitwise %s" % {n: _same(getattr(r32, n), getattr(h32, n)) for n in REDUCED + DENSE})
    assert _all_same(r32, h32) and not _same(r32.navK, rb.navK)
    b.set_linearization_f32(False)
    after = (b.trajectory_record(),) + b.scalars() + b.flags() + b.linearization()
    for a0, a1 in zip(before, after):
        assert _same(a0, a1)
    b.close(), c.close()


def test_rocketland_track_mc_single_problem_on_an_estimate():
    from successiveconvexification_amd import rocketland as rl, sample_problems as sp
    from successiveconvexification_amd.dynamics import IntegratorCache, McNavReport
    from successiveconvexification_amd.montecarlo import measurement_rows
    p = sp.base_prob_scaled
    c = IntegratorCache(p, npts=10)
    ip = rl.create_initial(p, c)
    ip, _, _ = rl.solve_step(ip, c)
    sd = np.zeros(14)
    sd[1:7] = 1e-3
    nav = (0.5 * sd, measurement_rows("r"), 1e-8)
    r = rl.track_mc(ip, c, sd, samples=66, seed=2, w=1e-9, dense=True, nav=nav)
    assert isinstance(r, McNavReport) and len(r) == 1 and r.navfed.shape == (1, 66, p.K, 14) and r.S[0] == 66 and np.isfinite(r.raw[0, :13]).all()
    rb = ip.model.track_mc(sd, samples=66, seed=2, w=1e-9, dense=True, nav=nav)
    print("single problem: bitwise %s; NAV_R %s MAX_FED %s" % ({n: _same(getattr(r, n), getattr(rb, n)) for n in REDUCED + DENSE}, r.NAV_R, r.MAX_FED))
    assert _all_same(r, rb)
    assert not isinstance(rl.track_mc(ip, c, sd, samples=66, seed=2), McNavReport)
    with pytest.raises(ValueError):
        rl.track_mc(ip, c, sd, nav=(None, None, None))
    c.close()


def test_arguments_are_checked():
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache, _p, linearize_batch, track_gains_batch, track_mc_nav_batch
    pp, po, x, u, s = _golden()
    c = IntegratorCache(pp, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (po.K + 1))
    gain = track_gains_batch(c, d)
    L, h, K, S, m = c._L, c.handle, pp.K, 4, 6
    C0 = np.ascontiguousarray(np.stack([np.eye(14) * 1e-3] * 2))
    CN = 0.5 * C0
    N0 = np.ascontiguousarray(np.einsum("bij,bkj->bik", CN, CN))
    H, rm = _model(m, x[0, 0])
    H = np.ascontiguousarray(H)
    xi0, eta, xin, nud, kf = np.zeros((S, 14)), np.zeros((S, K, 14)), np.zeros((S, 14)), np.zeros((S, K, m)), np.zeros((2, K, 14, m))
    outs = dict(rep=np.full((2, 48), 7.0), xm=np.full((2, 14), 7.0), xc=np.full((2, 14, 14), 7.0), jm=np.full((2, 28), 7.0),
                jc=np.full((2, 28, 28), 7.0), nv=np.full((2, 8), 7.0))
    err = lambda: L.scvx_last_error(h).decode()   # noqa: E731
    dev = lambda v: C.c_void_p(1) if v is not None else None   # noqa: E731  the checks come before any device pointer is used

    def bad(a, v):
        a = np.array(a, float)
        a.reshape(-1)[1] = v
        return a

    cases = [(dict(S=0), "S >= 1"), (dict(B=0), "B"), (dict(K=K - 1), "K must equal"), (dict(nsub=0), "nsub"), (dict(nsub=1001), "nsub"),
             (dict(flags=2), "unknown flags"), (dict(w=bad(np.zeros(14), -1.0)), "w must be"), (dict(w=bad(np.zeros(14), np.nan)), "w must be"),
             (dict(w=bad(np.zeros(14), np.inf)), "w must be"), (dict(tol=-1.0), "tol must be"), (dict(tol=np.nan), "tol must be"),
             (dict(eta=eta, w=None), "eta without w14"), (dict(m=15), "m must be"), (dict(m=-1), "m must be"), (dict(rm=bad(rm, 0.0)), "rm must be"),
             (dict(rm=bad(rm, np.nan)), "rm must be"), (dict(H=None), "needs H"), (dict(rm=None), "needs H"), (dict(H=bad(H, np.inf)), "H must be"),
             (dict(kf=None), "needs kf"), (dict(nud=None), "needs kf")]
    cases += [({n: None}, "null") for n in ("x", "u", "s", "gain", "C0", "xi0", "d", "CN", "xin", "rep", "xm", "xc", "jm", "jc", "nv")]
    ptrs = ("x", "u", "s", "gain", "C0", "xi0", "eta")
    navp = ("d", "kf", "CN", "xin", "nud")
    for kw, word in cases:
        v = dict(B=2, K=K, S=S, x=x, u=u, s=s, gain=gain, C0=C0, xi0=xi0, eta=None, w=np.zeros(14), d=d, kf=kf, CN=CN, xin=xin, nud=nud, m=m,
                 H=H, rm=rm, nsub=10, flags=0, tol=0.0, **outs)
        v.update(kw)
        host = lambda n: None if v[n] is None else _p(np.ascontiguousarray(v[n]))   # noqa: E731
        mid = [v["m"], host("H"), host("rm"), v["nsub"], v["flags"], v["tol"]]
        a_host = [v["B"], v["K"], v["S"]] + [host(n) for n in ptrs] + [host("w")] + [host(n) for n in navp] + mid + \
                 [host(n) for n in outs] + [None] * 5
        a_dev = [v["B"], v["K"], v["S"]] + [dev(v[n]) for n in ptrs] + [host("w")] + [dev(v[n]) for n in navp] + mid + \
                [dev(v[n]) for n in outs] + [None] * 5
        for fn, a in ((L.scvx_track_mc_nav_f64_host, a_host), (L.scvx_track_mc_nav_f64, a_dev)):
            assert fn(h, *a) == -1, (kw, fn)
            assert word in err(), (kw, err())
    assert all(np.all(o == 7.0) for o in outs.values())                               # nothing ran
    b = ScvxBatch(c, 2).init(None)
    b.set_trajectory(x, u, s)
    q, r, qf = np.ones(14), np.ones(3), np.full(14, 100.0)
    o = [_p(outs[n]) for n in outs]
    call = lambda **kw: L.scvx_batch_track_mc_nav(b.handle, kw.get("q", _p(q)), _p(kw.get("r", r)), _p(qf), kw.get("S", S), kw.get("C0", _p(C0)),   # noqa: E731
                                                  _p(xi0), kw.get("eta", None), kw.get("w", _p(np.zeros(14))), kw.get("N0", _p(N0)),
                                                  kw.get("CN", _p(CN)), _p(xin), kw.get("nud", _p(nud)), kw.get("m", m), _p(H),
                                                  kw.get("rm", _p(rm)), kw.get("nsub", 0), kw.get("flags", 0), kw.get("tol", 0.0), *o, None, None,
                                                  None, None, None)
    for kw, word in ((dict(S=0), "S >= 1"), (dict(C0=None), "null"), (dict(N0=None), "null"), (dict(CN=None), "null"), (dict(nud=None), "needs kf"),
                     (dict(eta=_p(eta), w=None), "eta without w14"), (dict(flags=4), "unknown flags"), (dict(m=15), "m must be"),
                     (dict(rm=_p(bad(rm, -1.0))), "rm must be"), (dict(tol=-1e-9), "tol must be"), (dict(nsub=2000), "nsub"),
                     (dict(r=np.zeros(3)), "r must be"), (dict(q=None), "null")):
        assert call(**kw) == -1 and word in err(), (kw, err())
    assert all(np.all(v == 7.0) for v in outs.values())
    assert call() == 0 and np.all(outs["rep"][:, 45] == S) and not np.any(outs["jc"] == 7.0)     # and with every argument in order it runs
    with pytest.raises(ValueError):
        track_mc_nav_batch(c, x, u, s, d, gain, np.full(14, 1e-3), np.full(14, 1e-3), H, rm, 0)
    with pytest.raises(ValueError):
        track_mc_nav_batch(c, x, u, s, d, gain, np.full(14, 1e-3), np.full(14, 1e-3), H, rm, 4, kf=kf[:, :, :, :3])
    with pytest.raises(ValueError):
        track_mc_nav_batch(c, x, u, s, d[:, :, :20], gain, np.full(14, 1e-3), np.full(14, 1e-3), H, rm, 4)
    with pytest.raises(ValueError):
        b.track_mc(np.full(14, 1e-3), samples=4, nav=(np.full(14, 1e-3), H))
    b.close(), c.close()
