"""Per-flight vehicle errors in the sampled closed-loop dispersion (scvx_track_mc_veh_f64, scvx_track_mc_nav_veh_f64, their batch forms;
vehicle= in Python) on the MI355X.

Bounds, none of them taken from the device:
  * veh = NULL through the new entry points against the _q / _rng calls, the device's draws against uploaded ones, shards, independent
    rows, the batch calls against the context-level ones: bit for bit.
  * mu = sp = 0 against the plain call, and every flight against the CPU chain through the C oracle (tests/mc_vehicle_reference.py):
    K * 1e-12 * A_cl, test_gpu_mc.py's closed-loop bound, with A_cl the sensitivity the REFERENCE chain (vehicle errors included)
    shows; G_* columns times flight_reference.g_lipschitz.  theta against fma(sp, zeta, mu) in exact arithmetic: equality.
  * dumped theta against the longdouble reference: test_gpu_mc_rng.py's rule, 8 x the float64 twin's own distance plus 4 ulp, on zeta
    (sp a power of two, mu = 0: theta / sp is zeta exactly).
  * J = d x_K / d theta against the CPU's: both are central differences of the SAME step h = 2^-10, so their truncation errors cancel
    and they differ by the flights' rounding only, 2 (K 1e-12 A_cl) / (2 h) = K 1e-12 A_cl / h.
  * statistics: six standard errors per entry (mc_reference.se_check), pooled over 8 x 1,024 independent flights.
Every comparison prints its figures before it asserts.  Recorded on one MI355X: mu = sp = 0 is NOT bitwise the plain call (landings within
2.6e-15, bounds 9.0e-11 and 4.8e-10), so only the bound is asserted; against the CPU chain the landings agree within 5.6e-14 (K = 50,
bounds from 8.4e-11) and 5.3e-14 (K = 3, bounds from 1.5e-11); theta / sp within 1.9 ulp of the longdouble reference; J within 2.3e-12 of
the CPU's (bound 9.2e-8); pooled statistics 2.56 standard errors; AERO on the CPU anchor's aerodynamic plan (K = 3, 1 sigma 0.1): its
column of J within 6.8e-13 of the CPU's (bound 1.5e-8), pooled statistics 2.31 standard errors (93 entries over 6 against Sigma_K
alone).  AERO moves the landing of these plans by 1.7e-7 .. 3.2e-4 at a 1 sigma
of 0.1 (the aerodynamic forces of these problems are small), above 10 x the bound in every case.
"""
import ctypes as C

import numpy as np
import pytest

import cov_reference as cr
import mc_reference as mr
import mc_rng_reference as rr
import mc_vehicle_reference as vr
from test_gpu_flight import _compare
from test_gpu_mc import _golden, _same
from test_gpu_mc_nav import _model
from test_gpu_mc_quantiles import _plans
from test_gpu_mc_rng import OLD, OLD_NAV, PROBS, _dump, _eq

pytestmark = pytest.mark.gpu

W = np.full(14, 1e-8)
W[0] = 0.0
# 1 sigma and mean of the parity cases: far above rounding; AERO large because the aerodynamic forces of these problems are small
SP_ALL = np.array([2e-3, 1e-3, 1.5e-3, 3e-3, 1e-1, 1e-2])
MU_ALL = np.array([-1e-3, 5e-4, -7e-4, 2e-3, -5e-2, 5e-3])


def _veh(c, sp=SP_ALL, mu=None):
    """(mu, sp) with the components the context's model lacks zeroed"""
    from successiveconvexification_amd.dynamics import AtmosphericData
    sp, mu = np.array(sp, float), np.zeros(6) if mu is None else np.array(mu, float)
    if not isinstance(c.problem.aero, AtmosphericData):
        sp[4] = mu[4] = 0.0
    if c.nu != 5:
        sp[5] = mu[5] = 0.0
    return mu, sp


def _null_veh(monkeypatch, L):
    """the four _veh entry points the Python layer calls, with veh, zeta and theta replaced by NULL on the way in"""
    for name in ("scvx_track_mc_veh_f64_host", "scvx_track_mc_nav_veh_f64_host", "scvx_batch_track_mc_veh", "scvx_batch_track_mc_nav_veh"):
        monkeypatch.setattr(L, name, (lambda f: lambda *a: f(*a[:-3], None, None, None))(getattr(L, name)))


@pytest.mark.parametrize("m", [None, 0, 3, 14])
@pytest.mark.parametrize("model", ["exo", "aero+fins+torque"])
def test_null_veh_is_the_q_and_the_rng_call(model, m, aero_tables, monkeypatch):
    """veh = NULL through scvx_track_mc_veh_f64_host / scvx_track_mc_nav_veh_f64_host: every output bitwise the _q call's (uploaded
    draws) and the _rng call's (device draws); m None: truth-fed, else flown on an estimate with m measurement rows"""
    c, po, dyn, par, x, u, s, d, L, S0 = _plans(model, aero_tables)
    _null_veh_is_the_plain_call("%s m %s" % (model, m), monkeypatch, c, x, u, s, L, S0, m, (1, 3), (1, 65, 130), 10)
    c.close()


def _null_veh_is_the_plain_call(tag, monkeypatch, c, x, u, s, L, S0, m, Bs, Ss, nsub):
    from successiveconvexification_amd.dynamics import track_mc_batch
    nav = None if m is None else (0.25 * S0, *_model(m, x[0, 0]))
    names = OLD if m is None else OLD_NAV
    dn = ("flights", "xland", "dx0", "pathv") + (() if m is None else ("navfed", "navK"))
    zero = (np.zeros(6), np.zeros(6))
    n = 0
    for B in Bs:
        for S in Ss:
            for rng in ("host", "device"):
                nb = None if nav is None else (nav[0][:B],) + nav[1:]
                kw = dict(seed=11, w=W if S != 65 else None, nsub=nsub, clamp=S == 130, tol=1e-6, quantiles=PROBS, per_node=True, dense=dn,
                          nav=nb, rng=rng)
                old = track_mc_batch(c, x[:B], u[:B], s[:B], L[:B], S0[:B], S, **kw)
                with monkeypatch.context() as mp:
                    _null_veh(mp, c._L)
                    new = track_mc_batch(c, x[:B], u[:B], s[:B], L[:B], S0[:B], S, vehicle=zero, **kw)
                same = {nm: _eq(getattr(old, nm), getattr(new, nm)) for nm in names}
                assert all(same.values()), (tag, B, S, rng, same)
                n += 1
    print("%s: %d calls with veh = NULL through the new entry point bitwise the _q / _rng call" % (tag, n))


@pytest.mark.parametrize("model", ["exo", "aero+fins+torque"])
def test_zero_errors_agree_with_the_plain_call(model, aero_tables):
    """mu = sp = 0 flies the ACT instantiations with theta = 0: within K 1e-12 A_cl of the plain call (A_cl of the reference chain on
    plan 0) at S = 1, 65 and 130; whether it is bitwise is printed, not asserted"""
    from successiveconvexification_amd.dynamics import track_mc_batch
    from successiveconvexification_amd.montecarlo import handover_factor, mc_draws
    c, po, dyn, par, x, u, s, d, L, S0 = _plans(model, aero_tables)
    K = po.K
    xi0, eta = mc_draws(5, K, 3, noise=True)
    A = mr.sensitivity(dyn, po, x[0], u[0], s[0], L[0], xi0 @ handover_factor(S0[0]).T, 10, 1e-9, 0, eta * np.sqrt(W), par=par)
    bound = K * 1e-12 * A
    H, rm = _model(3, x[0, 0])
    for S in (1, 65, 130):     # a block of one lane, a block and a lane, two blocks and a tail
        for nav in (None, (0.25 * S0[:1], H, rm)):
            for rng in ("host", "device"):
                kw = dict(seed=3, w=W, nsub=10, clamp=True, dense=("flights", "xland", "dx0"), nav=nav, rng=rng)
                plain = track_mc_batch(c, x[:1], u[:1], s[:1], L[:1], S0[:1], S, **kw)
                kw["dense"] = kw["dense"] + ("theta",)
                zero = track_mc_batch(c, x[:1], u[:1], s[:1], L[:1], S0[:1], S, vehicle=(np.zeros(6), np.zeros(6)), **kw)
                err = float(np.abs(zero.xland - plain.xland).max())
                fin = np.isfinite(plain.flights)
                ferr = float(np.abs(zero.flights[fin] - plain.flights[fin]).max())
                print("%s S %d nav %s rng %s: mu = sp = 0 against the plain call: xland %.3e, flights %.3e (bound %.3e, A_cl %.3f); bitwise: xland %s, "
                      "flights %s, report %s" % (model, S, nav is not None, rng, err, ferr, bound, A, _same(zero.xland, plain.xland),
                                                 _same(zero.flights, plain.flights), _same(zero.raw, plain.raw)))
                assert not zero.theta.any() and zero.theta.shape == (1, S, 6)
                assert _same(zero.dx0, plain.dx0)
                assert err <= bound and np.array_equal(fin, np.isfinite(zero.flights))
    c.close()


def _parity(tag, c, po, dyn, par, x, u, s, L, S0, b, nsub, clamp, noise, nav=None, zero_mean=True):
    """flights 0..5 with one component each, 6..7 with all six (one launch, by zeta; skipped without zero_mean), then all six with a
    non-zero mu (a second launch), against the CPU chain"""
    from successiveconvexification_amd.dynamics import track_mc_batch
    from successiveconvexification_amd.montecarlo import handover_factor, mc_draws, mc_nav_draws
    import track_reference as tr
    K, S = po.K, 8
    sl = slice(b, b + 1)
    xi0, eta = mc_draws(S, K, 41, noise=noise)
    zeta = np.zeros((S, 6))
    zeta[:6] = np.diag([1.0, -1.0, 1.0, -1.0, 1.0, -1.0])
    zeta[6:] = np.random.default_rng(8).standard_normal((2, 6))
    dx0 = xi0 @ handover_factor(S0[b]).T
    imp = eta * np.sqrt(W) if noise else None
    worst = 0.0
    for mu, sp in ((_veh(c),) if zero_mean else ()) + (_veh(c, mu=MU_ALL),):
        dn = ("flights", "xland", "dx0", "theta") + (("navfed",) if nav else ())
        draws = (xi0, eta) + (mc_nav_draws(S, K, nav[1].shape[0], 41) if nav else ())
        nb = None if nav is None else (nav[0][sl],) + nav[1:]
        kw = dict(w=W if noise else None, nsub=nsub, clamp=clamp, dense=dn, draws=draws, nav=nb)
        dev = track_mc_batch(c, x[sl], u[sl], s[sl], L[sl], S0[sl], S, vehicle=(mu, sp, zeta), **kw)
        theta = vr.fma(sp[None, :], zeta, mu[None, :])
        assert _same(dev.theta[0], theta), (tag, np.abs(dev.theta[0] - theta).max())
        fed = dev.navfed[0] if nav else None
        if nav:   # the recursion of the estimate's error does not see the vehicle
            assert _same(fed, track_mc_batch(c, x[sl], u[sl], s[sl], L[sl], S0[sl], S, **dict(kw, dense=("navfed",))).navfed[0])
        fl = tr.CLAMP if clamp else 0
        ref, xref, _, cmd = vr.fly_plan(dyn, po, x[b], u[b], s[b], L[b], dx0, nsub, theta, fl, imp, par, fed)
        A = vr.sensitivity(dyn, po, x[b], u[b], s[b], L[b], dx0, nsub, theta, 1e-9, fl, imp, draws=1, par=par, nav=fed)
        bound = K * 1e-12 * A
        err = np.abs(dev.xland[0] - xref[:, -1]).max(axis=1)
        moved = np.abs(xref[:, -1] - vr.fly_plan(dyn, po, x[b], u[b], s[b], L[b], dx0, nsub, np.zeros((S, 6)), fl, imp, par, fed)[1][:, -1]).max(axis=1)
        print("%s plan %d clamp %s noise %s nav %s mu %s: A_cl %.3f, bound %.3e, xland error per flight %s; the errors moved the landing "
              "by %s" % (tag, b, clamp, noise, nav is not None, bool(mu.any()), A, bound, " ".join("%.1e" % v for v in err),
                         " ".join("%.1e" % v for v in moved)))
        assert err.max() <= bound
        live = [i for i in range(6) if sp[i] > 0.0]
        assert np.all(moved[live] > 10.0 * bound)                    # every component the model has is felt, above the bound
        _compare("%s plan %d" % (tag, b), dev.flights[0], ref, bound, po)
        worst = max(worst, float(err.max() / bound))
    return worst


@pytest.mark.parametrize("model", ["exo", "aero+fins"])
def test_against_the_cpu_chain_at_k_50(model, aero_tables):
    """the golden plans, and the unconverged aero + fins plans (the C oracle: ISP and AERO take one parameter set per flight, which the
    torque model's reference is too slow for at this horizon -- it is checked at K = 3 below)"""
    c, po, dyn, par, x, u, s, d, L_dev, S0 = _plans(model, aero_tables)
    import track_reference as tr
    L, _ = tr.gains(d, po.K)                                        # the REFERENCE's gains, fed to both sides
    H, rm = _model(3, x[0, 0])
    for clamp, noise in ((False, False), (True, True)) + (((True, False), (False, True)) if model == "exo" else ()):
        _parity(model, c, po, dyn, par, x, u, s, L, S0, 0, 10, clamp, noise)
    _parity(model, c, po, dyn, par, x, u, s, L, S0, 1, 10, True, True, nav=(0.25 * S0, H, rm))
    c.close()


@pytest.mark.parametrize("model", ["exo", "aero+fins", "aero+fins+torque"])
def test_against_the_cpu_chain_at_k_3(model, aero_tables):
    import horizon_cases as hc
    import track_reference as tr
    from successiveconvexification_amd.dynamics import IntegratorCache, linearize_batch
    pp, po, dyn, par, x, u, s = hc.case(model, 3, aero_tables)
    c = IntegratorCache(pp, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (po.K + 1))
    L, _ = tr.gains(d, po.K)
    S0 = np.stack([cr.handover_s0(x[b, 0])[0] for b in range(x.shape[0])])
    H, rm = _model(3, x[0, 0])
    if "torque" in model:   # its reference takes a parameter set per flight through torch: one launch, every component and a mean
        _parity("%s K = 3" % model, c, po, dyn, par, x, u, s, L, S0, 2, 10, True, True, zero_mean=False)
    else:
        for b in (0, 2):
            _parity("%s K = 3" % model, c, po, dyn, par, x, u, s, L, S0, b, 10, b == 2, b == 0)
        _parity("%s K = 3" % model, c, po, dyn, par, x, u, s, L, S0, 1, 10, False, True, nav=(0.25 * S0, H, rm))
    c.close()


@pytest.mark.parametrize("m", [None, 3])
@pytest.mark.parametrize("model", ["exo", "aero+fins+torque"])
def test_device_draws(model, m, aero_tables):
    """sp a power of two and mu = 0: the rng call is bitwise the uploaded-draw call fed the dump and zeta = theta / sp; the dumped theta
    against the longdouble reference of stream 8; a shard is rows of the whole; row b of an independent call is the B = 1 call on its
    own stream"""
    from successiveconvexification_amd.dynamics import track_mc_batch
    from successiveconvexification_amd.montecarlo import mc_vehicle_draws_device
    c, po, dyn, par, x, u, s, d, L, S0 = _plans(model, aero_tables)
    K, seed = po.K, 2 ** 63 + 5
    mu, sp = _veh(c, sp=[2.0 ** -9, 2.0 ** -10, 2.0 ** -10, 2.0 ** -8, 2.0 ** -6, 2.0 ** -7])
    live = sp > 0.0
    nav = None if m is None else (0.25 * S0, *_model(m, x[0, 0]))
    names = (OLD if m is None else OLD_NAV) + ("theta",)
    dn = ("flights", "xland", "dx0", "pathv", "theta") + (() if m is None else ("navfed", "navK"))
    for B in (1, 3):
        nb = None if nav is None else (nav[0][:B],) + nav[1:]
        for S in (1, 65, 130):
            kw = dict(w=W, nsub=10, clamp=True, tol=1e-6, quantiles=PROBS, per_node=True, dense=dn, nav=nb)
            new = track_mc_batch(c, x[:B], u[:B], s[:B], L[:B], S0[:B], S, seed=seed, rng="device", vehicle=(mu, sp), **kw)
            assert _same(new.theta[0], new.theta[B - 1]) and not new.theta[..., ~live].any()       # shared draws
            zeta = np.where(live, new.theta[0] / np.where(live, sp, 1.0), 0.0)
            xi0, eta, xin, nud = _dump(c, S, K, seed, True, m or 0)
            old = track_mc_batch(c, x[:B], u[:B], s[:B], L[:B], S0[:B], S, draws=(xi0, eta) + ((xin, nud) if nav else ()),
                                 vehicle=(mu, sp, zeta), **kw)
            same = {nm: _eq(getattr(old, nm), getattr(new, nm)) for nm in names}
            assert all(same.values()), (model, m, B, S, same)
            ld = np.stack([rr.normals(rr.words(seed, 8, 0, i, 2)).reshape(-1)[:6] for i in range(S)])
            tw = mc_vehicle_draws_device(S, seed)
            own = np.abs(tw.astype(np.longdouble) - ld)
            ulp = np.spacing(np.abs(ld).astype(np.float64)).astype(np.longdouble)
            err = np.abs(zeta.astype(np.longdouble) - ld)
            ratio = float((err / (8 * own + 4 * ulp))[:, live].max())
            if B == 3 and S == 130:
                print("%s m %s: theta / sp against the longdouble reference of stream 8: %.2f ulp, error / (8 x twin's + 4 ulp) %.3f"
                      % (model, m, float((err / ulp)[:, live].max()), ratio))
            assert np.all((err <= 8 * own + 4 * ulp)[:, live]), ratio
    # a shard; an independent row
    kw = dict(seed=seed, w=W, nsub=10, rng="device", vehicle=(mu, sp), dense=("xland", "theta"),
              nav=None if nav is None else (nav[0][:3],) + nav[1:])
    for ind in (False, True):
        whole = track_mc_batch(c, x[:3], u[:3], s[:3], L[:3], S0[:3], 130, independent=ind, **kw)
        part = track_mc_batch(c, x[:3], u[:3], s[:3], L[:3], S0[:3], 66, sample_lo=64, independent=ind, **kw)
        assert _same(part.xland, whole.xland[:, 64:130]) and _same(part.theta, whole.theta[:, 64:130]), ind
    for b in range(3):
        sl = slice(b, b + 1)
        one = track_mc_batch(c, x[sl], u[sl], s[sl], L[sl], S0[sl], 130, independent=True, plan_lo=b,
                             **dict(kw, nav=None if nav is None else (nav[0][sl],) + nav[1:]))
        assert _same(one.xland[0], whole.xland[b]) and _same(one.theta[0], whole.theta[b]), b
    assert not _same(whole.theta[0], whole.theta[1])
    ld = np.stack([rr.normals(rr.words(seed, 8, 1 + 2, i, 2)).reshape(-1)[:6] for i in range(130)])     # plan 2's own stream
    z2 = whole.theta[2][:, live] / sp[live]
    assert np.abs(z2 - ld[:, live].astype(np.float64)).max() < 1e-12
    c.close()


def test_sensitivity_and_pooled_statistics_within_six_standard_errors():
    """Golden plan 0 replicated 8 times, independent draws, S = 1,024, THRUST, MIS_Y and MIS_Z dispersed with the CPU anchor's sp: the
    covariance pooled over the 8,192 flights against the device's own scvx_cov_propagate_f64 plus J diag(sp^2) J', J from
    vehicle_sensitivity_batch; J itself against the CPU's central differences"""
    from oracle import dynamics as od
    from test_mc_vehicle_cpu import H_FD, anchor_case
    from successiveconvexification_amd.dynamics import (IntegratorCache, cov_propagate_batch, linearize_batch, track_gains_batch,
                                                          track_mc_batch, vehicle_sensitivity_batch)
    from successiveconvexification_amd.montecarlo import vehicle_budget
    B, S = 8, 1024
    p, par, x, u, s, d_ref, L_ref, S0, covK_ref, J_ref = anchor_case()
    c = IntegratorCache(_golden()[0], npts=10)
    sl = slice(0, 1)
    _, d = linearize_batch(c, x[sl], u[sl], s[sl], 1.0 / (p.K + 1))
    L = track_gains_batch(c, d)
    # J: the device under the REFERENCE's gains against the CPU chain under the same gains
    Jd = vehicle_sensitivity_batch(c, x[sl], u[sl], s[sl], L_ref[sl], h=H_FD)[0]
    th = np.zeros((8, 6))
    for i in range(4):
        th[2 * i, i], th[2 * i + 1, i] = H_FD, -H_FD
    A = vr.sensitivity(od, p, x[0], u[0], s[0], L_ref[0], np.zeros((8, 14)), 10, th, 1e-9, par=par)
    bound = p.K * 1e-12 * A / H_FD
    err = float(np.abs(Jd - J_ref).max())
    print("J = dx_K/dtheta, device against the CPU's central differences (h = 2^-10): |J| per component %s, largest difference %.3e, "
          "bound K 1e-12 A_cl / h = %.3e (A_cl %.3f)" % (np.linalg.norm(Jd, axis=0), err, bound, A))
    assert not Jd[:, 4:].any() and err <= bound
    # statistics under the device's own gains
    J = vehicle_sensitivity_batch(c, x[sl], u[sl], s[sl], L, h=H_FD)[0]
    covK = cov_propagate_batch(c, x[sl], u[sl], d, L, S0[None], None, dense=("covK",)).covK[0][:14, :14]
    sp = np.zeros(6)
    sp[:3] = vr.equal_share_sp(J_ref, (0, 1, 2), float(np.trace(covK_ref)))
    rep8 = lambda a: np.repeat(np.asarray(a)[:1], B, axis=0)   # noqa: E731
    r = track_mc_batch(c, rep8(x), rep8(u), rep8(s), rep8(L), S0, S, seed=0, nsub=10, rng="device", independent=True, dense=("xland",),
                       vehicle=(np.zeros(6), sp))
    xcov = np.cov((r.xland - x[0, -1]).reshape(B * S, 14), rowvar=False)
    worst, over = mr.se_check(xcov, vehicle_budget(J, sp, covK)["cov"], B * S)
    worst0, over0 = mr.se_check(xcov, covK, B * S)
    print("8 x 1,024 independent flights pooled, sp %.3e: worst entry %.2f standard errors of Sigma_K + J diag(sp^2) J', %d over 6; against "
          "Sigma_K alone %.2f, %d over 6" % (sp[0], worst, over, worst0, over0))
    assert r.N_BAD.sum() == 0 and over == 0, (worst, over)
    assert over0 > 0
    c.close()


def test_aero_sensitivity_and_pooled_statistics_within_six_standard_errors(aero_tables):
    """The same for AERO on the CPU anchor's aerodynamic plan (test_mc_vehicle_cpu.aero_anchor_case: K = 3, aero + fins, a 1 sigma of
    0.1 on force_scalar beside a handover of the same share), replicated 8 times, independent draws, S = 1,024, under the reference's
    gains: pooled covariance against the device's own scvx_cov_propagate_f64 plus J diag(sp^2) J', J from vehicle_sensitivity_batch;
    its AERO column against the CPU's central differences"""
    import horizon_cases as hc
    from test_mc_vehicle_cpu import AERO_K, AERO_SP, H_FD, aero_anchor_case
    from successiveconvexification_amd.dynamics import (IntegratorCache, cov_propagate_batch, linearize_batch, track_mc_batch,
                                                          vehicle_sensitivity_batch)
    from successiveconvexification_amd.montecarlo import vehicle_budget
    B, S = 8, 1024
    po, par, x, u, s, d_ref, L, S0, covK_ref, J_ref = aero_anchor_case(aero_tables)
    pp, _, dyn, _ = hc.problems("aero+fins", AERO_K, aero_tables)
    c = IntegratorCache(pp, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (AERO_K + 1))
    J = vehicle_sensitivity_batch(c, x, u, s, L, h=H_FD)[0]
    th = np.zeros((2, 6))
    th[0, vr.AERO], th[1, vr.AERO] = H_FD, -H_FD
    A = vr.sensitivity(dyn, po, x[0], u[0], s[0], L[0], np.zeros((2, 14)), 10, th, 1e-9, par=par)
    bound = AERO_K * 1e-12 * A / H_FD
    err = float(np.abs(J[:, vr.AERO] - J_ref[:, vr.AERO]).max())
    print("dx_K/dAERO, device against the CPU's central differences (h = 2^-10): norm %.3e, largest difference %.3e, bound "
          "K 1e-12 A_cl / h = %.3e (A_cl %.3f)" % (np.linalg.norm(J[:, vr.AERO]), err, bound, A))
    assert err <= bound
    covK = cov_propagate_batch(c, x, u, d, L, S0[None], None, dense=("covK",)).covK[0][:14, :14]
    sp = np.zeros(6)
    sp[vr.AERO] = AERO_SP
    rep8 = lambda a: np.repeat(np.asarray(a)[:1], B, axis=0)   # noqa: E731
    r = track_mc_batch(c, rep8(x), rep8(u), rep8(s), rep8(L), S0, S, seed=0, nsub=10, rng="device", independent=True, dense=("xland",),
                       vehicle=(np.zeros(6), sp))
    xcov = np.cov((r.xland - x[0, -1]).reshape(B * S, 14), rowvar=False)
    worst, over = mr.se_check(xcov, vehicle_budget(J, sp, covK)["cov"], B * S)
    worst0, over0 = mr.se_check(xcov, covK, B * S)
    print("AERO, 8 x 1,024 independent flights pooled, sp %.1e, trace of Sigma_K %.3e: worst entry %.2f standard errors of Sigma_K + "
          "J diag(sp^2) J', %d over 6; against Sigma_K alone %.2f, %d over 6" % (AERO_SP, np.trace(covK), worst, over, worst0, over0))
    assert r.N_BAD.sum() == 0 and over == 0, (worst, over)
    assert over0 > 0
    c.close()


def test_batch_calls_float_tiles_and_back_offs():
    """ScvxBatch.track_mc(vehicle=) is the context-level call (also flown on an estimate, also on float tiles: against the batch call fed
    the dump); margins_from_mc(vehicle=) and robustify(mc=dict(vehicle=)) are the manual sequence of calls, bit for bit"""
    import bench
    from test_gpu_flight import _flyable
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache, track_mc_batch
    from successiveconvexification_amd.montecarlo import margins_from_quantiles, vehicle_errors
    pp, po = _flyable()
    B = 3
    c = IntegratorCache(pp, npts=10)
    b, b2 = (ScvxBatch(c, B).init(bench.disperse_ics(pp, 0, B, 7)) for _ in range(2))
    b.solve(), b2.solve()
    x, u, s = b.trajectory()
    assert all(_same(a0, a1) for a0, a1 in zip((x, u, s), b2.trajectory()))
    sd = np.zeros(14)
    sd[1:7] = 1e-3 * np.abs(x[0, 0, 1:7])
    sd[7:] = 1e-3
    w = np.full(14, 1e-9)
    H, rm = _model(3, x[0, 0])
    nav = (0.25 * np.diag(sd * sd), H, rm)
    veh = vehicle_errors(thrust=2e-3, misalign=1e-3, isp=3e-3)
    for rng in ("host", "device"):
        kw = dict(seed=4, w=w, clamp=True, tol=1e-6, quantiles=PROBS, per_node=True, rng=rng, sample_lo=64, vehicle=veh)
        rb = b.track_mc(sd, samples=70, dense=("flights", "pathv", "theta"), **kw)
        rh = track_mc_batch(c, x, u, s, b.track_gains(), sd, 70, nsub=10, dense=("flights", "pathv", "theta"), **kw)
        assert all(_same(getattr(rb, n), getattr(rh, n)) for n in ("raw", "xcov", "flights", "q", "pathq", "pathv", "theta")), rng
        nb = b.track_mc(sd, samples=70, nav=nav, dense=("pathv", "navfed", "theta"), **kw)
        nh = track_mc_batch(c, x, u, s, b.track_gains(), sd, 70, nsub=10, nav=nav, dense=("pathv", "navfed", "theta"), **kw)
        assert all(_same(getattr(nb, n), getattr(nh, n)) for n in ("raw", "navraw", "navfed", "q", "pathq", "pathv", "theta")), rng
        plain = b.track_mc(sd, samples=70, dense=("flights",), **dict(kw, vehicle=None))
        assert not _same(plain.flights, rb.flights) and rb.theta.shape == (B, 70, 6)
    # float tiles: the device-draw batch call against the batch call fed the dump
    b.set_linearization_f32(True)
    xi0, eta, xin, nud = _dump(c, 70, pp.K, 4, True, 3)
    k0 = dict(seed=4, w=w, clamp=True, tol=1e-6, quantiles=PROBS, per_node=True, dense=("flights", "xland", "dx0", "navfed", "navK", "pathv", "theta"))
    vp = (np.zeros(6), np.array([2.0 ** -9, 2.0 ** -10, 2.0 ** -10, 2.0 ** -8, 0.0, 0.0]))
    f_new = b.track_mc(sd, samples=70, nav=nav, rng="device", vehicle=vp, **k0)
    zeta = np.where(vp[1] > 0, f_new.theta[0] / np.where(vp[1] > 0, vp[1], 1.0), 0.0)
    f_old = b.track_mc(sd, nav=nav, draws=(xi0, eta, xin, nud), vehicle=vp + (zeta,), **k0)
    same = {n: _same(getattr(f_old, n), getattr(f_new, n)) for n in OLD_NAV + ("theta",)}
    print("float tiles through the batch call with vehicle errors: bitwise %s" % same)
    assert all(same.values()), same
    b.set_linearization_f32(False)
    # the back-offs: margins_from_mc is track_mc + margins_from_quantiles + the two setters
    for nv in (None, nav):
        b.set_thrust_margins(None, None).set_path_margins()
        rep, lo, hi, pm = b.margins_from_mc(sd, samples=256, seed=3, nav=nv, rng="device", independent=True, vehicle=veh)
        man = b.track_mc(sd, samples=256, seed=3, nav=nv, rng="device", independent=True, vehicle=veh, quantiles=(1.0 - 0.99865, 0.99865),
                         per_node=True)
        assert _same(man.pathq, rep.pathq) and _same(man.raw, rep.raw)
        want = margins_from_quantiles(pp, x, u, man.pathq[..., 0], man.pathq[..., 1], "all", 0.25)
        got = b.thrust_margins() + (b.path_margins(),)
        for a0, a1, a2 in zip(got, want, (lo, hi, pm)):
            assert np.array_equal(a0, a1) and np.array_equal(a0, a2)
        none = b.track_mc(sd, samples=256, seed=3, nav=nv, rng="device", independent=True, quantiles=(1.0 - 0.99865, 0.99865), per_node=True)
        assert not _same(none.pathq, rep.pathq)                                   # the vehicle errors reach the quantiles
    # robustify(mc=dict(vehicle=)): one round is margins_from_mc, replan, solve
    mc = dict(p=0.99865, samples=128, rng="device", independent=True, vehicle=veh)
    b.set_thrust_margins(None, None).set_path_margins()
    out = b.robustify(sd, mc=mc)
    xr, ur, sr = b.trajectory()
    _, lo, hi, _ = b2.margins_from_mc(sd, constraints=("thrust",), **mc)      # a second batch, solved alike and never touched since
    b2.replan()
    man = b2.solve()
    xm, um, sm = b2.trajectory()
    print("robustify(mc=dict(vehicle=)): status %s, bitwise the manual sequence: x %s u %s" % (out[0], _same(xr, xm), _same(ur, um)))
    assert _same(xr, xm) and _same(ur, um) and _same(sr, sm) and _same(out[4], lo) and _same(out[5], hi)
    assert all(_same(a0, a1) for a0, a1 in zip(out[:4], man))
    b.close(), b2.close(), c.close()


def test_rocketland_track_mc_with_vehicle_errors():
    from successiveconvexification_amd import rocketland as rl, sample_problems as sp
    from successiveconvexification_amd.dynamics import IntegratorCache
    from successiveconvexification_amd.montecarlo import vehicle_errors
    p = sp.base_prob_scaled
    c = IntegratorCache(p, npts=10)
    it = rl.create_initial(p, c)
    it, _, _ = rl.solve_step(it, c)
    sd = np.full(14, 1e-4)
    sd[0] = 0.0
    veh = vehicle_errors(thrust=1e-3, misalign=1e-3)
    a = rl.track_mc(it, c, sd, samples=65, seed=2, w=1e-10, rng="device", dense=("xland", "theta"), vehicle=veh)
    a2 = rl.track_mc(it, c, sd, samples=65, seed=2, w=1e-10, rng="device", dense=("xland", "theta"), vehicle=veh)
    h = rl.track_mc(it, c, sd, samples=65, seed=2, w=1e-10, rng="device", dense=("xland",))
    assert _same(a.xland, a2.xland) and not _same(a.xland, h.xland) and a.S[0] == 65 and a.theta.shape == (1, 65, 6) and h.theta is None
    c.close()


def test_argument_errors(aero_tables):
    from successiveconvexification_amd import _lib
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache, linearize_batch, track_gains_batch, track_mc_batch
    pp, po, x, u, s = _golden()
    c = IntegratorCache(pp, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (po.K + 1))
    gain = track_gains_batch(c, d)
    L, h, K, S = c._L, c.handle, pp.K, 4
    _dp = C.POINTER(C.c_double)
    ptr = lambda a: None if a is None else a.ctypes.data_as(_dp)   # noqa: E731
    C0 = np.ascontiguousarray(np.stack([np.eye(14) * 1e-3] * 2))
    rep, xm, xc = np.full((2, 48), 7.0), np.full((2, 14), 7.0), np.full((2, 14, 14), 7.0)
    jm, jc, nv = np.full((2, 28), 7.0), np.full((2, 28, 28), 7.0), np.full((2, 8), 7.0)
    xi0, zeta, theta = np.zeros((S, 14)), np.zeros((S, 6)), np.full((2, S, 6), 7.0)
    sw = np.full(14, 1e-4)
    err = lambda: L.scvx_last_error(h).decode()   # noqa: E731
    rg = _lib.ScvxMcRng(1, 0, 0, 0, 0)
    b = ScvxBatch(c, 2).init(None)
    b.set_trajectory(x, u, s)
    q, r, qf = np.ones(14), np.ones(3), np.full(14, 100.0)

    def vehicle(mu=None, sp=None, reserved=(0, 0)):
        return _lib.ScvxMcVehicle((C.c_double * 6)(*(mu or [0.0] * 6)), (C.c_double * 6)(*(sp or [0.0] * 6)), (C.c_int32 * 2)(*reserved))

    def calls(veh, rng=None, noise=0, xi=xi0, eta=None, xin=xi0, zt=zeta, th=theta, res=None):
        """the four entry points; res (the `reserved` argument): the two truth-fed ones, which have it"""
        v = None if veh is None else C.byref(veh)
        p = None if rng is None else C.byref(rng)
        qt = [0, None, None, None, None]
        tail = [p, noise, v, ptr(zt), ptr(th)]
        sww = ptr(sw) if (eta is not None or noise) else None
        yield L.scvx_track_mc_veh_f64_host(h, 2, K, S, ptr(x), ptr(u), ptr(s), ptr(gain), ptr(C0), ptr(xi), ptr(eta), sww, res, 10, 0, 0.0,
                                           ptr(rep), ptr(xm), ptr(xc), None, None, None, *qt, *tail)
        if res is None:
            yield L.scvx_track_mc_nav_veh_f64_host(h, 2, K, S, ptr(x), ptr(u), ptr(s), ptr(gain), ptr(C0), ptr(xi), ptr(eta), sww, ptr(d),
                                                   None, ptr(C0), ptr(xin), None, 0, None, None, 10, 0, 0.0, ptr(rep), ptr(xm), ptr(xc),
                                                   ptr(jm), ptr(jc), ptr(nv), None, None, None, None, None, *qt, *tail)
        yield L.scvx_batch_track_mc_veh(b.handle, ptr(q), ptr(r), ptr(qf), S, ptr(C0), ptr(xi), ptr(eta), sww, res, 10, 0, 0.0, ptr(rep),
                                        ptr(xm), ptr(xc), None, None, None, *qt, *tail)
        if res is None:
            yield L.scvx_batch_track_mc_nav_veh(b.handle, ptr(q), ptr(r), ptr(qf), S, ptr(C0), ptr(xi), ptr(eta), sww, ptr(C0), ptr(C0),
                                                ptr(xin), None, 0, None, None, 10, 0, 0.0, ptr(rep), ptr(xm), ptr(xc), ptr(jm), ptr(jc),
                                                ptr(nv), None, None, None, None, None, *qt, *tail)

    inf, nan = float("inf"), float("nan")
    one = lambda i, v: [v if j == i else 0.0 for j in range(6)]   # noqa: E731
    bad = [(dict(veh=vehicle(sp=one(4, 1e-3))), "AERO"), (dict(veh=vehicle(mu=one(4, 1e-3))), "AERO"),
           (dict(veh=vehicle(sp=one(5, 1e-3))), "FIN"), (dict(veh=vehicle(mu=one(5, -1e-3))), "FIN"),
           (dict(veh=vehicle(sp=one(0, -1e-3))), "sp"), (dict(veh=vehicle(sp=one(2, inf))), "sp"), (dict(veh=vehicle(sp=one(3, nan))), "sp"),
           (dict(veh=vehicle(mu=one(1, nan))), "mu"), (dict(veh=vehicle(mu=one(0, inf))), "mu"),
           (dict(veh=vehicle(reserved=(0, 1))), "reserved"), (dict(veh=vehicle(reserved=(2, 0))), "reserved"),
           (dict(veh=vehicle(sp=one(0, 1e-3)), zt=None), "zeta"),                               # sp > 0 without zeta or rng
           (dict(veh=vehicle(), rng=rg), "NULL"), (dict(veh=vehicle(), rng=rg, xi=None, xin=None), "NULL"),      # rng with uploaded draws
           (dict(veh=vehicle(), rng=rg, xi=None, xin=None, zt=None, eta=np.zeros((S, K, 14))), "NULL"),
           (dict(veh=vehicle(), noise=1), "noise"),                                             # noise without rng
           (dict(veh=None), "without veh"), (dict(veh=None, zt=None), "without veh"),            # zeta / theta without veh
           (dict(veh=vehicle(), res=C.c_void_p(1)), "reserved")]
    for kw, word in bad:
        for i, rc in enumerate(calls(**kw)):
            assert rc == -1 and word in err(), (word, i, rc, err())
    assert np.all(rep == 7.0) and np.all(theta == 7.0) and np.all(jc == 7.0)         # nothing ran
    good = [dict(veh=vehicle(sp=one(0, 1e-3))), dict(veh=vehicle(mu=one(3, 1e-3)), zt=None), dict(veh=None, zt=None, th=None),
            dict(veh=vehicle(sp=one(1, 1e-3)), rng=rg, xi=None, xin=None, zt=None, noise=1),
            dict(veh=None, rng=rg, xi=None, xin=None, zt=None, th=None)]
    for kw in good:
        for i, rc in enumerate(calls(**kw)):
            assert rc == 0, (kw, i, rc, err())
    assert np.all(rep[:, 45] == S) and np.isfinite(theta).all()
    # the old entry points still refuse `reserved`
    assert L.scvx_track_mc_f64_host(h, 2, K, S, ptr(x), ptr(u), ptr(s), ptr(gain), ptr(C0), ptr(xi0), None, None, C.c_void_p(1), 10, 0, 0.0,
                                    ptr(rep), ptr(xm), ptr(xc), None, None, None) == -1 and "reserved" in err()
    # AERO and FIN are accepted where the model has them
    cf, *_ = _plans("aero+fins+torque", aero_tables)
    assert _veh(cf)[1][4] > 0 and _veh(cf)[1][5] > 0 and _veh(c)[1][4] == 0
    cf.close()
    with pytest.raises(ValueError):
        track_mc_batch(c, x, u, s, gain, np.full(14, 1e-3), 4, dense=("theta",))
    with pytest.raises(ValueError):
        track_mc_batch(c, x, u, s, gain, np.full(14, 1e-3), 4, rng="device", vehicle=(np.zeros(6), np.zeros(6), np.zeros((4, 6))))
    with pytest.raises(_lib.ScvxError):
        track_mc_batch(c, x, u, s, gain, np.full(14, 1e-3), 4, vehicle=(np.zeros(6), np.array([0, 0, 0, 0, 1e-3, 0.0])))
    b.close(), c.close()
