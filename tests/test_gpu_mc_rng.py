"""The sampled dispersion with the draws made on the device (scvx_mc_draws_f64, scvx_track_mc_rng_f64, scvx_track_mc_nav_rng_f64, their
batch forms; rng="device" in Python) on the MI355X.

Bounds, none of them taken from the device:
  * the dumped draws against the longdouble reference (tests/mc_rng_reference.py: numpy's own Philox words, Box-Muller in longdouble):
    per entry, 8 x the distance of the float64 numpy twin (montecarlo.mc_draws_device) from that reference, recomputed here, plus 4 ulp
    of the entry -- test_gpu_mc_nav.py's rule for navfed, entry by entry.  Two launches bit for bit.
  * a fused call against the old call fed the dump, and a row of an independent call against the old call at B = 1: bit for bit.
  * sharding: rows of the whole, bit for bit.
  * statistics: six standard errors per entry (mc_reference.se_check), pooled over B S = 8,192 independent flights.
  * back-offs: exactly montecarlo.margins_from_quantiles of the report's own pathq.
Every comparison prints its figures before it asserts.
"""
import ctypes as C

import numpy as np
import pytest

import cov_reference as cr
import mc_nav_reference as mn
import mc_reference as mr
import mc_rng_reference as rr
from test_gpu_mc import _golden, _same
from test_gpu_mc_nav import _model
from test_gpu_mc_quantiles import _plans

pytestmark = pytest.mark.gpu

SEED = 2 ** 63 + 5
PROBS = (0.0, 0.5, 0.99, 1.0)
OLD = ("raw", "xmean", "xcov", "flights", "xland", "dx0", "q", "pathq", "pathv")
OLD_NAV = OLD + ("jmean", "jcov", "navraw", "navfed", "navK")
_REF = {}


def _eq(a, b):
    return (a is None and b is None) or (a is not None and b is not None and _same(a, b))


def _reference(s_lo, K=50):
    """the longdouble reference and the float64 twin of the largest case (P = 3, S = 130, K nodes), both streams: every smaller case is a
    slice of it -- the layout is random access by definition"""
    if (s_lo, K) not in _REF:
        from successiveconvexification_amd.montecarlo import mc_draws_device, mc_nav_draws_device
        out = {}
        for plans in (None, (0, 1, 2)):
            ld = [rr.draws(SEED, st, 130, K, s_lo, plans) for st in (rr.STREAM_TRUTH, rr.STREAM_NAV)]
            tw = mc_draws_device(130, K, SEED, noise=True, lo=s_lo, plans=plans) + mc_nav_draws_device(130, K, 14, SEED, lo=s_lo, plans=plans)
            out[1 if plans is None else 3] = ((ld[0][0], ld[0][1], ld[1][0], ld[1][1]), tuple(a[None] if plans is None else a for a in tw))
        _REF[(s_lo, K)] = out
    return _REF[(s_lo, K)]


def _dump_against_the_reference(c, ld, tw, s_lo, P, S, K):
    """one dump of P plans, S samples and K nodes against the slices of the reference ld and the twin tw: (the dump, largest error /
    (8 x the twin's own distance + 4 ulp))"""
    from successiveconvexification_amd.dynamics import mc_draws_device_batch
    d = mc_draws_device_batch(c, S, K=K, seed=SEED, sample_lo=s_lo, plans=None if P == 1 else P)
    again = mc_draws_device_batch(c, S, K=K, seed=SEED, sample_lo=s_lo, plans=None if P == 1 else P)
    worst = 0.0
    for i, n in enumerate(("xi0", "eta", "xin", "nud")):
        dev = d[n][None] if P == 1 else d[n]
        sl = (slice(None), slice(0, S)) + ((slice(0, K),) if i % 2 else ())
        r, t = ld[i][sl], tw[i][sl]
        assert dev.shape == r.shape == t.shape, (n, dev.shape, r.shape, t.shape)
        own = np.abs(t.astype(np.longdouble) - r)
        ulp = np.spacing(np.abs(r).astype(np.float64)).astype(np.longdouble)
        err = np.abs(dev.astype(np.longdouble) - r)
        ratio = float((err / (8 * own + 4 * ulp)).max())
        worst = max(worst, ratio)
        assert np.isfinite(dev).all() and np.all(err <= 8 * own + 4 * ulp), (P, S, K, n, ratio, float((err / ulp).max()))
        assert _same(d[n], again[n]), (P, S, K, n)                 # two launches: bit for bit
    return d, worst


@pytest.mark.parametrize("s_lo", [64, 2 ** 33])
def test_dumped_draws_against_the_longdouble_reference(s_lo):
    from successiveconvexification_amd.dynamics import IntegratorCache, mc_draws_device_batch
    c = IntegratorCache(_golden()[0], npts=10)
    ref = _reference(s_lo)
    names = ("xi0", "eta", "xin", "nud")
    worst = 0.0
    for P in (1, 3):
        ld, tw = ref[P]
        for S in (1, 63, 64, 65, 130):
            for K in (1, 3, 50):
                d, ratio = _dump_against_the_reference(c, ld, tw, s_lo, P, S, K)
                worst = max(worst, ratio)
                if S == 130 and K == 50:
                    eu = max(float((np.abs(d[n].reshape(ld[i].shape).astype(np.longdouble) - ld[i])
                                    / np.spacing(np.abs(ld[i]).astype(np.float64))).max()) for i, n in enumerate(names))
                    tu = max(float(rr.ulp_distance(tw[i], ld[i]).max()) for i in range(4))
                    print("s_lo %d P %d S 130 K 50: device vs longdouble %.2f ulp, float64 twin vs longdouble %.2f ulp" % (s_lo, P, eu, tu))
    print("s_lo %d: largest error / (8 x twin's + 4 ulp) over all shapes %.3f" % (s_lo, worst))
    # the independent plans differ from each other and from the shared stream; plan_lo shifts the rows
    d3 = mc_draws_device_batch(c, 5, K=2, seed=SEED, sample_lo=s_lo, plans=3)
    d1 = mc_draws_device_batch(c, 5, K=2, seed=SEED, sample_lo=s_lo, plan_lo=2, plans=1)
    assert _same(d1["eta"][0], d3["eta"][2]) and _same(d1["xin"][0], d3["xin"][2]) and not _same(d3["xi0"][0], d3["xi0"][1])
    c.close()


def _dump(c, S, K, seed, noise, m, lo=0, plans=None, plan_lo=0):
    from successiveconvexification_amd.dynamics import mc_draws_device_batch
    d = mc_draws_device_batch(c, S, K=K, seed=seed, sample_lo=lo, plan_lo=plan_lo, plans=plans)
    return d["xi0"], (d["eta"] if noise else None), d["xin"], (np.ascontiguousarray(d["nud"][..., :m]) if m else None)


def _fused_is_the_old_call(tag, c, po, x, u, s, d, L, S0, m, Ss, Bs, nsub):
    from successiveconvexification_amd.dynamics import nav_cov_batch, track_mc_batch, track_mc_nav_batch
    K = po.K
    w = np.full(14, 1e-8)
    w[0] = 0.0
    nav = m is not None
    if nav:
        H, rm = _model(m, x[0, 0])
        N0 = 0.25 * S0
    n = 0
    for wv in (None, w):
        kf = nav_cov_batch(c, x, u, d, L, np.zeros_like(S0), N0, H, rm, wv, dense=("kf",)).kf if nav and m else None
        for B in Bs:
            for S in Ss:
                xi0, eta, xin, nud = _dump(c, S, K, 17, wv is not None, m if nav else 0)
                for clamp in (False, True):
                    for quant in (False, True):
                        kw = dict(seed=17, w=wv, nsub=nsub, clamp=clamp, tol=1e-6)
                        if quant:
                            kw.update(quantiles=PROBS, per_node=True)
                        if nav:
                            a = (c, x[:B], u[:B], s[:B], d[:B], L[:B], S0[:B], N0[:B], H, rm, S)
                            dn = ("flights", "xland", "dx0", "navfed", "navK") + (("pathv",) if quant else ())
                            kk = dict(kf=None if kf is None else kf[:B], dense=dn, **kw)
                            old = track_mc_nav_batch(*a, draws=(xi0, eta, xin, nud), **kk)
                            new = track_mc_nav_batch(*a, rng="device", **kk)
                        else:
                            a = (c, x[:B], u[:B], s[:B], L[:B], S0[:B], S)
                            dn = ("flights", "xland", "dx0") + (("pathv",) if quant else ())
                            old = track_mc_batch(*a, draws=(xi0, eta), dense=dn, **kw)
                            new = track_mc_batch(*a, rng="device", dense=dn, **kw)
                        same = {nm: _eq(getattr(old, nm), getattr(new, nm)) for nm in (OLD_NAV if nav else OLD)}
                        if not all(same.values()):
                            print("%s B %d S %d clamp %s noise %s quantiles %s: %s" % (tag, B, S, clamp, wv is not None, quant, same))
                        assert all(same.values()), (tag, B, S, clamp, wv is not None, quant, same)
                        assert quant == (new.pathq is not None)
                        n += 1
        if wv is not None:
            assert not _same(new.xland, quiet)                                   # the impulses are felt
        quiet = new.xland
    print("%s: %d fused calls bitwise the old call fed the dump" % (tag, n))


@pytest.mark.parametrize("m", [None, 0, 3, 14])
@pytest.mark.parametrize("model", ["exo", "aero+fins+torque"])
def test_fused_flights_are_the_old_call_fed_the_dump(model, m, aero_tables):
    """m None: truth-fed (scvx_track_mc_rng_f64_host); else flown on an estimate with m measurement rows (scvx_track_mc_nav_rng_f64_host).
    exo: the golden plans and plan 0 with another S0; aero + fins + torque: the unconverged plans of the neighbouring tests"""
    c, po, dyn, par, x, u, s, d, L, S0 = _plans(model, aero_tables)
    _fused_is_the_old_call("%s m %s" % (model, m), c, po, x[:3], u[:3], s[:3], d[:3], L[:3], S0[:3], m, (1, 65, 130), (1, 3), 10)
    c.close()


@pytest.mark.parametrize("m", [None, 3])
@pytest.mark.parametrize("model", ["exo", "aero+fins"])
def test_fused_flights_at_a_short_horizon(model, m, aero_tables):
    import horizon_cases as hc
    from successiveconvexification_amd.dynamics import IntegratorCache, linearize_batch, track_gains_batch
    pp, po, dyn, par, x, u, s = hc.case(model, 3, aero_tables)
    c = IntegratorCache(pp, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (po.K + 1))
    S0 = np.stack([cr.handover_s0(x[b, 0])[0] for b in range(x.shape[0])])
    _fused_is_the_old_call("%s K = 3 m %s" % (model, m), c, po, x[:3], u[:3], s[:3], d[:3], track_gains_batch(c, d)[:3], S0[:3], m, (1, 65, 130),
                           (1, 3), 2)
    c.close()


def test_independent_rows_are_the_old_call_on_their_own_draws():
    """row b of one independent call with B = 3 is bitwise the old call at B = 1 on plan b fed dump[b]; with the same plan three times the
    shared draws give three identical rows, the independent ones three different xmean"""
    from successiveconvexification_amd.dynamics import track_mc_batch
    c, po, dyn, par, x, u, s, d, L, S0 = _plans("exo", None)
    K, S, m = po.K, 65, 6
    w = np.full(14, 1e-8)
    w[0] = 0.0
    H, rm = _model(m, x[0, 0])
    for nav in (None, (0.25 * S0, H, rm)):
        names = OLD_NAV if nav else OLD
        dn = ("flights", "xland", "dx0", "pathv") + (("navfed", "navK") if nav else ())
        kw = dict(seed=23, w=w, nsub=10, clamp=True, tol=1e-6, quantiles=PROBS, per_node=True, dense=dn)
        xi0, eta, xin, nud = _dump(c, S, K, 23, True, m, plans=3, plan_lo=4)
        new = track_mc_batch(c, x, u, s, L, S0, S, nav=nav, rng="device", independent=True, plan_lo=4, **kw)
        for b in range(3):
            sl = slice(b, b + 1)
            nb = None if nav is None else (nav[0][sl], H, rm)
            old = track_mc_batch(c, x[sl], u[sl], s[sl], L[sl], S0[sl], S, nav=nb,
                                 draws=(xi0[b], eta[b]) + ((xin[b], nud[b]) if nav else ()), **kw)
            same = {nm: _same(getattr(old, nm)[0], getattr(new, nm)[b]) for nm in names}
            print("independent, nav %s, row %d: bitwise the old call at B = 1 fed dump[%d]: %s" % (nav is not None, b, b, all(same.values())))
            assert all(same.values()), (b, same)
        x3, u3, s3, L3, S3 = (np.repeat(a[:1], 3, axis=0) for a in (x, u, s, L, S0))
        n3 = None if nav is None else (np.repeat(nav[0][:1], 3, axis=0), H, rm)
        sh = track_mc_batch(c, x3, u3, s3, L3, S3, S, nav=n3, rng="device", **kw)
        ind = track_mc_batch(c, x3, u3, s3, L3, S3, S, nav=n3, rng="device", independent=True, **kw)
        assert all(_same(getattr(sh, nm)[0], getattr(sh, nm)[b]) for nm in names for b in (1, 2))
        xm = ind.xmean[:, 1:7]
        print("one plan three times, nav %s: shared rows identical; independent xmean[1] %s" % (nav is not None, ind.xmean[:, 1]))
        assert not _same(xm[0], xm[1]) and not _same(xm[0], xm[2]) and not _same(xm[1], xm[2])
        assert not _same(ind.xmean[0], sh.xmean[0])                              # plan 0's own stream is not the shared one
    c.close()


def test_a_shard_is_rows_of_the_whole():
    from successiveconvexification_amd.dynamics import track_mc_batch
    c, po, dyn, par, x, u, s, d, L, S0 = _plans("exo", None)
    w = np.full(14, 1e-8)
    w[0] = 0.0
    H, rm = _model(3, x[0, 0])
    for nav in (None, (0.25 * S0, H, rm)):
        for ind in (False, True):
            kw = dict(seed=5, w=w, nsub=10, nav=nav, rng="device", independent=ind, dense=True)
            whole = track_mc_batch(c, x, u, s, L, S0, 130, **kw)
            part = track_mc_batch(c, x, u, s, L, S0, 66, sample_lo=64, **kw)
            for nm in ("flights", "xland", "dx0") + (("navfed", "navK") if nav else ()):
                assert _same(getattr(part, nm), getattr(whole, nm)[:, 64:130]), (nav is not None, ind, nm)
    c.close()


def test_pooled_statistics_over_independent_plans_within_six_standard_errors():
    """Golden plan 0 replicated 8 times, independent=True, S = 1,024: the covariance pooled over the 8,192 flights against the device's
    own covariance analysis with w (scvx_cov_propagate_f64), and flown on an estimate against scvx_nav_cov_f64 (28 x 28).  With shared
    draws this pooling is impossible: the eight rows would be the same 1,024 flights, and the pooled estimate would carry the error of
    1,024 samples while being judged by the standard error of 8,192."""
    from test_mc_cpu import w_case
    from test_mc_nav_cpu import nav_case
    from successiveconvexification_amd.dynamics import (IntegratorCache, cov_propagate_batch, linearize_batch, nav_cov_batch,
                                                          track_gains_batch, track_mc_batch)
    B, S = 8, 1024
    p, par, x, u, s, d_ref, L_ref, S0, w, covK_ref = w_case()
    c = IntegratorCache(_golden()[0], npts=10)
    sl = slice(0, 1)
    _, d = linearize_batch(c, x[sl], u[sl], s[sl], 1.0 / (p.K + 1))
    L = track_gains_batch(c, d)
    rep8 = lambda a: np.repeat(np.asarray(a)[:1], B, axis=0)   # noqa: E731
    covK = cov_propagate_batch(c, x[sl], u[sl], d, L, S0[None], w, dense=("covK",)).covK[0]
    r = track_mc_batch(c, rep8(x), rep8(u), rep8(s), rep8(L), S0, S, seed=0, w=w, nsub=10, rng="device", independent=True, dense=("xland",))
    e = (r.xland - x[0, -1]).reshape(B * S, 14)
    worst, over = mr.se_check(np.cov(e, rowvar=False), covK[:14, :14], B * S)
    sh = track_mc_batch(c, rep8(x), rep8(u), rep8(s), rep8(L), S0, S, seed=0, w=w, nsub=10, rng="device", dense=("xland",))
    worst_s, _ = mr.se_check(np.cov((sh.xland - x[0, -1]).reshape(B * S, 14), rowvar=False), covK[:14, :14], B * S)
    print("truth-fed, 8 x 1,024 independent flights pooled: worst entry %.2f standard errors, %d over 6 (the same pooling of SHARED draws: "
          "%.2f)" % (worst, over, worst_s))
    assert r.N_BAD.sum() == 0 and over == 0, (worst, over)
    p, par, x, u, s, d_ref, L_ref, S0, N0, H, rm, w, XiK_ref, kf_ref = nav_case()
    XiK = nav_cov_batch(c, x[sl], u[sl], d, L, S0[None], N0[None], H, rm, w, dense=("joint",)).joint[0, -1]
    r = track_mc_batch(c, rep8(x), rep8(u), rep8(s), rep8(L), S0, S, seed=0, w=w, nsub=10, nav=(N0, H, rm), rng="device", independent=True,
                       dense=("xland", "navK"))
    v = np.concatenate([r.xland - x[0, -1], r.navK], axis=2).reshape(B * S, 28)
    worst, over = mn.se_check(np.cov(v, rowvar=False), XiK, 14 + c.nu, B * S)
    print("flown on an estimate, pooled: worst entry of the 28 x 28 joint %.2f standard errors, %d over 6" % (worst, over))
    assert r.N_BAD.sum() == 0 and over == 0, (worst, over)
    c.close()


def test_batch_calls_margins_and_float_tiles():
    """ScvxBatch.track_mc(rng="device") is the context-level call (also on float tiles), margins_from_mc(rng="device") sets exactly
    montecarlo.margins_from_quantiles of its own pathq, and robustify(mc=dict(rng="device")) runs"""
    import bench
    from test_gpu_flight import _flyable
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache, track_mc_batch, track_mc_nav_batch
    from successiveconvexification_amd.montecarlo import margins_from_quantiles
    pp, po = _flyable()
    B = 3
    c = IntegratorCache(pp, npts=10)
    b = ScvxBatch(c, B).init(bench.disperse_ics(pp, 0, B, 7))
    b.solve()
    x, u, s = b.trajectory()
    sd = np.zeros(14)
    sd[1:7] = 1e-3 * np.abs(x[0, 0, 1:7])
    sd[7:] = 1e-3
    w = np.full(14, 1e-9)
    H, rm = _model(3, x[0, 0])
    nav = (0.25 * np.diag(sd * sd), H, rm)
    kw = dict(seed=4, w=w, clamp=True, tol=1e-6, quantiles=PROBS, per_node=True, rng="device", independent=True, sample_lo=64, plan_lo=2)
    rb = b.track_mc(sd, samples=70, dense=("flights", "pathv"), **kw)
    rh = track_mc_batch(c, x, u, s, b.track_gains(), sd, 70, nsub=10, dense=("flights", "pathv"), **kw)
    assert all(_same(getattr(rb, n), getattr(rh, n)) for n in ("raw", "xcov", "flights", "q", "pathq", "pathv"))
    nb = b.track_mc(sd, samples=70, nav=nav, dense=("pathv", "navfed"), **kw)
    nh = track_mc_batch(c, x, u, s, b.track_gains(), sd, 70, nsub=10, nav=nav, dense=("pathv", "navfed"), **kw)
    assert all(_same(getattr(nb, n), getattr(nh, n)) for n in ("raw", "navraw", "navfed", "q", "pathq", "pathv"))
    assert not _same(nb.raw, rb.raw)
    # float tiles: the batch call against the old batch call fed the dump
    b.set_linearization_f32(True)
    xi0, eta, xin, nud = _dump(c, 70, pp.K, 4, True, 3)
    k0 = dict(seed=4, w=w, clamp=True, tol=1e-6, quantiles=PROBS, per_node=True, dense=("flights", "xland", "dx0", "navfed", "navK", "pathv"))
    f_old = b.track_mc(sd, nav=nav, draws=(xi0, eta, xin, nud), **k0)
    f_new = b.track_mc(sd, samples=70, nav=nav, rng="device", **k0)
    same = {n: _same(getattr(f_old, n), getattr(f_new, n)) for n in OLD_NAV}
    print("float tiles through the batch call: bitwise %s" % same)
    assert all(same.values()), same
    b.set_linearization_f32(False)
    # the back-offs
    for nv in (None, nav):
        b.set_thrust_margins(None, None).set_path_margins()
        rep, lo, hi, pm = b.margins_from_mc(sd, samples=256, seed=3, nav=nv, rng="device", independent=True)
        want = margins_from_quantiles(pp, x, u, rep.pathq[..., 0], rep.pathq[..., 1], "all", 0.25)
        got = b.thrust_margins() + (b.path_margins(),)
        for a0, a1, a2 in zip(got, want, (lo, hi, pm)):
            assert np.array_equal(a0, a1) and np.array_equal(a0, a2)
        assert lo.any() and hi.any() and pm.any()
        host = b.track_mc(sd, samples=256, seed=3, nav=nv, quantiles=(1.0 - 0.99865, 0.99865), per_node=True)
        assert not _same(host.pathq, rep.pathq)                                  # rng="host" is still the uploaded draws
    st = b.robustify(sd, mc=dict(p=0.99865, samples=128, rng="device", independent=True))[0]
    print("robustify(mc=dict(rng='device', independent=True)): status %s" % st)
    assert st.shape == (B,)
    b.close(), c.close()


def test_rocketland_track_mc_with_device_draws():
    from successiveconvexification_amd import rocketland as rl, sample_problems as sp
    from successiveconvexification_amd.dynamics import IntegratorCache
    p = sp.base_prob_scaled
    c = IntegratorCache(p, npts=10)
    it = rl.create_initial(p, c)
    it, _, _ = rl.solve_step(it, c)
    sd = np.full(14, 1e-4)
    sd[0] = 0.0
    a = rl.track_mc(it, c, sd, samples=65, seed=2, w=1e-10, rng="device", dense=("xland",))
    b2 = rl.track_mc(it, c, sd, samples=65, seed=2, w=1e-10, rng="device", dense=("xland",))
    h = rl.track_mc(it, c, sd, samples=65, seed=2, w=1e-10, dense=("xland",))
    assert _same(a.xland, b2.xland) and not _same(a.xland, h.xland) and a.S[0] == 65
    c.close()


def test_argument_errors():
    from successiveconvexification_amd import _lib
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache, linearize_batch, track_gains_batch, track_mc_batch
    pp, po, x, u, s = _golden()
    c = IntegratorCache(pp, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (po.K + 1))
    gain = track_gains_batch(c, d)
    L, h, K, S = c._L, c.handle, pp.K, 4
    _dp = C.POINTER(C.c_double)
    ptr = lambda a: a.ctypes.data_as(_dp)   # noqa: E731
    C0 = np.ascontiguousarray(np.stack([np.eye(14) * 1e-3] * 2))
    rep, xm, xc = np.full((2, 48), 7.0), np.full((2, 14), 7.0), np.full((2, 14, 14), 7.0)
    jm, jc, nv = np.full((2, 28), 7.0), np.full((2, 28, 28), 7.0), np.full((2, 8), 7.0)
    err = lambda: L.scvx_last_error(h).decode()   # noqa: E731
    good = _lib.ScvxMcRng(1, 0, 0, 0, 0)
    b = ScvxBatch(c, 2).init(None)
    b.set_trajectory(x, u, s)
    q, r, qf = np.ones(14), np.ones(3), np.full(14, 100.0)
    out = np.full((1, S, 14), 7.0)

    def calls(rg):
        p = None if rg is None else C.byref(rg)
        tail = [None, None, None, 0, None, None, None, None]
        yield L.scvx_track_mc_rng_f64_host(h, 2, K, S, ptr(x), ptr(u), ptr(s), ptr(gain), ptr(C0), p, 0, None, None, 10, 0, 0.0, ptr(rep),
                                           ptr(xm), ptr(xc), *tail)
        yield L.scvx_track_mc_nav_rng_f64_host(h, 2, K, S, ptr(x), ptr(u), ptr(s), ptr(gain), ptr(C0), p, 0, None, ptr(d), None, ptr(C0), 0,
                                               None, None, 10, 0, 0.0, ptr(rep), ptr(xm), ptr(xc), ptr(jm), ptr(jc), ptr(nv), None, None,
                                               *tail)
        yield L.scvx_batch_track_mc_rng(b.handle, ptr(q), ptr(r), ptr(qf), S, ptr(C0), p, 0, None, None, 10, 0, 0.0, ptr(rep), ptr(xm),
                                        ptr(xc), *tail)
        yield L.scvx_batch_track_mc_nav_rng(b.handle, ptr(q), ptr(r), ptr(qf), S, ptr(C0), p, 0, None, ptr(C0), ptr(C0), 0, None, None, 10,
                                            0, 0.0, ptr(rep), ptr(xm), ptr(xc), ptr(jm), ptr(jc), ptr(nv), None, None, *tail)
        yield L.scvx_mc_draws_f64_host(h, p, 1, S, K, ptr(out), None, None, None)

    for rg, word in ((None, "null rng"), (_lib.ScvxMcRng(1, 0, 0, 0, 1), "reserved"), (_lib.ScvxMcRng(1, 0, 0, 2, 0), "independent")):
        for i, rc in enumerate(calls(rg)):
            assert rc == -1 and word in err(), (word, i, rc, err())
    assert np.all(rep == 7.0) and np.all(out == 7.0) and np.all(jc == 7.0)         # nothing ran
    assert L.scvx_mc_draws_f64_host(h, C.byref(good), 0, S, K, ptr(out), None, None, None) == -1 and "P" in err()
    assert L.scvx_track_mc_rng_f64_host(h, 2, K, S, ptr(x), ptr(u), ptr(s), ptr(gain), ptr(C0), C.byref(good), 1, None, None, 10, 0, 0.0,
                                        ptr(rep), ptr(xm), ptr(xc), None, None, None, 0, None, None, None, None) == -1   # noise without sw14
    for i, rc in enumerate(calls(good)):
        assert rc == 0, (i, rc, err())
    assert np.all(rep[:, 45] == S) and np.isfinite(out).all()
    with pytest.raises(ValueError):
        track_mc_batch(c, x, u, s, gain, np.full(14, 1e-3), 4, rng="device", draws=(np.zeros((4, 14)), None))
    with pytest.raises(ValueError):
        track_mc_batch(c, x, u, s, gain, np.full(14, 1e-3), 4, independent=True)
    with pytest.raises(ValueError):
        b.track_mc(np.full(14, 1e-3), samples=4, rng="device", draws=(np.zeros((4, 14)), None))
    b.close(), c.close()
