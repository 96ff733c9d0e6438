"""Order statistics and per-node samples of the sampled dispersion (scvx_order_stats_f64, scvx_track_mc_q_f64, scvx_track_mc_nav_q_f64,
their batch forms, ScvxBatch.margins_from_mc and robustify(mc=...)) on the MI355X.

Bounds, none of them taken from the device:
  * order statistics against numpy's sort and a rank: `==` on the values, identical NaN positions; two launches bit for bit.  flightq and
    pathq against numpy on the dense outputs of the SAME launch: bit for bit.
  * the outputs the old calls have: bit for bit the old calls'.
  * pathv against the flyer (scvx_track_fly_f64 / scvx_track_fly_nav_f64 with dense=True, fed the dx0 -- and navfed -- this call formed):
    MASS bit for bit; GLIDE within 4 eps (tan(gammaGs) |r[2:3]| + |r[1]|), TILT, RATE and (without the clamp) THRUST within 4 eps of
    their value: the kernel and numpy may contract the sum of squares differently, nothing else differs.
  * with the clamp and with noise, against mc_reference.chain through the C oracle: K * 1e-12 * A_cl on the states (test_gpu_mc.py's
    bound, A_cl the sensitivity of the REFERENCE chain), times the Lipschitz constant of each function in the sup norm -- 1 (MASS),
    sqrt(2) tan(gammaGs) + 1 (GLIDE), sqrt(2) (TILT), sqrt(3) (RATE) -- and for the commanded norm sqrt(3) (14 + nu) max(1, max |gain|),
    every entry of the law's input z = [dx; du] taken to be within the state bound.
  * back-offs: the batch holds exactly montecarlo.margins_from_quantiles of the report's own pathq.
Internal switches of scvx_quantile.hip, each with one S just below and one just above: up to QSMALL = 256 the ranks are counted by 64
lanes, above it a radix select runs on 256 lanes (S = 256, 257), and the keys leave LDS for global memory above QLDS = 4,096 (S = 4096,
4097).
Every comparison prints its figures before it asserts.
"""
import ctypes as C

import numpy as np
import pytest

import cov_reference as cr
import mc_quantile_reference as qr
import mc_reference as mr
import track_reference as tr
from test_gpu_flight import _case, _flyable
from test_gpu_mc import _golden, _same

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
QSMALL, QLDS = 256, 4096                  # scvx_quantile.hip
S_LIST = [1, 2, 3, 63, 64, 65, 127, 128, 129, 257, 1000, QSMALL, QLDS, QLDS + 1]   # 257 = QSMALL + 1 is in the issue's own list
PROBS = (0.0, 0.5, 0.99, 1.0)
OLD = ("raw", "xmean", "xcov", "flights", "xland", "dx0")
OLD_NAV = OLD + ("jmean", "jcov", "navraw", "navfed", "navK")
_ip = C.POINTER(C.c_int)
_dp = C.POINTER(C.c_double)


def _ptr(a):
    return a.ctypes.data_as(_dp)


def _rows(R, S, seed):
    """R rows of S values, the kinds cycling: normal draws (negatives), +-0 / +-inf / denormals among them, all equal, heavy ties, a few
    NaNs (both signs of the NaN), all NaNs, wide exponents, -0 and +0 only"""
    rng = np.random.default_rng(seed)
    v = np.empty((R, S))
    special = np.array([0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 2.2e-308, -1e-310, 1.0, -1.0])
    for r in range(R):
        kind = r % 8
        a = rng.standard_normal(S)
        if kind == 1:
            m = rng.random(S) < 0.6
            a[m] = rng.choice(special, int(m.sum()))
        elif kind == 2:
            a[:] = rng.standard_normal()
        elif kind == 3:
            a = rng.integers(-2, 2, S).astype(float)
        elif kind == 4:
            m = rng.random(S) < 0.1
            a[m] = np.nan
            a[m & (rng.random(S) < 0.5)] = -np.nan
            if S > 1:
                a[rng.integers(S)] = np.nan
        elif kind == 5:
            a[:] = np.nan
        elif kind == 6:
            a = a * 10.0 ** rng.integers(-300, 300, S)
        elif kind == 7:
            a = np.where(rng.random(S) < 0.5, 0.0, -0.0)
        v[r] = a
    return v


def _order_stats(c, v, inc, ranks):
    """scvx_order_stats_f64_host on the rows v [R][S] laid out inc apart in a padded buffer (ld = (S - 1) inc + 4); the padding holds
    -1e300, which a read outside a row would bring to rank 0"""
    R, S = v.shape
    ld = (S - 1) * inc + 4
    buf = np.full((R - 1) * ld + (S - 1) * inc + 1, -1e300)
    for r in range(R):
        buf[r * ld:r * ld + (S - 1) * inc + 1:inc] = v[r]
    rk = np.ascontiguousarray(ranks, np.int32)
    out = np.full((R, rk.size), 7.0)
    rc = c._L.scvx_order_stats_f64_host(c.handle, R, S, _ptr(buf), ld, inc, rk.size, rk.ctypes.data_as(_ip), _ptr(out))
    assert rc == 0, c._L.scvx_last_error(c.handle)
    return out


@pytest.mark.parametrize("S", S_LIST)
def test_order_statistics_against_numpy(S):
    from successiveconvexification_amd.dynamics import IntegratorCache
    c = IntegratorCache(_flyable()[0], npts=10)
    ranks = [S // 2, 0, S - 1, S // 2, 0, S - 1, S // 2]              # repeated and unsorted
    for R in (1, 5, 300):
        for inc in (1, 16):
            v = _rows(R, S, 1000 * S + 10 * R + inc)
            got = _order_stats(c, v, inc, ranks)
            ref = qr.order_stats(v, ranks)
            nan_g, nan_r = np.isnan(got), np.isnan(ref)
            ok = np.array_equal(nan_g, nan_r) and np.all(got[~nan_r] == ref[~nan_r])
            print("S %d R %d inc %d: %d values, %d NaN, equal %s" % (S, R, inc, got.size, nan_r.sum(), ok))
            assert np.array_equal(nan_g, nan_r), (S, R, inc)
            assert np.all(got[~nan_r] == ref[~nan_r]), (S, R, inc)
            # a selection: every output that is not a NaN is one of its row's inputs bit for bit
            for r in range(R):
                assert np.isin(got[r][~nan_g[r]].view(np.uint64), v[r].view(np.uint64)).all(), (S, R, inc, r)
            again = _order_stats(c, v, inc, ranks)
            assert np.array_equal(got.view(np.uint64), again.view(np.uint64))      # two launches: bit for bit
    one = _order_stats(c, _rows(5, S, S), 1, [S - 1])
    assert one.shape == (5, 1)
    all16 = _order_stats(c, _rows(3, S, S + 1), 1, [(7 * i) % S for i in range(16)])  # nq = SCVX_Q_MAX
    assert _same(all16, qr.order_stats(_rows(3, S, S + 1), [(7 * i) % S for i in range(16)]))
    c.close()


def test_order_statistics_refusals():
    from successiveconvexification_amd.dynamics import IntegratorCache
    c = IntegratorCache(_flyable()[0], npts=10)
    L, h = c._L, c.handle
    R, S = 3, 10
    v = np.arange(R * 12.0)
    out = np.full((R, 2), 7.0)
    rk = np.array([0, 9], np.int32)
    err = lambda: L.scvx_last_error(h).decode()   # noqa: E731
    good = dict(R=R, S=S, v=v, ld=12, inc=1, nq=2, ranks=rk, out=out)
    cases = [(dict(R=0), "R >= 1"), (dict(S=0), "S >= 1"), (dict(nq=0), "nq"), (dict(nq=17, ranks=np.zeros(17, np.int32)), "nq"),
             (dict(ranks=np.array([0, 10], np.int32)), "rank"), (dict(ranks=np.array([-1, 3], np.int32)), "rank"), (dict(inc=0), "inc"),
             (dict(ld=9), "ld"), (dict(inc=2, ld=18), "ld"), (dict(v=None), "null"), (dict(ranks=None), "null"), (dict(out=None), "null")]
    for kw, word in cases:
        a = dict(good)
        a.update(kw)
        pr = None if a["ranks"] is None else a["ranks"].ctypes.data_as(_ip)
        host = (a["R"], a["S"], None if a["v"] is None else _ptr(a["v"]), a["ld"], a["inc"], a["nq"], pr, None if a["out"] is None else _ptr(a["out"]))
        dev = (a["R"], a["S"], None if a["v"] is None else C.c_void_p(1), a["ld"], a["inc"], a["nq"], pr,
               None if a["out"] is None else C.c_void_p(1))        # the checks come before any device pointer is used
        for fn, args in ((L.scvx_order_stats_f64_host, host), (L.scvx_order_stats_f64, dev)):
            assert fn(h, *args) == -1, (kw, fn)
            assert word in err(), (kw, err())
    assert L.scvx_order_stats_f64_host(None, R, S, _ptr(v), 12, 1, 2, rk.ctypes.data_as(_ip), _ptr(out)) == -1
    assert np.all(out == 7.0)                                         # nothing ran
    assert L.scvx_order_stats_f64_host(h, R, S, _ptr(v), 12, 1, 2, rk.ctypes.data_as(_ip), _ptr(out)) == 0
    assert np.array_equal(out, [[0, 9], [12, 21], [24, 33]])
    # a single row needs no ld
    assert L.scvx_order_stats_f64_host(h, 1, S, _ptr(v), 0, 1, 2, rk.ctypes.data_as(_ip), _ptr(out)) == 0 and out[0, 1] == 9
    c.close()


def _plans(model, aero_tables, c=None):
    """(cache, po, dyn, par, x, u, s, deriv, gains, S0): exo = the golden plans and plan 0 again with another S0 (B = 3); else the
    unconverged dispersed plans of the model (B = 5)"""
    from oracle import dynamics as od
    from successiveconvexification_amd.dynamics import IntegratorCache, linearize_batch, track_gains_batch
    if model == "exo":
        pp, po, x, u, s = _golden()
        x, u, s = x[[0, 1, 0]], u[[0, 1, 0]], s[[0, 1, 0]]
        dyn, par = od, od.Params(po)
        S0 = np.stack([cr.handover_s0(x[0, 0])[0], cr.handover_s0(x[1, 0])[0], cr.handover_s0(x[0, 0], seed=1, size=3e-3)[0]])
    else:
        pp, po, dyn, par, x, u, s = _case(model, aero_tables)
        S0 = np.stack([cr.handover_s0(x[b, 0])[0] for b in range(x.shape[0])])
    c = IntegratorCache(pp, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (po.K + 1))
    return c, po, dyn, par, x, u, s, d, track_gains_batch(c, d), S0


def _check_flightq(tag, rep):
    B, S, _ = rep.flights.shape
    ref = qr.order_stats(rep.flights, rep.ranks, axis=1)               # [B][16][nq]
    assert rep.q.shape == ref.shape == (B, 16, len(rep.ranks))
    print("%s: flightq bitwise %s, -inf columns %s, NaN entries %d" % (tag, _same(rep.q, ref), np.isneginf(ref).all(axis=(0, 2)).nonzero()[0].tolist(),
                                                                     np.isnan(ref).sum()))
    assert _same(rep.q, ref), tag
    assert np.array_equal(rep.ranks, qr.ranks(rep.probs, S))


def _check_pathq(tag, rep):
    ref = qr.order_stats(rep.pathv, rep.ranks)                          # [B][K+1][5][nq]
    print("%s: pathq bitwise the order statistics of the launch's own pathv: %s" % (tag, _same(rep.pathq, ref)))
    assert _same(rep.pathq, ref), tag


@pytest.mark.parametrize("model", ["exo", "aero+fins+torque"])
def test_flightq_and_pathq_are_the_order_statistics_of_the_dense_outputs(model, aero_tables):
    """B in {1, 3}, S in {1, 63, 64, 65, 130}, with and without the clamp and the noise: flightq against numpy on the launch's own
    flights, pathq on its own pathv, and without the dense outputs (the workspace path) the same bits; the outputs the old call has are
    the old call's"""
    from successiveconvexification_amd.dynamics import track_mc_batch
    c, po, dyn, par, x, u, s, d, L, S0 = _plans(model, aero_tables)
    w = np.full(14, 1e-8)
    w[0] = 0.0
    for B in (1, 3):
        a = (c, x[:B], u[:B], s[:B], L[:B], S0[:B])
        for S in (1, 63, 64, 65, 130):
            for clamp in (False, True):
                for wv in (None, w):
                    tag = "%s B %d S %d clamp %s noise %s" % (model, B, S, clamp, wv is not None)
                    kw = dict(seed=11, w=wv, nsub=10, clamp=clamp, tol=1e-6)
                    old = track_mc_batch(*a, S, dense=True, **kw)
                    new = track_mc_batch(*a, S, dense=("flights", "xland", "dx0", "pathv"), quantiles=PROBS, per_node=True, **kw)
                    assert all(_same(getattr(old, n), getattr(new, n)) for n in OLD), tag
                    assert old.q is None and old.pathq is None and old.pathv is None
                    _check_flightq(tag, new)
                    _check_pathq(tag, new)
                    assert np.isneginf(new.q[:, 13]).all()                  # G_DP: not enforced by these models, -inf stays -inf
                    assert np.isneginf(new.q[:, 14]).all() == ("fins" not in model)
                    lean = track_mc_batch(*a, S, quantiles=PROBS, per_node=True, **kw)                  # no dense output: the workspace
                    assert lean.flights is None and lean.pathv is None
                    assert _same(lean.q, new.q) and _same(lean.pathq, new.pathq) and _same(lean.raw, old.raw), tag
                    only = track_mc_batch(*a, S, quantiles=PROBS, **kw)                                 # flightq alone
                    assert only.pathq is None and _same(only.q, new.q) and _same(only.xcov, old.xcov)
    # p = 0 and p = 1 are the minimum and MAX_c
    assert _same(new.q[:, :, 3], new.raw[:, :16]) and _same(new.q[:, :, 0], new.flights.min(axis=1))
    c.close()


def test_a_nan_gain_poisons_the_quantiles_of_its_plan_only():
    from successiveconvexification_amd.dynamics import track_mc_batch
    c, po, dyn, par, x, u, s, d, L, S0 = _plans("exo", None)
    S = 70
    good = track_mc_batch(c, x, u, s, L, S0, S, seed=9, nsub=10, quantiles=PROBS, per_node=True, dense=("pathv",))
    Ln = L.copy()
    Ln[1, 20, 1, 3] = np.nan
    bad = track_mc_batch(c, x, u, s, Ln, S0, S, seed=9, nsub=10, quantiles=PROBS, per_node=True, dense=("pathv",))
    I = mr.FLIGHT.index
    print("NaN gain in plan 1: flightq NaN columns %s; pathq NaN from node %d" % (np.isnan(bad.q[1]).all(axis=1).nonzero()[0].tolist(),
                                                                                int(np.isnan(bad.pathq[1]).any(axis=(1, 2)).argmax())))
    for col in ("GAP", "MISS_R", "MISS_V", "MISS_Q", "MISS_W", "G_MASS", "G_GLIDE", "G_TILT", "G_RATE", "QNORM"):
        assert np.isnan(bad.q[1, I(col)]).all(), col
    assert np.isnan(bad.pathq[1, 22:]).all() and _same(bad.pathq[1, :21, :4], good.pathq[1, :21, :4])
    for b in (0, 2):
        assert _same(bad.q[b], good.q[b]) and _same(bad.pathq[b], good.pathq[b]) and _same(bad.pathv[b], good.pathv[b])
    c.close()


def _against_the_flyer(tag, po, x, u, pathv, xfly, ufly, clamp):
    """pathv [B][K+1][5][S] against the flyer's dense xfly [B S][K+1][14], ufly [B S][K+1][nu]"""
    B, K1, _, S = pathv.shape
    pv = np.moveaxis(pathv, 3, 1).reshape(B * S, K1, 5)
    tg = qr.tggs(po)
    r23 = np.sqrt(xfly[:, :, 2] ** 2 + xfly[:, :, 3] ** 2)
    ref = qr.path_values(po, xfly, np.linalg.norm(ufly[:, 1:, :3], axis=-1), [1.0, 0.0, 0.0])
    bound = np.stack([np.zeros_like(r23), 4 * EPS * (tg * r23 + np.abs(xfly[:, :, 1])), 4 * EPS * ref[:, :, 2], 4 * EPS * ref[:, :, 3],
                      4 * EPS * ref[:, :, 4]], axis=-1)
    err = np.abs(pv - ref)
    cols = range(4) if clamp else range(5)                              # with the clamp ufly is the CLAMPED control: THRUST is checked elsewhere
    for f in cols:
        k = slice(1, None) if f == 4 else slice(None)
        ratio = float((err[:, k, f] / np.where(bound[:, k, f] > 0, bound[:, k, f], 1.0)).max())
        print("%s %-6s: largest error %.3e, largest error / bound %.3f%s" % (tag, qr.COLUMNS[f], err[:, k, f].max(), ratio, " (bitwise)" if f == 0 else ""))
        assert np.all(err[:, k, f] <= bound[:, k, f]), (tag, qr.COLUMNS[f])
    assert _same(pv[:, :, 0], xfly[:, :, 0])                            # MASS: bit for bit
    # node 0: the state is xbar_0 + dx0 (xfly[0] of the flyer IS that sum), the thrust |ubar_0|, one value for every sample
    u0 = np.linalg.norm(u[:, 0, :3], axis=-1)
    t0 = pathv[:, 0, 4, :]
    assert np.all(t0 == t0[:, :1]) and np.all(np.abs(t0[:, 0] - u0) <= 4 * EPS * u0)
    assert _same(pathv[:, 0, 0, :], xfly[:, 0, 0].reshape(B, S))


@pytest.mark.parametrize("model", ["exo", "aero+fins+torque"])
def test_pathv_against_the_flyer_truth_fed(model, aero_tables):
    from successiveconvexification_amd.dynamics import track_fly_batch, track_mc_batch
    c, po, dyn, par, x, u, s, d, L, S0 = _plans(model, aero_tables)
    B, K = x.shape[0], po.K
    for S in (65, 130):
        for clamp in (False, True):
            r = track_mc_batch(c, x, u, s, L, S0, S, seed=5, nsub=10, clamp=clamp, dense=("dx0", "pathv"), quantiles=(0.5,), per_node=True)
            assert r.pathv.shape == (B, K + 1, 5, S) and _same(r.dx0[:, :, 0], np.zeros((B, S)))
            t = track_fly_batch(c, cr.rep(x, S), cr.rep(u, S), cr.rep(s, S), cr.rep(L, S), r.dx0.reshape(B * S, 14), nsub=10, clamp=clamp, dense=True)
            _against_the_flyer("%s S %d clamp %s" % (model, S, clamp), po, x, u, r.pathv, t.xfly, t.ufly, clamp)
            assert _same(r.pathv[:, 0, 0, :], (x[:, 0, 0][:, None] + r.dx0[:, :, 0]))
            _check_pathq("%s S %d clamp %s" % (model, S, clamp), r)
    c.close()


def _against_the_chain(tag, c, po, dyn, par, x, u, s, nsub, S, seed):
    """with the clamp and with noise: pathv against mc_reference.chain's xfly and cmd, gains of the REFERENCE fed to both sides"""
    from successiveconvexification_amd.dynamics import linearize_batch, track_mc_batch
    from successiveconvexification_amd.montecarlo import handover_factor, mc_draws
    B, K = x.shape[0], po.K
    _, d = linearize_batch(c, x, u, s, 1.0 / (K + 1))
    L, _ = tr.gains(d, K)
    S0 = np.stack([cr.handover_s0(x[b, 0])[0] for b in range(B)])
    w = np.full(14, 1e-8)
    w[0] = 0.0
    xi0, eta = mc_draws(S, K, seed, noise=True)
    imp = eta * np.sqrt(w)
    nu = u.shape[-1]
    lip = np.array([1.0, np.sqrt(2.0) * qr.tggs(po) + 1.0, np.sqrt(2.0), np.sqrt(3.0), np.sqrt(3.0) * (14 + nu) * max(1.0, float(np.abs(L).max()))])
    for clamp in (False, True):
        dev = track_mc_batch(c, x, u, s, L, S0, S, seed=seed, w=w, nsub=nsub, clamp=clamp, dense=("pathv",), quantiles=(0.5,), per_node=True)
        for b in range(B):
            dx0 = xi0 @ handover_factor(S0[b]).T
            flags = tr.CLAMP if clamp else 0
            bc = lambda a: np.broadcast_to(np.asarray(a, float), (S,) + np.shape(a))   # noqa: E731
            _, _, xf, _, cmd = mr.chain(dyn, par, po, bc(x[b]), bc(u[b]), np.full(S, float(s[b])), bc(L[b]), dx0, nsub, flags, imp)
            A = mr.sensitivity(dyn, po, x[b], u[b], s[b], L[b], dx0, nsub, 1e-9, flags, imp, par=par)
            bound = K * 1e-12 * A
            ref = qr.path_values(po, xf, cmd, u[b, 0])
            err = np.abs(np.moveaxis(dev.pathv[b], 2, 0) - ref).max(axis=(0, 1))
            print("%s plan %d nsub %d clamp %s: A_cl %.3f, state bound %.3e, errors %s, bounds %s" % (tag, b, nsub, clamp, A, bound, err, bound * lip))
            assert np.all(err <= bound * lip), (tag, b, clamp)
            if clamp:
                out = (cmd < po.Tmin) | (cmd > po.Tmax)
                print("    %d of %d commanded norms are outside the band: pathv holds them UNCLAMPED" % (out.sum(), out.size))
        _check_pathq(tag, dev)


@pytest.mark.parametrize("model", ["exo", "aero+fins"])
def test_pathv_with_clamp_and_noise_against_the_cpu_chain_at_a_short_horizon(model, aero_tables):
    import horizon_cases as hc
    from successiveconvexification_amd.dynamics import IntegratorCache
    pp, po, dyn, par, x, u, s = hc.case(model, 3, aero_tables)
    c = IntegratorCache(pp, npts=10)
    _against_the_chain("%s K = 3" % model, c, po, dyn, par, x, u, s, 2, 5, 31)
    c.close()


def test_pathv_with_clamp_and_noise_against_the_cpu_chain_on_the_golden_plans():
    from oracle import dynamics as od
    from successiveconvexification_amd.dynamics import IntegratorCache
    pp, po, x, u, s = _golden()
    c = IntegratorCache(pp, npts=10)
    _against_the_chain("golden plans K = 50", c, po, od, od.Params(po), x, u, s, 10, 5, 32)
    c.close()


def test_navigation_form(aero_tables):
    """CN = 0, no measurement, no noise: pathv, pathq and flightq bit for bit the truth-fed call's.  With estimate errors: the outputs
    the old navigation call has are the old call's, and pathv is checked against the flyer on estimates fed the navfed this call formed"""
    from test_gpu_mc_nav import _model
    from successiveconvexification_amd.dynamics import track_fly_batch, track_mc_batch, track_mc_nav_batch
    c, po, dyn, par, x, u, s, d, L, S0 = _plans("exo", None)
    B, K, S = x.shape[0], po.K, 130
    kwq = dict(quantiles=PROBS, per_node=True)
    for clamp in (False, True):
        tf = track_mc_batch(c, x, u, s, L, S0, S, seed=5, nsub=10, clamp=clamp, dense=("pathv",), **kwq)
        nv = track_mc_nav_batch(c, x, u, s, d, L, S0, np.zeros((14, 14)), None, None, S, seed=5, nsub=10, clamp=clamp, dense=("pathv",), **kwq)
        same = {n: _same(getattr(tf, n), getattr(nv, n)) for n in ("pathv", "pathq", "q", "raw")}
        print("no estimate error, clamp %s: bitwise the truth-fed call's %s" % (clamp, same))
        assert all(same.values()), same
    H, rm = _model(6, x[0, 0])
    w = np.full(14, 1e-8)
    w[0] = 0.0
    for clamp in (False, True):
        for wv in (None, w):
            kw = dict(seed=5, w=wv, nsub=10, clamp=clamp, tol=1e-6)
            old = track_mc_nav_batch(c, x, u, s, d, L, S0, 0.25 * S0, H, rm, S, dense=True, **kw)
            new = track_mc_nav_batch(c, x, u, s, d, L, S0, 0.25 * S0, H, rm, S, dense=("flights", "xland", "dx0", "navfed", "navK", "pathv"), **kw, **kwq)
            tag = "navigation m 6 clamp %s noise %s" % (clamp, wv is not None)
            assert all(_same(getattr(old, n), getattr(new, n)) for n in OLD_NAV), tag
            _check_flightq(tag, new)
            _check_pathq(tag, new)
            lean = track_mc_nav_batch(c, x, u, s, d, L, S0, 0.25 * S0, H, rm, S, **kw, **kwq)
            assert lean.pathv is None and _same(lean.pathq, new.pathq) and _same(lean.q, new.q) and _same(lean.navraw, old.navraw), tag
            if wv is None:
                t = track_fly_batch(c, cr.rep(x, S), cr.rep(u, S), cr.rep(s, S), cr.rep(L, S), new.dx0.reshape(B * S, 14), nsub=10, clamp=clamp,
                                    dense=True, nav=new.navfed.reshape(B * S, K, 14))
                _against_the_flyer(tag, po, x, u, new.pathv, t.xfly, t.ufly, clamp)
                assert not _same(new.pathv, tf.pathv)                  # the estimate's error is felt
    c.close()


def test_batch_level_calls_are_the_context_level_ones():
    import bench
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache, track_mc_batch
    from test_gpu_mc_nav import _model
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
    kw = dict(seed=4, w=w, clamp=True, tol=1e-6, quantiles=PROBS, per_node=True)
    rb = b.track_mc(sd, samples=70, dense=("flights", "pathv"), **kw)
    rh = track_mc_batch(c, x, u, s, b.track_gains(), sd, 70, nsub=10, dense=("flights", "pathv"), **kw)
    for n in ("raw", "xcov", "flights", "q", "pathq", "pathv"):
        assert _same(getattr(rb, n), getattr(rh, n)), n
    _check_flightq("batch", rb)
    _check_pathq("batch", rb)
    assert _same(b.track_mc(sd, samples=70, **kw).pathq, rb.pathq) and _same(b.track_mc(sd, samples=70, seed=4, w=w, clamp=True, tol=1e-6).raw, rb.raw)
    H, rm = _model(3, x[0, 0])
    nav = (0.25 * np.diag(sd * sd), H, rm)
    nb = b.track_mc(sd, samples=70, nav=nav, dense=("pathv", "navfed"), **kw)
    nh = track_mc_batch(c, x, u, s, b.track_gains(), sd, 70, nsub=10, nav=nav, dense=("pathv", "navfed"), **kw)
    for n in ("raw", "navraw", "navfed", "q", "pathq", "pathv"):
        assert _same(getattr(nb, n), getattr(nh, n)), n
    _check_pathq("batch, navigation", nb)
    assert _same(b.track_mc(sd, samples=70, nav=nav, seed=4, w=w, clamp=True, tol=1e-6).raw, nb.raw)
    assert np.array_equal(rb.quantile("MISS_R", 0.5), np.sort(rb.flights[:, :, 1], axis=1)[:, 34])      # named access: ceil(0.5 * 70) - 1
    assert nb.quantile("MISS_R", 0.99).shape == (B,) and nb.path_quantile("THRUST", 1.0).shape == (B, pp.K + 1)
    b.close(), c.close()


def test_new_arguments_are_checked():
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache, linearize_batch, track_gains_batch, track_mc_batch
    pp, po, x, u, s = _golden()
    c = IntegratorCache(pp, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (po.K + 1))
    gain = track_gains_batch(c, d)
    L, h, K, S = c._L, c.handle, pp.K, 4
    C0 = np.ascontiguousarray(np.stack([np.eye(14) * 1e-3] * 2))
    xi0 = np.zeros((S, 14))
    rep, xm, xc = np.full((2, 48), 7.0), np.full((2, 14), 7.0), np.full((2, 14, 14), 7.0)
    fq = np.full((2, 16, 2), 7.0)
    err = lambda: L.scvx_last_error(h).decode()   # noqa: E731
    rk = lambda *v: np.array(v, np.int32).ctypes.data_as(_ip)   # noqa: E731
    head = [h, 2, K, S] + [_ptr(a) for a in (x, u, s, gain, C0, xi0)] + [None, None, None, 10, 0, 0.0, _ptr(rep), _ptr(xm), _ptr(xc), None, None, None]
    for tail, word in (([0, None, _ptr(fq), None, None], "nq"), ([17, rk(*range(17)), _ptr(fq), None, None], "nq"), ([2, None, _ptr(fq), None, None], "null"),
                       ([2, rk(0, 4), _ptr(fq), None, None], "rank"), ([2, rk(-1, 0), None, _ptr(fq), None], "rank")):
        assert L.scvx_track_mc_q_f64_host(*head, *tail) == -1 and word in err(), (tail, err())
    bad_old = list(head)
    bad_old[3] = 0                                                    # and everything the old call refuses
    assert L.scvx_track_mc_q_f64_host(*bad_old, 2, rk(0, 0), _ptr(fq), None, None) == -1 and "S >= 1" in err()
    assert np.all(rep == 7.0) and np.all(fq == 7.0)                   # nothing ran
    assert L.scvx_track_mc_q_f64_host(*head, 0, None, None, None, None) == 0 and np.all(rep[:, 45] == S)   # nothing asked for: the old call
    old = np.empty((2, 48))
    assert L.scvx_track_mc_f64_host(*head[:16], _ptr(old), *head[17:]) == 0 and _same(old, rep)
    assert L.scvx_track_mc_q_f64_host(*head, 2, rk(3, 0), _ptr(fq), None, None) == 0 and np.all(fq[:, :, 0] >= fq[:, :, 1])
    b = ScvxBatch(c, 2).init(None)
    b.set_trajectory(x, u, s)
    q, r, qf = np.ones(14), np.ones(3), np.full(14, 100.0)
    bh = [b.handle, _ptr(q), _ptr(r), _ptr(qf), S, _ptr(C0), _ptr(xi0), None, None, None, 0, 0, 0.0, _ptr(rep), _ptr(xm), _ptr(xc), None, None, None]
    assert L.scvx_batch_track_mc_q(*bh, 2, rk(0, 9), _ptr(fq), None, None) == -1 and "rank" in err()
    assert L.scvx_batch_track_mc_q(*bh, 2, rk(0, 3), _ptr(fq), None, None) == 0
    with pytest.raises(ValueError):
        track_mc_batch(c, x, u, s, gain, np.full(14, 1e-3), 4, quantiles=(1.2,))
    with pytest.raises(ValueError):
        track_mc_batch(c, x, u, s, gain, np.full(14, 1e-3), 4, per_node=True)
    with pytest.raises(ValueError):
        b.margins_from_mc(np.full(14, 1e-3), samples=8, constraints=("gimbal",))
    with pytest.raises(ValueError):
        b.robustify(np.full(14, 1e-3), mc=dict(sample=8))
    b.close(), c.close()


def test_margins_from_mc_sets_what_margins_from_quantiles_says():
    """the two golden plans, S = 256: the batch holds exactly montecarlo.margins_from_quantiles of the report's own pathq; the kinds
    that are not selected keep their values"""
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache
    from successiveconvexification_amd.montecarlo import margins_from_quantiles
    from test_gpu_mc_nav import _model
    pp, po, x, u, s = _golden()
    c = IntegratorCache(pp, npts=10)
    b = ScvxBatch(c, 2).init(None)
    b.set_trajectory(x, u, s)
    S0 = np.stack([cr.handover_s0(x[i, 0])[0] for i in range(2)])
    H, rm = _model(3, x[0, 0])
    for nav in (None, (0.25 * S0, H, rm)):
        b.set_thrust_margins(None, None).set_path_margins()
        rep, lo, hi, pm = b.margins_from_mc(S0, samples=256, seed=3, nav=nav)
        assert rep.pathq.shape == (2, pp.K + 1, 5, 2) and rep.probs.tolist() == [1.0 - 0.99865, 0.99865] and rep.ranks.tolist() == [0, 255]
        want = margins_from_quantiles(pp, x, u, rep.pathq[..., 0], rep.pathq[..., 1], "all", 0.25)
        got = b.thrust_margins() + (b.path_margins(),)
        print("margins_from_mc nav %s: back-offs up to lo %s hi %s mass %s glide %s tilt %s rate %s" % (nav is not None, lo.max(axis=1), hi.max(axis=1),
              *[pm[:, :, i].max(axis=1) for i in range(4)]))
        for a0, a1, a2 in zip(got, want, (lo, hi, pm)):
            assert np.array_equal(a0, a1) and np.array_equal(a0, a2)
        assert lo.any() and hi.any() and pm.any() and not np.array_equal(lo, hi)
    # unselected kinds are untouched
    b.set_thrust_margins(0.011, 0.012).set_path_margins(mass=0.0013, glide=0.0014, tilt=0.0015, rate=0.0016)
    before = b.thrust_margins() + (b.path_margins(),)
    rep, lo, hi, pm = b.margins_from_mc(S0, samples=256, seed=3, constraints=("tilt", "mass"), clamp=True)
    after = b.thrust_margins() + (b.path_margins(),)
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1]) and np.array_equal(after[2][:, :, [1, 3]], before[2][:, :, [1, 3]])
    want = margins_from_quantiles(pp, x, u, rep.pathq[..., 0], rep.pathq[..., 1], ("tilt", "mass"), 0.25, current=before)
    assert np.array_equal(after[2], want[2]) and not np.array_equal(after[2][:, :, 2], before[2][:, :, 2])
    b.close(), c.close()


@pytest.mark.parametrize("with_nav", [False, True])
def test_one_round_of_replanning_on_the_sampled_closed_loop(with_nav):
    """robustify(mc=dict(p=0.99865, samples=256)), truth-fed and flown on the estimate: both plans end converged, and a sampled run on
    the SAME draws shows fewer commanded controls outside the thrust band than the base plans do, for both.  The counts, the step
    counts, the final masses and the first-order report's N_TMIN / N_TMAX are printed for the README, not asserted."""
    import os
    from conftest import GOLDEN
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache
    f = np.load(os.path.join(GOLDEN, "oracle_nav_margin_runs.npz"))
    pp, po = _flyable()
    c = IntegratorCache(pp, npts=10)
    base, rob = (ScvxBatch(c, f["ic"].shape[0]).init(f["ic"]) for _ in range(2))
    for b in (base, rob):
        assert np.all(b.solve()[0] == 0)
    S0 = f["S0"]
    nav = (f["N0"], f["H"], f["rm"]) if with_nav else None
    st, it, nu, dj, lo, hi = rob.robustify(S0, mc=dict(p=0.99865, samples=256), nav=nav)
    r0 = base.track_mc(S0, samples=256, seed=0, nav=nav)
    r1 = rob.track_mc(S0, samples=256, seed=0, nav=nav)
    out0, out1 = (r0.OUT_LO + r0.OUT_HI) * 256 * pp.K, (r1.OUT_LO + r1.OUT_HI) * 256 * pp.K
    rep0, rep1 = ((b.navigation(S0, *nav) if with_nav else b.covariance(S0)) for b in (base, rob))
    print("robustify(mc, nav %s): status %s in %s steps; commanded controls outside the band on the same 256 draws x %d nodes: base %s -> %s; "
          "final mass %s -> %s; first-order report N_TMIN %s -> %s, N_TMAX %s -> %s; back-offs up to lo %s hi %s"
          % (with_nav, st, it, pp.K, out0, out1, base.trajectory()[0][:, -1, 0], rob.trajectory()[0][:, -1, 0], rep0.N_TMIN, rep1.N_TMIN, rep0.N_TMAX,
             rep1.N_TMAX, lo.max(axis=1), hi.max(axis=1)))
    assert np.all(st == 0), (st, it)
    assert np.all(out1 < out0), (out0, out1)
    base.close(), rob.close(), c.close()
