"""Plan tracking (scvx_track_gains_f64 / scvx_track_fly_f64 / scvx_batch_track_*) on the MI355X against the independent CPU reference
(tests/track_reference.py: the recursion of include/scvx.h in numpy, float64 and longdouble; the closed loop driven through the C
oracle -- or tests/aero_torque_reference.py for the torque models -- substep by substep).

Bounds, none of them taken from the device:
  * gains: with e_ref = the largest difference between the float64 and the longdouble reference gains of the case, the device must be
    within max(16 e_ref, K n 2^-52 max|L|) of the longdouble gains.  The first term lets the device's other summation order and fma
    contraction cost one more decimal digit than numpy's own rounding on the same data; the second is the textbook forward error of K
    chained n-term dot products and keeps the bound from collapsing where numpy happens to be exact (or where longdouble is no wider
    than double).  The same for P0 with max|P0|.
  * cost identity (z0' P0 z0 = the cost summed along the closed loop), evaluated on the host with the device's own L and P0: relative
    mismatch within max(16 x the mismatch of the float64 reference's own L and P0 on the case, K n 2^-52).
  * closed loop, reference gains fed to both sides: K * 1e-12 * A_cl -- one K2-sized difference per segment carried with the
    sensitivity A_cl the REFERENCE closed loop shows (track_reference.sensitivity, start perturbed by 1e-9); G_* columns times
    flight_reference.g_lipschitz; ufly times max(1, max|L|).
Every comparison prints its figures before it asserts.
"""
from dataclasses import replace

import numpy as np
import pytest

import flight_reference as fr
import track_reference as tr
from test_gpu_flight import _case, _compare, _flyable, _problems

pytestmark = pytest.mark.gpu

MODELS = ["exo", "aero", "aero+fins", "aero+fins+torque"]
WEIGHTS = [(1.0, 1.0, 100.0), (1.0, 1e-2, 1e4), (10.0, 1.0, 1e6)]
EPS = 2.0 ** -52
FLYABLE = dict(mdry=0.55, nuTol=1e-6, delTol=1e-3, imax=40, tf_guess=8.0)


def _gain_bounds(deriv, K, w):
    """(longdouble gains, P0, bound on the gains, bound on P0, the float64 reference's cost-identity mismatch) of a case"""
    L64, P64 = tr.gains(deriv, K, *w)
    Lld, Pld = tr.gains(deriv, K, *w, dtype=np.longdouble)
    n = L64.shape[-1]
    eL, eP = float(np.abs(L64 - Lld).max()), float(np.abs(P64 - Pld).max())
    bL = max(16.0 * eL, K * n * EPS * float(np.abs(Lld).max()))
    bP = max(16.0 * eP, K * n * EPS * float(np.abs(Pld).max()))
    return Lld, Pld, bL, bP, eL, eP, tr.cost_identity(deriv, K, L64, P64, *w)


def _check_gains(tag, deriv, K, w, L, P0):
    Lld, Pld, bL, bP, eL, eP, cid_ref = _gain_bounds(deriv, K, w)
    n = L.shape[-1]
    dL, dP = float(np.abs(L - Lld).max()), float(np.abs(P0 - Pld).max())
    cid = tr.cost_identity(deriv, K, L, P0, *w)
    bC = max(16.0 * cid_ref, K * n * EPS)
    print("%s weights %s: max|L| %.4g, gains device-vs-longdouble %.3e (float64 reference %.3e, bound %.3e); P0 %.3e (reference %.3e, "
          "bound %.3e); cost identity %.3e (reference %.3e, bound %.3e)"
          % (tag, w, np.abs(Lld).max(), dL, eL, bL, dP, eP, bP, cid, cid_ref, bC))
    assert np.isfinite(L).all() and np.isfinite(P0).all()
    assert dL <= bL, (tag, w, dL, bL)
    assert dP <= bP, (tag, w, dP, bP)
    assert cid <= bC, (tag, w, cid, bC)
    return bL


_PLANS = {}


def _flyable_plans(model, aero_tables):
    """B = 8 dispersed plans of the flyable variant of `model` after scvx_solve: (pp, po, dyn, par, x, u, sigma, status)"""
    if model not in _PLANS:
        import bench
        from successiveconvexification_amd.batch import ScvxBatch
        from successiveconvexification_amd.dynamics import IntegratorCache
        pp, po, dyn, par = _problems(model, aero_tables)
        pp, po = replace(pp, **FLYABLE), replace(po, **FLYABLE)
        par = dyn.Params(po, torque=True) if "torque" in model else dyn.Params(po)
        c = IntegratorCache(pp, npts=10)
        b = ScvxBatch(c, 8).init(bench.disperse_ics(pp, 0, 8, 7))
        st, it, _, _ = b.solve()
        _PLANS[model] = (pp, po, dyn, par) + b.trajectory() + (st,)
        b.close()
        c.close()
    return _PLANS[model]


@pytest.mark.parametrize("mfma", ["0", "1"])
@pytest.mark.parametrize("model", MODELS)
def test_gains_parity_unconverged_plans(model, mfma, aero_tables, monkeypatch):
    """both forms of the kernel's 14-deep products (SCVX_TRACK_MFMA, read at every launch), whichever is the default"""
    from successiveconvexification_amd.dynamics import IntegratorCache, linearize_batch, track_gains_batch
    monkeypatch.setenv("SCVX_TRACK_MFMA", mfma)
    pp, po, dyn, par, x, u, s = _case(model, aero_tables)
    c = IntegratorCache(pp, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (po.K + 1))
    for w in WEIGHTS:
        L, P0 = track_gains_batch(c, d, *w, cost=True)
        assert L.shape == (5, po.K, c.nu, 14 + c.nu)
        _check_gains("%s B = 5 unconverged, SCVX_TRACK_MFMA=%s" % (model, mfma), d, po.K, w, L, P0)
        assert np.array_equal(track_gains_batch(c, d, *w), L)       # without the cost output: the same gains
    c.close()


@pytest.mark.parametrize("model", MODELS)
def test_gains_parity_device_solved_plans_of_the_flyable_variant(model, aero_tables):
    from successiveconvexification_amd.dynamics import IntegratorCache, linearize_batch, track_gains_batch
    pp, po, dyn, par, x, u, s, st = _flyable_plans(model, aero_tables)
    print("%s flyable variant: statuses after scvx_solve %s" % (model, st.tolist()))
    if model == "exo":
        assert np.all(st == 0), st      # the variant test_gpu_flight.py converges; the other models' plans are used as they come out
    c = IntegratorCache(pp, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (po.K + 1))
    for w in WEIGHTS:
        L, P0 = track_gains_batch(c, d, *w, cost=True)
        _check_gains("%s B = 8 flyable" % model, d, po.K, w, L, P0)
    c.close()


@pytest.mark.parametrize("model", MODELS)
def test_zero_state_weights_zero_gains_and_the_shoot_flight(model, aero_tables):
    from successiveconvexification_amd.dynamics import IntegratorCache, flight_check_batch, linearize_batch, track_fly_batch, track_gains_batch
    pp, po, dyn, par, x, u, s = _case(model, aero_tables)
    c = IntegratorCache(pp, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (po.K + 1))
    L, P0 = track_gains_batch(c, d, 0.0, 1.0, 0.0, cost=True)
    assert not L.any() and not P0.any()
    t = track_fly_batch(c, x, u, s, L, dense=True)
    sh = flight_check_batch(c, x, u, s, mode="shoot", dense=True)
    A = fr.sensitivity(dyn, po, x, u, s, 10, 1e-9, par=par)
    bound = po.K * 1e-12 * A
    print("%s zero gains vs SHOOT: report bitwise %s, xfly bitwise %s, largest difference %.3e (bound %.3e)"
          % (model, np.array_equal(t.raw, sh.raw), np.array_equal(t.xfly, sh.xfly), np.abs(t.xfly - sh.xfly).max(), bound))
    assert t.mode == "track" and np.array_equal(t.ufly, u)
    assert float(np.abs(t.xfly - sh.xfly).max()) <= bound
    _compare("%s zero gains vs SHOOT" % model, t.raw, sh.raw, bound, po)
    c.close()


def _near_bound(po, cmd, bound):
    """trajectories with a node whose commanded thrust norm lies within `bound` of Tmin or Tmax"""
    return (np.minimum(np.abs(cmd - po.Tmin), np.abs(cmd - po.Tmax)) <= bound).any(axis=1)


def _closed_loop_parity(tag, c, po, dyn, par, x, u, s, L, dx0, nsub, clamp):
    from successiveconvexification_amd.dynamics import track_fly_batch
    flags = tr.CLAMP if clamp else 0
    dev = track_fly_batch(c, x, u, s, L, dx0, nsub=nsub, clamp=clamp, dense=True)
    ref, xref, uref, cmd = tr.fly(dyn, po, x, u, s, L, dx0, nsub, flags, par)
    A = tr.sensitivity(dyn, po, x, u, s, L, dx0, nsub, 1e-9, flags, par=par)
    bound = po.K * 1e-12 * A
    keep = np.ones(x.shape[0], bool)
    margin = float(np.minimum(np.abs(cmd - po.Tmin), np.abs(cmd - po.Tmax)).min())
    if clamp:
        keep = ~_near_bound(po, cmd, bound)
        assert (~keep).sum() <= 0.1 * x.shape[0], (tag, (~keep).sum())
        t = np.linalg.norm(dev.ufly[:, 1:, :3], axis=-1)
        assert t.min() >= po.Tmin * (1 - 4 * EPS) and t.max() <= po.Tmax * (1 + 4 * EPS), (t.min(), t.max())
    dxs, dus = float(np.abs(dev.xfly - xref)[keep].max()), float(np.abs(dev.ufly - uref)[keep].max())
    bu = bound * max(1.0, float(np.abs(L).max()))
    print("%s nsub %d clamp %s: A_cl %.3f, bound %.3e, xfly %.3e, ufly %.3e (bound %.3e), closest commanded norm to a thrust bound %.3e, "
          "excluded %d" % (tag, nsub, clamp, A, bound, dxs, dus, bu, margin, (~keep).sum()))
    assert np.array_equal(dev.xfly[:, 0], x[:, 0] + dx0) and np.array_equal(dev.ufly[:, 0], u[:, 0])
    assert dxs <= bound and dus <= bu
    _compare("%s nsub %d clamp %s" % (tag, nsub, clamp), dev.raw[keep], ref[keep], bound, po)
    return dev, ref


@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("nsub", [1, 4, 10])
@pytest.mark.parametrize("model", MODELS)
def test_closed_loop_parity(model, nsub, clamp, aero_tables):
    from successiveconvexification_amd.dynamics import IntegratorCache, linearize_batch
    from successiveconvexification_amd.montecarlo import disperse_handover
    pp, po, dyn, par, x, u, s = _case(model, aero_tables)
    c = IntegratorCache(pp, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (po.K + 1))
    L, _ = tr.gains(d, po.K)                                   # the REFERENCE's gains, fed to both sides
    dx0 = disperse_handover(x[:, 0], 0, x.shape[0], 20261016, frac_r=1e-3, frac_v=1e-3, rate=1e-3)
    _closed_loop_parity(model, c, po, dyn, par, x, u, s, L, dx0, nsub, clamp)
    c.close()


def test_closed_loop_on_the_golden_plans_beats_open_loop():
    """the oracle's converged plans through the device: parity, and the point of the feature -- the miss shrinks"""
    import os
    from conftest import GOLDEN
    from oracle import dynamics as od
    from successiveconvexification_amd.dynamics import IntegratorCache, linearize_batch, track_fly_batch, track_gains_batch
    from successiveconvexification_amd.montecarlo import disperse_handover
    g = np.load(os.path.join(GOLDEN, "oracle_flight_runs.npz"))
    pp, po = _flyable()
    par = od.Params(po)
    x, u, s = g["x"], g["u"], g["sigma"]
    c = IntegratorCache(pp, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (po.K + 1))
    L = track_gains_batch(c, d)
    _check_gains("golden plans", d, po.K, tr.DEFAULT_WEIGHTS, *track_gains_batch(c, d, cost=True))
    dx0 = disperse_handover(x[:, 0], 0, 2, 1, frac_r=1e-3, frac_v=1e-3, rate=1e-3)
    for clamp in (False, True):
        _closed_loop_parity("golden plans, device gains", c, po, od, par, x, u, s, L, dx0, 10, clamp)
    closed = track_fly_batch(c, x, u, s, L, dx0)
    opened = track_fly_batch(c, x, u, s, np.zeros_like(L), dx0)
    print("MISS_R open %s closed %s; MISS_V open %s closed %s" % (opened.MISS_R, closed.MISS_R, opened.MISS_V, closed.MISS_V))
    assert np.all(closed.MISS_R < opened.MISS_R) and np.all(closed.MISS_V < opened.MISS_V)
    c.close()


def test_batch_level_gains_fly_and_the_batch_is_untouched():
    import bench
    from oracle import dynamics as od
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache, linearize_batch, track_fly_batch, track_gains_batch
    from successiveconvexification_amd.montecarlo import disperse_handover
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
    # the stale-tile check: the batch's own tiles must be those of the iterate that converged
    _, d = linearize_batch(c, x, u, s, 1.0 / (K + 1))
    Lb, Pb = b.track_gains(cost=True)
    Lh, Ph = track_gains_batch(c, d, cost=True)
    bL = _check_gains("batch, converged plans", d, K, tr.DEFAULT_WEIGHTS, Lb, Pb)
    print("batch gains vs gains of a fresh linearisation: %.3e (bound %.3e), bitwise %s" % (np.abs(Lb - Lh).max(), bL, np.array_equal(Lb, Lh)))
    assert float(np.abs(Lb - Lh).max()) <= bL
    w = (1.0, 1e-2, 1e4)
    assert float(np.abs(b.track_gains(*w) - track_gains_batch(c, d, *w)).max()) <= _gain_bounds(d, K, w)[2]
    dx0 = disperse_handover(x[:, 0], 0, B, 5, frac_r=1e-3, frac_v=1e-3, rate=1e-3)
    for clamp in (False, True):
        rb = b.track(dx0, nsub=10, clamp=clamp, dense=True)
        rh = track_fly_batch(c, x, u, s, Lb, dx0, nsub=10, clamp=clamp, dense=True)
        assert np.array_equal(rb.raw, rh.raw) and np.array_equal(rb.xfly, rh.xfly) and np.array_equal(rb.ufly, rh.ufly)
    assert np.array_equal(b.track(dx0).raw, b.track(dx0, nsub=10).raw)        # nsub = 0 takes the context's
    shoot = b.flight_check(mode="shoot")
    closed, opened = b.track(dx0), b.track(dx0, q=0.0, qf=0.0)
    _compare("batch, zero state weights vs SHOOT", b.track(q=0.0, qf=0.0).raw, shoot.raw,
             K * 1e-12 * fr.sensitivity(od, po, x, u, s, 10, 1e-9), po)
    print("batch: MISS_R open %s closed %s" % (opened.MISS_R, closed.MISS_R))
    assert np.all(closed.MISS_R < opened.MISS_R)
    after = (b.trajectory_record(),) + b.scalars() + b.flags() + b.linearization()
    for a0, a1 in zip(before, after):
        assert np.array_equal(a0, a1, equal_nan=True)
    # float tiles: widened on load; the same tiles, widened on the host, through the context-level call
    b.set_linearization_f32(True)
    d32 = b.linearization()[1]
    assert np.array_equal(d32, d32.astype(np.float32).astype(np.float64)) and not np.array_equal(d32, d)
    L32, P32 = b.track_gains(cost=True)
    b32 = _check_gains("batch, float tiles", d32, K, tr.DEFAULT_WEIGHTS, L32, P32)
    L32h = track_gains_batch(c, d32)
    print("float tiles: batch vs host-widened %.3e (bound %.3e), bitwise %s" % (np.abs(L32 - L32h).max(), b32, np.array_equal(L32, L32h)))
    assert float(np.abs(L32 - L32h).max()) <= b32
    b.set_linearization_f32(False)
    assert np.array_equal(b.linearization()[1], before[-1])
    # a following solve_step equals, bit for bit, that of a twin batch never tracked
    r1, r2 = b.solve_step(), twin.solve_step()
    for a0, a1 in zip(r1 + (b.trajectory_record(),) + b.scalars(), r2 + (twin.trajectory_record(),) + twin.scalars()):
        assert np.array_equal(a0, a1, equal_nan=True)
    b.close(), twin.close(), c.close()


def test_arguments_are_checked():
    import ctypes as C
    from oracle import model as om
    from successiveconvexification_amd import _lib, sample_problems as sp
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache, _p, linearize_batch, track_fly_batch, track_gains_batch
    pp, po = sp.base_prob_scaled, om.base_prob_scaled()
    c = IntegratorCache(pp, npts=10)
    b = ScvxBatch(c, 5).init(om.disperse_ics(po, 5, 20261004))
    b.solve_step()
    x, u, s = b.trajectory()
    _, d = linearize_batch(c, x, u, s, 1.0 / (po.K + 1))
    L, h, K = c._L, c.handle, pp.K
    q, r, qf = np.ones(14), np.ones(3), np.full(14, 100.0)
    gain, rep = np.full((5, K, 3, 17), 7.0), np.full((5, 16), 7.0)
    err = lambda: L.scvx_last_error(h).decode()   # noqa: E731
    dev = lambda v: C.c_void_p(1) if v is not None else None   # noqa: E731  the checks come before any device pointer is used

    def neg(i):
        a = np.ones(14 if i != 1 else 3)
        a[1] = -1.0
        return a

    def bad_r(v):
        a = np.ones(3)
        a[2] = v
        return a

    gcases = [(dict(B=0), "B >= 1"), (dict(K=K - 1), "K must equal"), (dict(d=None), "null"), (dict(q=None), "null"),
              (dict(r=None), "null"), (dict(qf=None), "null"), (dict(gain=None), "null"), (dict(r=bad_r(0.0)), "r must be"),
              (dict(r=bad_r(-1.0)), "r must be"), (dict(r=bad_r(np.nan)), "r must be"), (dict(r=bad_r(np.inf)), "r must be"),
              (dict(q=neg(0)), "q and qf"), (dict(qf=neg(2)), "q and qf"), (dict(q=np.full(14, np.nan)), "q and qf"),
              (dict(qf=np.full(14, np.inf)), "q and qf")]
    for kw, word in gcases:
        v = dict(B=5, K=K, d=d, q=q, r=r, qf=qf, gain=gain)
        v.update(kw)
        pw = [None if v[n] is None else _p(np.ascontiguousarray(v[n])) for n in ("q", "r", "qf")]
        a_host = [v["B"], v["K"], None if v["d"] is None else _p(d)] + pw + [None if v["gain"] is None else _p(gain), None]
        a_dev = [v["B"], v["K"], dev(v["d"])] + pw + [dev(v["gain"]), None]
        for fn, a in ((L.scvx_track_gains_f64_host, a_host), (L.scvx_track_gains_f64, a_dev)):
            assert fn(h, *a) == -1, (kw, fn)
            assert word in err(), (kw, err())
    assert np.all(gain == 7.0)                                   # nothing ran
    fcases = [(dict(B=0), "B >= 1"), (dict(K=K + 1), "K must equal"), (dict(nsub=0), "nsub"), (dict(nsub=1001), "nsub"),
              (dict(flags=2), "flags"), (dict(flags=-1), "flags"), (dict(x=None), "null"), (dict(u=None), "null"), (dict(s=None), "null"),
              (dict(gain=None), "null"), (dict(rep=None), "null")]
    for kw, word in fcases:
        v = dict(B=5, K=K, x=x, u=u, s=s, gain=gain, nsub=10, flags=0, rep=rep)
        v.update(kw)
        ptr = lambda n: None if v[n] is None else _p(v[n])   # noqa: E731
        a_host = [v["B"], v["K"], ptr("x"), ptr("u"), ptr("s"), ptr("gain"), None, v["nsub"], v["flags"], ptr("rep"), None, None]
        a_dev = [v["B"], v["K"]] + [dev(v[n]) for n in ("x", "u", "s", "gain")] + [None, v["nsub"], v["flags"], dev(v["rep"]), None, None]
        for fn, a in ((L.scvx_track_fly_f64_host, a_host), (L.scvx_track_fly_f64, a_dev)):
            assert fn(h, *a) == -1, (kw, fn)
            assert word in err(), (kw, err())
    assert np.all(rep == 7.0)
    # batch level
    bh = b.handle
    assert L.scvx_batch_track_gains(bh, _p(q), _p(bad_r(0.0)), _p(qf), _p(gain), None) == -1 and "r must be" in err()
    assert L.scvx_batch_track_gains(bh, None, _p(r), _p(qf), _p(gain), None) == -1 and "null" in err()
    assert L.scvx_batch_track_fly(bh, _p(q), _p(r), _p(neg(2)), None, 0, 0, _p(rep), None, None) == -1 and "q and qf" in err()
    assert L.scvx_batch_track_fly(bh, _p(q), _p(r), _p(qf), None, -1, 0, _p(rep), None, None) == -1 and "nsub" in err()
    assert L.scvx_batch_track_fly(bh, _p(q), _p(r), _p(qf), None, 0, 4, _p(rep), None, None) == -1 and "flags" in err()
    assert np.all(gain == 7.0) and np.all(rep == 7.0)
    with pytest.raises(_lib.ScvxError, match="r must be"):
        b.track_gains(r=0.0)
    with pytest.raises(ValueError):
        b.track(dx0=np.zeros((4, 14)))
    with pytest.raises(ValueError):
        track_gains_batch(c, d[:, :, :20])
    with pytest.raises(ValueError):
        track_fly_batch(c, x, u, s, gain[:, :, :, :16])
    # any output of the batch forms may be left out; the context and the batch still work
    assert L.scvx_batch_track_gains(bh, _p(q), _p(r), _p(qf), None, None) == 0
    assert L.scvx_batch_track_fly(bh, _p(q), _p(r), _p(qf), None, 0, 0, None, None, None) == 0
    assert np.array_equal(b.track().raw, track_fly_batch(c, x, u, s, b.track_gains()).raw)
    b.close(), c.close()


def test_rocketland_track_single_problem():
    from successiveconvexification_amd import rocketland as rl, sample_problems as sp
    from successiveconvexification_amd.dynamics import IntegratorCache
    p = sp.base_prob_scaled
    c = IntegratorCache(p, npts=10)
    ip = rl.create_initial(p, c)
    ip, _, _ = rl.solve_step(ip, c)
    dx0 = np.zeros(14)
    dx0[1:4] = 1e-3
    r = rl.track(ip, c, dx0, dense=True)
    assert len(r) == 1 and r.mode == "track" and r.xfly.shape == (1, p.K + 1, 14) and r.ufly.shape == (1, p.K + 1, 3)
    rb = ip.model.track(dx0[None], dense=True)
    assert np.array_equal(r.raw, rb.raw) and np.array_equal(r.ufly, rb.ufly)
    c.close()


def test_at_size_headline_batch():
    import bench
    from oracle import dynamics as od, model as om
    from successiveconvexification_amd import montecarlo as mc, sample_problems as sp
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache, track_fly_batch
    pp, po = sp.base_prob_scaled, om.base_prob_scaled()
    B, K = 8192, pp.K
    c = IntegratorCache(pp, npts=10)
    b = ScvxBatch(c, B).init(bench.disperse_ics(pp, 0, B, 20261004))
    for _ in range(2):
        b.solve_step_async()
    status, _, _ = b.flags()
    x, u, s = b.trajectory()
    d = b.linearization()[1]
    dx0 = mc.disperse_handover(x[:, 0], 0, B, 20261016, frac_r=1e-3, frac_v=1e-3, rate=1e-3)
    L, P0 = b.track_gains(cost=True)
    closed = b.track(dx0, dense=True)
    shoot = b.flight_check(mode="shoot")
    cols = [i for i in range(16) if i not in (13, 14)]
    fine = np.isfinite(shoot.raw[:, cols]).all(axis=1)
    print("B = 8192: %d rows with a finite open-loop report; closed loop finite in %d of them" %
          (fine.sum(), np.isfinite(closed.raw[fine][:, cols]).all(axis=1).sum()))
    assert fine.sum() >= 16
    assert np.isfinite(closed.raw[fine][:, cols]).all() and np.isfinite(L[fine]).all() and np.isfinite(closed.ufly[fine]).all()
    assert np.all(np.isneginf(closed.raw[:, 13:15]))
    rows = np.random.default_rng(20261016).choice(np.flatnonzero(fine), 16, replace=False)
    par = od.Params(po)
    _check_gains("B = 8192 rows %s" % rows.tolist(), d[rows], K, tr.DEFAULT_WEIGHTS, L[rows], P0[rows])
    # the rows of the big launch are what a launch of their own gives
    own = track_fly_batch(c, x[rows], u[rows], s[rows], L[rows], dx0[rows], dense=True)
    assert np.array_equal(own.raw, closed.raw[rows]) and np.array_equal(own.ufly, closed.ufly[rows])
    # and the closed loop against the reference, the reference's gains fed to both
    Lref, _ = tr.gains(d[rows], K)
    _closed_loop_parity("B = 8192 rows", c, po, od, par, x[rows], u[rows], s[rows], Lref, dx0[rows], 10, False)
    summ = mc.flight_summary(closed, status, 0.0)
    assert sum(summ["counts"].values()) == B == summ["n"]
    b.close(), c.close()
