"""The sampled closed-loop dispersion on the MI355X at horizons other than the K = 3 and K = 50 its own modules pin it at: K = 1 (the
node loop's only trip is first and last, the prefetch of "the next node's" A and Kf never runs, the three code sites that write pathv
produce every row there is, one Philox group per stream), K = 2 (the prefetch runs once, the two trips touch), K = 100 (groups no
K <= 50 case forms, a K + 1 stride of 101 in the order statistics), and the batch-level forms at K = 64 and 100 and at K = BATCH_SMALL.

The cases are those of tests/horizon_cases.py (B = 3; K = 100 the dispersed batch after three solve_steps), the tiles the device's own
linearize_batch, the gains the REFERENCE's, fed to both sides.  S = 5 where the CPU chain flies along, S = 130 (three blocks per plan,
the last with two live lanes) for the bitwise and the reduction checks; nsub = 2 at the short horizons and 4 at K = 100.

No tolerance here is new: every comparison goes through the helper of the module that pins the same call at K = 3 and 50, with that
helper's bound, computed from the reference and printed before the assert --
  * test_gpu_mc: _bitwise_against_the_flyer (equality; dx0 within 14 eps |C0| |xi0|), _impulse_parity (K 1e-12 A_cl, A_cl of the
    reference chain), _check_reduction (2 S eps max|v|, 4 S eps max|e|^2, the counts and maxima exact);
  * test_gpu_mc_nav: _no_error_is_the_old_call and _bitwise_against_the_flyer_on_estimates (equality), _recursion_against_the_reference
    (8 x the float64 recursion's own distance from the longdouble one + 4 ulp of max|eps|), _impulse_parity (K 1e-12 A_cl);
  * test_gpu_mc_rng: _fused_is_the_old_call (equality), _dump_against_the_reference (8 x the float64 twin's distance + 4 ulp);
  * test_gpu_mc_vehicle: _parity (K 1e-12 A_cl, theta exact), _null_veh_is_the_plain_call (equality);
  * test_gpu_mc_quantiles: _against_the_flyer (MASS equal, the others 4 eps of their terms), _against_the_chain (K 1e-12 A_cl times
    the Lipschitz constant of each function), _check_flightq / _check_pathq (`==`, identical NaN positions).
What test_mc_horizons_cpu.py finds exact on the references is asserted bit for bit here: the K = 1 dump is the leading groups of the
K = 100 dump, and navfed[..., :j, :] of the K-horizon call is the j-horizon call on the inputs cut to j nodes.

pathv at K = 1: the _host entry points stage their outputs through device buffers of their own, so a sentinel in the host array could
not show what the kernel wrote; instead all (K + 1) 5 = 10 rows per plan are compared with the flyer's (the five functions of both
nodes; the thrust row of node 0 against |ubar_0|).

The count comparison of OUT_LO / OUT_HI in the two _impulse_parity helpers is conditional (taken where the commanded norm's distance to
a thrust bound exceeds bound max(1, |L|max)); this module keeps its own tally and its last test asserts that at most one third of the
plans of any (model, K) leave it out.  Nothing else is left out: _against_the_flyer skips THRUST under the clamp by construction (ufly
is the clamped control there), and the same launches are checked without the clamp.

Recorded on the first run on one MI355X (98 tests, 12 s; worst error / bound per group, K = 1 / 2 / 100; profiles/mc_horizons_parity.md):
every bitwise check held (flyer truth-fed and on estimates, no-error = old call, fused = dump-fed, NULL veh, K = 1 dump = leading groups
of the K = 100 dump, truncation of navfed, batch = context on double tiles, device draws = dump-fed on float tiles, pathq / flightq);
dx0 0.112 / 0.107 / 0.089; impulses against the CPU chain, landing 2.1e-4 / 3.6e-4 / 5.2e-5 (errors 2.2e-16, 1.9e-14, 7.1e-15 under
bounds 1.0e-12, 5.4e-11, 1.4e-10), on an estimate 3.1e-4 / 5.1e-4 / 4.5e-5; report columns (test_gpu_flight._compare) states 4.3e-4 /
2.4e-4 / 5.1e-5, G columns 2.1e-3 / 4.0e-4 / 1.9e-5; error recursion 0.12 / 0.14 / 0.19; dump against the longdouble reference 0.48 (K = 1) and 0.50 (K = 100); vehicle errors 3.2e-4 / 3.1e-4 / 4.6e-5; pathv against the
flyer GLIDE 0.12 / 0.15 / 0.38, TILT 0.24 / 0.23 / 0.25, RATE 0.22 / 0.24 / 0.25, THRUST 0.24 / 0.24 / 0.33, MASS equal; pathv against
the chain 2.1e-4 / 7.7e-5; reduction MEAN 0.058 / - / 0.016, xmean 9.4e-3 / - / 9.0e-3, xcov 6.1e-3 / - / 4.7e-3.  The count equality was
made for every plan of every (call, model, K): nothing left out.  BATCH_SMALL: K = 4, 8 and 9 all pass flyable_batch's status
assertion, on double and on float tiles, so 4 is used.
What the run found: test_gpu_mc._check_reduction recovered the two counts as OUT * S * K, a double that need not divide back to the
same fraction (3520 / 13000 does not; 703 of the 6501 possible counts at K = 50 do not either) -- the helper now takes the integers the
fractions stand for and still compares exactly.  No kernel or staging defect was found.
"""
from dataclasses import replace

import numpy as np
import pytest

import cov_reference as cr
import horizon_cases as hc
import test_gpu_mc as tgm
import test_gpu_mc_nav as tgn
import test_gpu_mc_quantiles as tgq
import test_gpu_mc_rng as tgr
import test_gpu_mc_vehicle as tgv
import track_reference as tr
from test_gpu_mc import _same

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
BATCH_SMALL = 4      # the smallest horizon at which horizon_cases.flyable_batch's own status assertion holds (4, 8, 9 were to be tried in turn)
BITWISE_MODELS = ("exo", hc.FLIGHT_ONLY_MODEL)
NAV_CASES = [(model, K, m) for model in hc.MODELS for K in hc.MC_HORIZONS for m in (0, 3, 14) if not (K == hc.LONG and m == 14 and model != "exo")]
VEH_CASES = [(model, K) for model in hc.MODELS for K in hc.MC_HORIZONS] + [(hc.FLIGHT_ONLY_MODEL, K) for K in hc.MC_SHORT]
W = np.full(14, 1e-8)
W[0] = 0.0
_SETUP = {}
_COUNT = {}          # (call, model, K) -> [plans that took the count equality, plans that left it out]


def _setup(model, K, aero_tables):
    """(pp, po, dyn, par, x, u, sigma, the device's tiles d, the reference's gains at the default weights, S0)"""
    key = (model, K)
    if key not in _SETUP:
        from successiveconvexification_amd.dynamics import IntegratorCache, linearize_batch
        pp, po, dyn, par, x, u, s = hc.case(model, K, aero_tables, device=True)
        c = IntegratorCache(pp, npts=10)
        _, d = linearize_batch(c, x, u, s, 1.0 / (K + 1))
        c.close()
        assert np.isfinite(d).all()
        S0 = np.stack([cr.handover_s0(x[b, 0])[0] for b in range(hc.B)])
        _SETUP[key] = (pp, po, dyn, par, x, u, s, d, tr.gains(d, K)[0], S0)
    return _SETUP[key]


def _context(pp):
    from successiveconvexification_amd.dynamics import IntegratorCache
    return IntegratorCache(pp, npts=10)


def _tally(call, model, K, taken):
    t = _COUNT.setdefault((call, model, K), [0, 0])
    t[0] += sum(bool(v) for v in taken)
    t[1] += sum(not v for v in taken)


# ---- 2a: the plain call -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", hc.MC_HORIZONS)
@pytest.mark.parametrize("model", BITWISE_MODELS)
def test_bitwise_against_the_flyer(model, K, aero_tables):
    pp, po, dyn, par, x, u, s, d, L, S0 = _setup(model, K, aero_tables)
    c = _context(pp)
    tgm._bitwise_against_the_flyer("%s K = %d" % (model, K), c, x, u, s, L, S0, hc.MC_S_BLOCKS, 5, hc.mc_nsub(K))
    c.close()


@pytest.mark.parametrize("K", hc.MC_HORIZONS)
@pytest.mark.parametrize("model", hc.MODELS)
def test_impulses_against_the_cpu_chain(model, K, aero_tables):
    pp, po, dyn, par, x, u, s, d, L, S0 = _setup(model, K, aero_tables)
    c = _context(pp)
    _tally("plain", model, K, tgm._impulse_parity("%s K = %d" % (model, K), c, po, dyn, par, x, u, s, hc.mc_nsub(K), hc.MC_S, hc.MC_SEED))
    c.close()


@pytest.mark.parametrize("K", [1, hc.LONG])
def test_reduction_against_numpy_on_the_dense_outputs(K, aero_tables):
    from successiveconvexification_amd.dynamics import track_fly_batch, track_mc_batch
    pp, po, dyn, par, x, u, s, d, L, S0 = _setup("aero+fins", K, aero_tables)
    c = _context(pp)
    S, nsub = hc.MC_S_BLOCKS, hc.mc_nsub(K)
    base = track_mc_batch(c, x, u, s, L, S0, S, seed=3, nsub=nsub, dense=True)
    # no clamp, tol = 0: the commanded norms are the applied ones of the flyer, counted the way test_gpu_mc.py counts them
    t = track_fly_batch(c, cr.rep(x, S), cr.rep(u, S), cr.rep(s, S), cr.rep(L, S), base.dx0.reshape(hc.B * S, 14), nsub=nsub, dense=True)
    tn = np.linalg.norm(t.ufly[:, :, :3], axis=-1).reshape(hc.B, S, K + 1)
    counts = [(int((tn[b, :, 1:] < po.Tmin).sum()), int((tn[b, :, 1:] > po.Tmax).sum())) for b in range(hc.B)]
    print("aero+fins K = %d: commanded node controls outside [Tmin, Tmax], %d starts x %d nodes: %s" % (K, S, K, counts))
    tgm._check_reduction("aero+fins K = %d, no noise" % K, po, x, base, 0.0, counts)
    assert tgm._all_same(base, track_mc_batch(c, x, u, s, L, S0, S, seed=3, nsub=nsub, dense=True))     # two launches: bit for bit
    tol = max(0.0, float(np.median(base.flights[0, :, 11])))              # a threshold some flights' G_TMIN pass and some do not
    for clamp in (False, True):
        noisy = track_mc_batch(c, x, u, s, L, S0, S, seed=3, w=W, nsub=nsub, clamp=clamp, tol=tol, dense=True)
        tgm._check_reduction("aero+fins K = %d, w > 0, clamp %s, tol %.3e" % (K, clamp, tol), po, x, noisy, tol)
    r64 = track_mc_batch(c, x, u, s, L, S0, 64, seed=3, w=W, nsub=nsub, dense=True)
    r65 = track_mc_batch(c, x, u, s, L, S0, 65, seed=3, w=W, nsub=nsub, dense=True)
    assert _same(r64.flights, r65.flights[:, :64]) and _same(r64.xland, r65.xland[:, :64])
    tgm._check_reduction("aero+fins K = %d S = 64" % K, po, x, r64, 0.0)
    tgm._check_reduction("aero+fins K = %d S = 65" % K, po, x, r65, 0.0)
    c.close()


# ---- 2b: on an estimate -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", hc.MC_HORIZONS)
@pytest.mark.parametrize("model", hc.MODELS)
def test_no_estimate_error_is_the_old_call(model, K, aero_tables):
    pp, po, dyn, par, x, u, s, d, L, S0 = _setup(model, K, aero_tables)
    c = _context(pp)
    tgn._no_error_is_the_old_call("%s K = %d" % (model, K), c, x, u, s, d, L, S0, hc.MC_S_BLOCKS, 7, hc.mc_nsub(K))
    c.close()


def _ms(model, K):
    return tuple(m for mdl, k, m in NAV_CASES if (mdl, k) == (model, K))


@pytest.mark.parametrize("K", hc.MC_HORIZONS)
@pytest.mark.parametrize("model", hc.MODELS)
def test_error_recursion_against_the_reference(model, K, aero_tables):
    pp, po, dyn, par, x, u, s, d, L, S0 = _setup(model, K, aero_tables)
    c = _context(pp)
    tgn._recursion_against_the_reference("%s K = %d" % (model, K), c, x, u, s, d, L, S0, hc.MC_S, 21, hc.mc_nsub(K), ms=_ms(model, K))
    c.close()


@pytest.mark.parametrize("K", hc.MC_HORIZONS)
@pytest.mark.parametrize("model", hc.MODELS)
def test_bitwise_against_the_flyer_on_estimates(model, K, aero_tables):
    pp, po, dyn, par, x, u, s, d, L, S0 = _setup(model, K, aero_tables)
    c = _context(pp)
    for m in _ms(model, K):
        tgn._bitwise_against_the_flyer_on_estimates("%s K = %d" % (model, K), c, x, u, s, d, L, S0, m, hc.MC_S_BLOCKS, 5, hc.mc_nsub(K))
    c.close()


@pytest.mark.parametrize("model,K,m", NAV_CASES)
def test_impulses_on_an_estimate_against_the_cpu_chain(model, K, m, aero_tables):
    pp, po, dyn, par, x, u, s, d, L, S0 = _setup(model, K, aero_tables)
    c = _context(pp)
    _tally("on an estimate", model, K,
           tgn._impulse_parity("%s K = %d" % (model, K), c, po, dyn, par, x, u, s, m, hc.mc_nsub(K), hc.MC_S, hc.MC_SEED))
    c.close()


@pytest.mark.parametrize("K", [2, hc.LONG])
@pytest.mark.parametrize("model", hc.MODELS)
def test_truncation_of_the_error_recursion_on_the_device(model, K, aero_tables):
    """navfed[..., :j, :] of the K-horizon call is the j-horizon call fed the tiles, filter gains and uploaded draws cut to j nodes
    (contexts of the two horizons): bit for bit, as test_mc_horizons_cpu.py finds it on the reference.  The flights of the short call
    are not looked at -- its plan is a cut of a longer one"""
    from successiveconvexification_amd.dynamics import nav_cov_batch, track_mc_nav_batch
    from successiveconvexification_amd.montecarlo import mc_draws, mc_nav_draws
    pp, po, dyn, par, x, u, s, d, L, S0 = _setup(model, K, aero_tables)
    cK = _context(pp)
    N0 = 0.25 * S0
    S = 70
    xi0, eta = mc_draws(S, K, 21, noise=True)
    for m in _ms(model, K):
        H, rm = tgn._model(m, x[0, 0])
        xin, nud = mc_nav_draws(S, K, m, 21)
        kf = nav_cov_batch(cK, x, u, d, L, np.zeros((hc.B, 14, 14)), N0, H, rm, W, dense=("kf",)).kf if m else None
        whole = track_mc_nav_batch(cK, x, u, s, d, L, S0, N0, H, rm, S, w=W, kf=kf, nsub=2, dense=("navfed", "navK"), draws=(xi0, eta, xin, nud))
        assert np.isfinite(whole.navfed).all() and whole.navfed.shape == (hc.B, S, K, 14)
        for j in (1, 2):
            if j >= K:
                continue
            cj = _context(replace(pp, K=j))
            cut = lambda a: None if a is None else np.ascontiguousarray(a[:, :j])   # noqa: E731
            part = track_mc_nav_batch(cj, np.ascontiguousarray(x[:, :j + 1]), np.ascontiguousarray(u[:, :j + 1]), s, cut(d), cut(L), S0, N0, H,
                                      rm, S, w=W, kf=cut(kf), nsub=2, dense=("navfed", "navK"), draws=(xi0, cut(eta), xin, cut(nud)))
            same = _same(part.navfed, whole.navfed[:, :, :j])
            print("%s K = %d -> %d m %d: navfed of the first %d nodes bitwise %s (largest difference %.3e)"
                  % (model, K, j, m, j, same, np.abs(part.navfed - whole.navfed[:, :, :j]).max()))
            assert same
            cj.close()
    cK.close()


# ---- 2c: the draws made on the device -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [None, 3])
@pytest.mark.parametrize("K", hc.MC_HORIZONS)
@pytest.mark.parametrize("model", BITWISE_MODELS)
def test_fused_flights_are_the_old_call_fed_the_dump(model, K, m, aero_tables):
    pp, po, dyn, par, x, u, s, d, L, S0 = _setup(model, K, aero_tables)
    c = _context(pp)
    tgr._fused_is_the_old_call("%s K = %d m %s" % (model, K, m), c, po, x, u, s, d, L, S0, m, (1, 65, 130), (1, 3), hc.mc_nsub(K))
    c.close()


def test_dumped_draws_at_k1_and_k100(aero_tables):
    """the dumps of K = 1 and K = 100 against the longdouble reference (test_gpu_mc_rng.py's rule), and the K = 1 dump as the leading
    groups of the K = 100 dump, bit for bit"""
    from successiveconvexification_amd.dynamics import mc_draws_device_batch
    c = _context(_setup("exo", 1, aero_tables)[0])          # the draws do not depend on the context's horizon: K is an argument
    s_lo = 64
    ref = tgr._reference(s_lo, hc.LONG)
    for P in (1, 3):
        ld, tw = ref[P]
        for S in (1, 65, 130):
            d1, r1 = tgr._dump_against_the_reference(c, ld, tw, s_lo, P, S, 1)
            dL, rL = tgr._dump_against_the_reference(c, ld, tw, s_lo, P, S, hc.LONG)
            lead = {n: _same(d1[n], dL[n] if n in ("xi0", "xin") else dL[n][..., :1, :]) for n in ("xi0", "eta", "xin", "nud")}
            print("P %d S %d: largest error / (8 x twin's + 4 ulp) K = 1 %.3f, K = 100 %.3f; K = 1 dump bitwise the leading groups %s"
                  % (P, S, r1, rL, lead))
            assert dL["eta"].shape[-2:] == (hc.LONG, 14) and d1["nud"].shape[-2:] == (1, 14)
            assert all(lead.values()), lead
    d2 = mc_draws_device_batch(c, 65, K=2, seed=tgr.SEED, sample_lo=s_lo, plans=3)
    assert _same(d2["eta"], dL["eta"][:, :65, :2]) and _same(d2["nud"], dL["nud"][:, :65, :2])
    c.close()


# ---- 2d: vehicle errors -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,K", VEH_CASES)
def test_vehicle_errors_against_the_cpu_chain(model, K, aero_tables):
    """the flag combinations of test_gpu_mc_vehicle.test_against_the_cpu_chain_at_k_3, one nav= case per horizon"""
    pp, po, dyn, par, x, u, s, d, L, S0 = _setup(model, K, aero_tables)
    c = _context(pp)
    nsub, tag = hc.mc_nsub(K), "%s K = %d" % (model, K)
    H, rm = tgn._model(3, x[0, 0])
    if "torque" in model:
        worst = tgv._parity(tag, c, po, dyn, par, x, u, s, L, S0, 2, nsub, True, True, zero_mean=False)
    else:
        worst = max(tgv._parity(tag, c, po, dyn, par, x, u, s, L, S0, b, nsub, b == 2, b == 0) for b in (0, 2))
        worst = max(worst, tgv._parity(tag, c, po, dyn, par, x, u, s, L, S0, 1, nsub, False, True, nav=(0.25 * S0, H, rm)))
    print("%s: vehicle errors against the CPU chain, worst landing error / bound %.3e" % (tag, worst))
    c.close()


@pytest.mark.parametrize("K", [1, hc.LONG])
@pytest.mark.parametrize("model", BITWISE_MODELS)
def test_null_veh_is_the_plain_call(model, K, aero_tables, monkeypatch):
    pp, po, dyn, par, x, u, s, d, L, S0 = _setup(model, K, aero_tables)
    c = _context(pp)
    for m in (None, 3):
        tgv._null_veh_is_the_plain_call("%s K = %d m %s" % (model, K, m), monkeypatch, c, x, u, s, L, S0, m, (1, 3), (1, 65, 130), hc.mc_nsub(K))
    c.close()


# ---- 2e: path values and quantiles --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", hc.MC_HORIZONS)
@pytest.mark.parametrize("model", BITWISE_MODELS)
def test_pathv_against_the_flyer_truth_fed(model, K, aero_tables):
    from successiveconvexification_amd.dynamics import track_fly_batch, track_mc_batch
    pp, po, dyn, par, x, u, s, d, L, S0 = _setup(model, K, aero_tables)
    c = _context(pp)
    B, S, nsub = hc.B, hc.MC_S_BLOCKS, hc.mc_nsub(K)
    for clamp in (False, True):
        tag = "%s K = %d S %d clamp %s" % (model, K, S, clamp)
        r = track_mc_batch(c, x, u, s, L, S0, S, seed=5, nsub=nsub, clamp=clamp, dense=("flights", "dx0", "pathv"), quantiles=tgq.PROBS,
                           per_node=True)
        assert r.pathv.shape == (B, K + 1, 5, S) and r.pathq.shape == (B, K + 1, 5, len(tgq.PROBS))
        t = track_fly_batch(c, cr.rep(x, S), cr.rep(u, S), cr.rep(s, S), cr.rep(L, S), r.dx0.reshape(B * S, 14), nsub=nsub, clamp=clamp, dense=True)
        assert np.isfinite(t.xfly).all()
        # every row: the five functions at every node but THRUST at node 0 against the flyer's states and controls, THRUST at node 0
        # against |ubar_0|.  At K = 1 these are all (K + 1) 5 = 10 rows per plan, written from three code sites
        tgq._against_the_flyer(tag, po, x, u, r.pathv, t.xfly, t.ufly, clamp)
        assert np.isfinite(r.pathv).all()
        assert _same(r.pathv[:, 0, 0, :], (x[:, 0, 0][:, None] + r.dx0[:, :, 0]))
        tgq._check_pathq(tag, r)
        tgq._check_flightq(tag, r)
    c.close()


@pytest.mark.parametrize("K", hc.MC_SHORT)
@pytest.mark.parametrize("model", hc.MODELS)
def test_pathv_with_clamp_and_noise_against_the_cpu_chain(model, K, aero_tables):
    pp, po, dyn, par, x, u, s, d, L, S0 = _setup(model, K, aero_tables)
    c = _context(pp)
    tgq._against_the_chain("%s K = %d" % (model, K), c, po, dyn, par, x, u, s, hc.mc_nsub(K), hc.MC_S, hc.MC_SEED)
    c.close()


@pytest.mark.parametrize("K", hc.MC_HORIZONS)
def test_flightq_and_pathq_are_the_order_statistics_of_the_dense_outputs(K, aero_tables):
    """with the clamp and the noise, truth-fed and on an estimate, device draws too: B (K + 1) 5 rows of S values each"""
    from successiveconvexification_amd.dynamics import track_mc_batch
    pp, po, dyn, par, x, u, s, d, L, S0 = _setup("aero+fins", K, aero_tables)
    c = _context(pp)
    H, rm = tgn._model(3, x[0, 0])
    for S in (hc.MC_S, 65, hc.MC_S_BLOCKS):
        for nav in (None, (0.25 * S0, H, rm)):
            for rng in ("host", "device"):
                tag = "aero+fins K = %d S %d nav %s rng %s" % (K, S, nav is not None, rng)
                r = track_mc_batch(c, x, u, s, L, S0, S, seed=11, w=W, nsub=hc.mc_nsub(K), clamp=True, tol=1e-6, nav=nav, rng=rng,
                                   dense=("flights", "pathv"), quantiles=tgq.PROBS, per_node=True)
                assert r.pathv.shape == (hc.B, K + 1, 5, S)
                tgq._check_flightq(tag, r)
                tgq._check_pathq(tag, r)
                lean = track_mc_batch(c, x, u, s, L, S0, S, seed=11, w=W, nsub=hc.mc_nsub(K), clamp=True, tol=1e-6, nav=nav, rng=rng,
                                      quantiles=tgq.PROBS, per_node=True)                     # no dense output: the workspace
                assert lean.pathv is None and _same(lean.q, r.q) and _same(lean.pathq, r.pathq) and _same(lean.raw, r.raw), tag
    c.close()


# ---- 2f: the batch-level forms ------------------------------------------------------------------------------------------------------
def _batch_inputs(c, b):
    from successiveconvexification_amd.montecarlo import vehicle_errors
    x, u, s = b.trajectory()
    sd = np.zeros(14)
    sd[1:7] = 1e-3 * np.abs(x[0, 0, 1:7])
    sd[7:] = 1e-3
    H, rm = tgn._model(3, x[0, 0])
    return x, u, s, sd, np.full(14, 1e-9), (0.5 * sd, H, rm), vehicle_errors(thrust=2e-3, misalign=1e-3, isp=3e-3)


@pytest.mark.parametrize("K", [BATCH_SMALL, 64, hc.LONG])
def test_batch_level_calls_are_the_context_level_ones(K):
    """double tiles: ScvxBatch.track_mc plain, with nav= and with vehicle= is the context-level call on b.trajectory(), the batch's own
    tiles and gains (and, on an estimate, the filter gains of its own navigation()), bit for bit, with the host's draws and with the
    device's; margins_from_mc sets exactly montecarlo.margins_from_quantiles of the pathq of the same launch; the batch comes back
    untouched.  K = BATCH_SMALL = 4 is the smallest horizon at which horizon_cases.flyable_batch's status assertion holds."""
    from successiveconvexification_amd.dynamics import track_mc_batch, track_mc_nav_batch
    from successiveconvexification_amd.montecarlo import margins_from_quantiles
    c, b = hc.flyable_batch(K)
    state = lambda: (b.trajectory_record(),) + b.scalars() + b.flags() + b.linearization()   # noqa: E731
    before = state()
    x, u, s, sd, w, nav, veh = _batch_inputs(c, b)
    d, L = b.linearization()[1], b.track_gains()
    assert x.shape == (2, K + 1, 14) and L.shape == (2, K, 3, 17) and np.isfinite(L).all()
    S = 70
    kf = b.navigation(sd, nav[0], nav[1], nav[2], w=w, dense=("kf",)).kf
    for nv in (None, nav):
        for vh in (None, veh):
            for rng in ("host", "device"):
                dn = ("flights", "xland", "dx0", "pathv") + (("navfed", "navK") if nv else ()) + (("theta",) if vh else ())
                kw = dict(seed=4, w=w, nsub=4, clamp=True, tol=1e-6, quantiles=tgq.PROBS, per_node=True, rng=rng, sample_lo=64, vehicle=vh, dense=dn)
                rb = b.track_mc(sd, samples=S, nav=nv, **kw)
                if nv:
                    rh = track_mc_nav_batch(c, x, u, s, d, L, sd, nv[0], nv[1], nv[2], S, kf=kf, **kw)
                else:
                    rh = track_mc_batch(c, x, u, s, L, sd, S, **kw)
                names = (tgr.OLD_NAV if nv else tgr.OLD) + (("theta",) if vh else ())
                same = {n: tgr._eq(getattr(rb, n), getattr(rh, n)) for n in names}
                print("K = %d batch, nav %s vehicle %s rng %s: bitwise the context-level call %s" % (K, nv is not None, vh is not None, rng, all(same.values())))
                assert all(same.values()), same
                assert rb.pathv.shape == (2, K + 1, 5, S) and rb.N_BAD.sum() == 0
                tgq._check_pathq("K = %d batch" % K, rb)
                tgq._check_flightq("K = %d batch" % K, rb)
    for a0, a1 in zip(before, state()):
        assert _same(a0, a1)
    # the back-offs: test_gpu_mc_quantiles.test_margins_from_mc_sets_what_margins_from_quantiles_says at this horizon
    for nv in (None, nav):
        b.set_thrust_margins(None, None).set_path_margins()
        rep, lo, hi, pm = b.margins_from_mc(sd, samples=256, seed=3, nav=nv, nsub=4)
        assert rep.pathq.shape == (2, K + 1, 5, 2) and rep.ranks.tolist() == [0, 255]
        want = margins_from_quantiles(c.problem, x, u, rep.pathq[..., 0], rep.pathq[..., 1], "all", 0.25)
        got = b.thrust_margins() + (b.path_margins(),)
        print("K = %d margins_from_mc nav %s: back-offs up to lo %s hi %s tilt %s" % (K, nv is not None, lo.max(axis=1), hi.max(axis=1), pm[:, :, 2].max(axis=1)))
        for a0, a1, a2 in zip(got, want, (lo, hi, pm)):
            assert np.array_equal(a0, a1) and np.array_equal(a0, a2)
        assert lo.shape == (2, K + 1) and pm.shape == (2, K + 1, 4)
    b.set_thrust_margins(None, None).set_path_margins()
    b.close(), c.close()


@pytest.mark.parametrize("K", [BATCH_SMALL, 64, hc.LONG])
def test_batch_level_calls_on_float_tiles(K):
    """float tiles (DS = float in the NAV instantiations), by the rule of test_gpu_mc_rng.test_batch_calls_margins_and_float_tiles and
    test_gpu_mc_vehicle.test_batch_calls_float_tiles_and_back_offs: the device-draw batch call is bitwise the batch call fed the dump,
    plain, on an estimate and with vehicle errors (sp a power of two, mu = 0: zeta = theta / sp exactly); the batch comes back untouched"""
    c, b = hc.flyable_batch(K, tiles_f32=True)
    state = lambda: (b.trajectory_record(),) + b.scalars() + b.flags() + b.linearization()   # noqa: E731
    before = state()
    x, u, s, sd, w, nav, _ = _batch_inputs(c, b)
    S = 70
    xi0, eta, xin, nud = tgr._dump(c, S, K, 4, True, 3)
    vp = (np.zeros(6), np.array([2.0 ** -9, 2.0 ** -10, 2.0 ** -10, 2.0 ** -8, 0.0, 0.0]))
    for nv in (None, nav):
        for vh in (None, vp):
            dn = ("flights", "xland", "dx0", "pathv") + (("navfed", "navK") if nv else ()) + (("theta",) if vh else ())
            k0 = dict(seed=4, w=w, nsub=4, clamp=True, tol=1e-6, quantiles=tgq.PROBS, per_node=True, dense=dn, nav=nv)
            f_new = b.track_mc(sd, samples=S, rng="device", vehicle=vh, **k0)
            vo = None if vh is None else vh + (np.where(vh[1] > 0, f_new.theta[0] / np.where(vh[1] > 0, vh[1], 1.0), 0.0),)
            f_old = b.track_mc(sd, draws=(xi0, eta) + ((xin, nud) if nv else ()), vehicle=vo, **k0)
            names = (tgr.OLD_NAV if nv else tgr.OLD) + (("theta",) if vh else ())
            same = {n: tgr._eq(getattr(f_old, n), getattr(f_new, n)) for n in names}
            print("K = %d float tiles through the batch call, nav %s vehicle %s: bitwise %s" % (K, nv is not None, vh is not None, all(same.values())))
            assert all(same.values()), same
            assert f_new.pathv.shape == (2, K + 1, 5, S) and f_new.N_BAD.sum() == 0
            tgq._check_pathq("K = %d float tiles" % K, f_new)
    # the tiles are the float ones: the same batch on double tiles flies another estimate
    r32 = b.track_mc(sd, samples=S, seed=4, w=w, nsub=4, nav=nav, dense=("navK",))
    for a0, a1 in zip(before, state()):
        assert _same(a0, a1)
    b.set_linearization_f32(False)
    assert not _same(r32.navK, b.track_mc(sd, samples=S, seed=4, w=w, nsub=4, nav=nav, dense=("navK",)).navK)
    b.close(), c.close()


# ---- 2g ------------------------------------------------------------------------------------------------------------------------------
def test_count_comparisons_left_out_stay_below_a_third():
    """runs after the parity tests of this module: the OUT_LO / OUT_HI comparisons the two _impulse_parity helpers made and left out, per
    (call, model, K).  No other comparison of this module is conditional"""
    for (call, model, K), (made, left) in sorted(_COUNT.items()):
        print("%-14s %-10s K = %3d: count equality made for %d plans, left out for %d" % (call, model, K, made, left))
    assert _COUNT
    for key, (made, left) in _COUNT.items():
        assert 3 * left <= made + left, key
