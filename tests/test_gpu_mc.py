"""Sampled closed-loop dispersion (scvx_track_mc_f64 / scvx_batch_track_mc) on the MI355X: bit for bit against the existing flyer
(scvx_track_fly_f64) where there is no noise, against the CPU chain with impulses (tests/mc_reference.py, the C oracle substep by
substep) where there is, against numpy on the dense outputs of the same launch for the reduction, and against the device's own
covariance analysis WITH w for the statistics.

Bounds, none of them taken from the device:
  * no noise: equality.  dx0 against C0 @ xi0: 14 eps (|C0| |xi0|), the forward error of a 14-term dot product.
  * impulses against the CPU chain: K * 1e-12 * A_cl, test_gpu_track.py's closed-loop bound, with A_cl the sensitivity the REFERENCE
    chain (impulses included) shows; G_* columns times flight_reference.g_lipschitz.
  * reduction: MAX_*, P_*, OUT_*, N_BAD exact; MEAN_* and xmean 2 S eps max|value|; xcov 4 S eps max_s |e_s|_inf^2, the summation bound
    of the two accumulated sums.
  * statistics: six standard errors per entry (cov_reference.mc_check's bound).
Every comparison prints its figures before it asserts.
"""
import ctypes as C
import os

import numpy as np
import pytest

import cov_reference as cr
import mc_reference as mr
import track_reference as tr
from conftest import GOLDEN
from test_gpu_flight import _case, _compare, _flyable

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
_G = {}


def _golden():
    """(pp, po, x, u, s) of the two plans the oracle converges on"""
    if not _G:
        g = np.load(os.path.join(GOLDEN, "oracle_flight_runs.npz"))
        _G["v"] = _flyable() + (g["x"], g["u"], g["sigma"])
    return _G["v"]


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _all_same(r0, r1):
    return all(_same(getattr(r0, n), getattr(r1, n)) for n in ("raw", "xmean", "xcov", "flights", "xland", "dx0"))


def _bitwise_against_the_flyer(tag, c, x, u, s, L, S0, S, seed, nsub=10):
    from successiveconvexification_amd.dynamics import track_fly_batch, track_mc_batch
    from successiveconvexification_amd.montecarlo import handover_factor, mc_draws
    B, K = x.shape[0], x.shape[1] - 1
    xi0, _ = mc_draws(S, K, seed)
    for clamp in (False, True):
        r = track_mc_batch(c, x, u, s, L, S0, S, seed=seed, nsub=nsub, clamp=clamp, dense=True)
        assert r.flights.shape == (B, S, 16) and r.xland.shape == (B, S, 14) and r.dx0.shape == (B, S, 14)
        t = track_fly_batch(c, cr.rep(x, S), cr.rep(u, S), cr.rep(s, S), cr.rep(L, S), r.dx0.reshape(B * S, 14), nsub=nsub, clamp=clamp,
                            dense=True)
        fl, xl = r.flights.reshape(B * S, 16), r.xland.reshape(B * S, 14)
        print("%s S %d clamp %s: flights bitwise %s (largest difference %.3e), xland bitwise %s"
              % (tag, S, clamp, _same(fl, t.raw), np.nanmax(np.abs(np.nan_to_num(fl - t.raw, posinf=0, neginf=0))), _same(xl, t.xfly[:, K])))
        assert np.isfinite(fl[:, 0]).all()
        assert _same(fl, t.raw)
        assert _same(xl, t.xfly[:, K])
        if clamp:
            tn = np.linalg.norm(t.ufly[:, 1:, :3], axis=-1)
            print("%s: %d of %d applied node controls sit on a thrust bound" % (tag, ((tn <= c.problem.Tmin * (1 + 4 * EPS)) | (tn >= c.problem.Tmax * (1 - 4 * EPS))).sum(), tn.size))
        lean = track_mc_batch(c, x, u, s, L, S0, S, seed=seed, nsub=nsub, clamp=clamp)
        assert _same(lean.raw, r.raw) and _same(lean.xcov, r.xcov) and lean.flights is None and lean.dx0 is None
    C0 = np.stack([handover_factor(cr.s0_full(S0, B)[b]) for b in range(B)])
    ref = np.einsum("bij,sj->bsi", C0, xi0)
    bound = 14 * EPS * np.einsum("bij,sj->bsi", np.abs(C0), np.abs(xi0))
    err = np.abs(r.dx0 - ref)
    print("%s: dx0 vs C0 @ xi0, largest error / bound %.3f" % (tag, float((err / np.where(bound > 0, bound, 1.0)).max())))
    assert np.all(err <= bound)


def test_bitwise_against_the_flyer_on_the_golden_plans():
    """B = 3 (the two golden plans and plan 0 again with another S0), S = 130: three blocks per plan, the last with two live lanes"""
    from successiveconvexification_amd.dynamics import IntegratorCache, linearize_batch, track_gains_batch
    pp, po, x, u, s = _golden()
    c = IntegratorCache(pp, npts=10)
    x3, u3, s3 = x[[0, 1, 0]], u[[0, 1, 0]], s[[0, 1, 0]]
    _, d = linearize_batch(c, x3, u3, s3, 1.0 / (po.K + 1))
    L = track_gains_batch(c, d)
    S0 = np.stack([cr.handover_s0(x[0, 0])[0], cr.handover_s0(x[1, 0])[0], cr.handover_s0(x[0, 0], seed=1, size=3e-3)[0]])
    _bitwise_against_the_flyer("golden plans", c, x3, u3, s3, L, S0, 130, 5)
    c.close()


def test_bitwise_against_the_flyer_on_unconverged_torque_plans(aero_tables):
    from successiveconvexification_amd.dynamics import IntegratorCache, linearize_batch, track_gains_batch
    pp, po, dyn, par, x, u, s = _case("aero+fins+torque", aero_tables)
    c = IntegratorCache(pp, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (po.K + 1))
    L = track_gains_batch(c, d)
    S0 = np.stack([cr.handover_s0(x[b, 0])[0] for b in range(x.shape[0])])
    _bitwise_against_the_flyer("aero+fins+torque B = 5 unconverged", c, x, u, s, L, S0, 130, 6)
    c.close()


def _impulse_parity(tag, c, po, dyn, par, x, u, s, nsub, S, seed):
    from successiveconvexification_amd.dynamics import linearize_batch, track_mc_batch
    from successiveconvexification_amd.montecarlo import handover_factor, mc_draws
    B, K = x.shape[0], po.K
    _, d = linearize_batch(c, x, u, s, 1.0 / (K + 1))
    L, _ = tr.gains(d, K)                                          # the REFERENCE's gains, fed to both sides
    S0 = np.stack([cr.handover_s0(x[b, 0])[0] for b in range(B)])
    w = np.full(14, 1e-8)
    w[0] = 0.0
    xi0, eta = mc_draws(S, K, seed, noise=True)
    dev = track_mc_batch(c, x, u, s, L, S0, S, seed=seed, w=w, nsub=nsub, dense=True)
    quiet = track_mc_batch(c, x, u, s, L, S0, S, seed=seed, nsub=nsub, dense=True)
    assert not _same(dev.xland, quiet.xland)                       # the impulses are felt
    imp = eta * np.sqrt(w)
    taken = []                                                     # per plan: was the count comparison below made
    for b in range(B):
        dx0 = xi0 @ handover_factor(S0[b]).T
        ref, xref, _, cmd = mr.fly_plan(dyn, po, x[b], u[b], s[b], L[b], dx0, nsub, 0, imp, par)
        A = mr.sensitivity(dyn, po, x[b], u[b], s[b], L[b], dx0, nsub, 1e-9, 0, imp, par=par)
        bound = K * 1e-12 * A
        dxl = float(np.abs(dev.xland[b] - xref[:, -1]).max())
        print("%s plan %d nsub %d: A_cl %.3f, bound %.3e, xland %.3e, dx0 %.3e" % (tag, b, nsub, A, bound, dxl, np.abs(dev.dx0[b] - dx0).max()))
        assert dxl <= bound
        _compare("%s plan %d nsub %d" % (tag, b, nsub), dev.flights[b], ref, bound, po)
        lo, hi = mr.out_counts(cmd, po.Tmin, po.Tmax)
        margin = float(np.minimum(np.abs(cmd - po.Tmin), np.abs(cmd - po.Tmax)).min())
        print("    commanded norms outside the band: reference %d / %d, device %.1f / %.1f (closest to a bound %.3e)"
              % (lo, hi, dev.OUT_LO[b] * S * K, dev.OUT_HI[b] * S * K, margin))
        taken.append(margin > bound * max(1.0, float(np.abs(L).max())))
        if taken[-1]:
            assert dev.OUT_LO[b] == lo / (S * K) and dev.OUT_HI[b] == hi / (S * K)
    # eta all zeros, sw all zeros and no eta: one result, bit for bit
    for draws, wv in (((xi0, np.zeros_like(eta)), w), ((xi0, eta), np.zeros(14)), ((xi0, eta), 0.0), ((xi0, None), w)):
        z = track_mc_batch(c, x, u, s, L, S0, S, w=wv, nsub=nsub, dense=True, draws=draws)
        assert _all_same(z, quiet), (tag, wv)
    one = track_mc_batch(c, x, u, s, L, S0, 1, seed=seed, w=w, nsub=nsub, dense=True)
    assert one.flights.shape == (B, 1, 16) and not one.xcov.any() and np.all(one.S == 1)
    assert _same(one.flights[:, 0], dev.flights[:, 0]) and _same(one.xmean, one.xland[:, 0] - x[:, -1]) and _same(one.raw[:, :16], one.flights[:, 0])
    return taken


@pytest.mark.parametrize("model", ["exo", "aero+fins"])
def test_impulses_against_the_cpu_chain_at_a_short_horizon(model, aero_tables):
    import horizon_cases as hc
    from successiveconvexification_amd.dynamics import IntegratorCache
    pp, po, dyn, par, x, u, s = hc.case(model, 3, aero_tables)
    c = IntegratorCache(pp, npts=10)
    _impulse_parity("%s K = 3" % model, c, po, dyn, par, x, u, s, 2, 5, 31)
    c.close()


def test_impulses_against_the_cpu_chain_on_the_golden_plans():
    from oracle import dynamics as od
    from successiveconvexification_amd.dynamics import IntegratorCache
    pp, po, x, u, s = _golden()
    c = IntegratorCache(pp, npts=10)
    _impulse_parity("golden plans K = 50", c, po, od, od.Params(po), x, u, s, 10, 5, 32)
    c.close()


def _check_reduction(tag, po, x, rep, tol, counts=None):
    """the report of one launch against numpy on its own dense outputs"""
    B, S, _ = rep.flights.shape
    K = po.K
    I = mr.IDX
    for b in range(B):
        e = rep.xland[b] - x[b, -1]
        # without counts of the caller's: the integers the two fractions stand for (OUT * S * K itself need not come back to the same
        # double when divided again: 3520 / 13000 does not), which the exact comparison below then holds the report to
        lo, hi = counts[b] if counts is not None else (int(round(rep.OUT_LO[b] * S * K)), int(round(rep.OUT_HI[b] * S * K)))
        r, xm, xc = mr.reduce(rep.flights[b], e, lo, hi, K, tol)
        exact = list(range(16)) + list(range(32, 48))
        assert _same(rep.raw[b, exact], r[exact]), (tag, b, rep.raw[b, exact], r[exact])
        inf = np.isneginf(r[16:32])
        assert np.array_equal(inf, np.isneginf(rep.raw[b, 16:32]))
        vmax = np.abs(np.where(np.isfinite(rep.flights[b]), rep.flights[b], 0.0)).max(axis=0)
        em = np.abs(rep.raw[b, 16:32] - r[16:32])[~inf]
        bm = (2 * S * EPS * vmax)[~inf]
        emax = float(np.abs(e).max())
        ex, ec = np.abs(rep.xmean[b] - xm), np.abs(rep.xcov[b] - xc)
        print("%s plan %d: MEAN error / bound %.3f, xmean %.3e (bound %.3e), xcov %.3e (bound %.3e), P_ANY %.4f OUT_LO %.5f OUT_HI %.5f"
              % (tag, b, float((em / bm).max()), ex.max(), 2 * S * EPS * emax, ec.max(), 4 * S * EPS * emax ** 2, rep.P_ANY[b],
                 rep.OUT_LO[b], rep.OUT_HI[b]))
        assert np.all(em <= bm)
        assert np.all(ex <= 2 * S * EPS * np.abs(e).max(axis=0))
        assert ec.max() <= 4 * S * EPS * emax ** 2
        assert _same(rep.xcov[b], rep.xcov[b].T)
        assert rep.raw[b, I["S"]] == S and rep.raw[b, I["N_BAD"]] == 0


def test_reduction_against_numpy_on_the_dense_outputs():
    from successiveconvexification_amd.dynamics import IntegratorCache, linearize_batch, track_fly_batch, track_gains_batch, track_mc_batch
    pp, po, x, u, s = _golden()
    K, S = po.K, 130
    c = IntegratorCache(pp, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (K + 1))
    L = track_gains_batch(c, d)
    S0 = np.stack([cr.handover_s0(x[b, 0])[0] for b in range(2)])
    base = track_mc_batch(c, x, u, s, L, S0, S, seed=3, nsub=10, dense=True)
    # the base golden plans, no clamp, tol = 0: the commanded norms are the applied ones, counted the way test_gpu_margins.py counts
    t = track_fly_batch(c, cr.rep(x, S), cr.rep(u, S), cr.rep(s, S), cr.rep(L, S), base.dx0.reshape(2 * S, 14), nsub=10, dense=True)
    tn = np.linalg.norm(t.ufly[:, :, :3], axis=-1).reshape(2, S, K + 1)
    counts = [(int((tn[b, :, 1:] < pp.Tmin).sum()), int((tn[b, :, 1:] > pp.Tmax).sum())) for b in range(2)]
    print("commanded node controls k = 1..K outside [Tmin, Tmax], %d starts x %d nodes: below %s, above %s; node 0 (the plan's own): %s"
          % (S, K, [n[0] for n in counts], [n[1] for n in counts], ((tn[:, :, 0] < pp.Tmin) | (tn[:, :, 0] > pp.Tmax)).sum(axis=1)))
    assert sum(counts[0]) > 0
    _check_reduction("golden plans, no noise", po, x, base, 0.0, counts)
    again = track_mc_batch(c, x, u, s, L, S0, S, seed=3, nsub=10, dense=True)
    assert _all_same(base, again)                                   # two launches: bit for bit
    w = np.full(14, 1e-8)
    w[0] = 0.0
    tol = max(0.0, float(np.median(base.flights[0, :, 11])))               # a threshold some flights' G_TMIN pass and some do not
    for clamp in (False, True):
        noisy = track_mc_batch(c, x, u, s, L, S0, S, seed=3, w=w, nsub=10, clamp=clamp, tol=tol, dense=True)
        _check_reduction("golden plans, w > 0, clamp %s, tol %.3e" % (clamp, tol), po, x, noisy, tol)
        assert 0.0 < noisy.P_TMIN[0] < 1.0 or clamp
    # S = 64 and S = 65: the common prefix of the flights, one block and two
    r64 = track_mc_batch(c, x, u, s, L, S0, 64, seed=3, w=w, nsub=10, dense=True)
    r65 = track_mc_batch(c, x, u, s, L, S0, 65, seed=3, w=w, nsub=10, dense=True)
    assert _same(r64.flights, r65.flights[:, :64]) and _same(r64.xland, r65.xland[:, :64])
    _check_reduction("S = 64", po, x, r64, 0.0)
    _check_reduction("S = 65", po, x, r65, 0.0)
    assert not _same(r64.xmean, r65.xmean)
    c.close()


def test_a_nan_poisons_only_its_plan():
    from successiveconvexification_amd.dynamics import IntegratorCache, linearize_batch, track_gains_batch, track_mc_batch
    pp, po, x, u, s = _golden()
    x3, u3, s3 = x[[0, 1, 0]], u[[0, 1, 0]], s[[0, 1, 0]]
    c = IntegratorCache(pp, npts=10)
    _, d = linearize_batch(c, x3, u3, s3, 1.0 / (po.K + 1))
    L = track_gains_batch(c, d)
    S0 = np.stack([cr.handover_s0(x3[b, 0])[0] for b in range(3)])
    S = 70
    good = track_mc_batch(c, x3, u3, s3, L, S0, S, seed=9, nsub=10, dense=True)
    Ln = L.copy()
    Ln[1, 20, 1, 3] = np.nan
    for tag, bad, row in (("gain", track_mc_batch(c, x3, u3, s3, Ln, S0, S, seed=9, nsub=10, dense=True), 1),):
        I = mr.IDX
        print("NaN in the %s of plan %d: N_BAD %s, MAX_GAP %s, P_ANY %s" % (tag, row, bad.N_BAD, bad.MAX_GAP, bad.P_ANY))
        assert bad.N_BAD[row] == S and np.isnan(bad.raw[row, [I["MAX_GAP"], I["MEAN_GAP"], I["MAX_MISS_R"], I["MEAN_G_GLIDE"]]]).all()
        assert np.isnan(bad.xmean[row]).any() and np.isnan(bad.xcov[row]).any() and np.isnan(bad.flights[row, :, 0]).all()
        assert bad.P_ANY[row] <= 1.0 and bad.S[row] == S
        others = [b for b in range(3) if b != row]
        for n in ("raw", "xmean", "xcov", "flights", "xland", "dx0"):
            assert _same(getattr(bad, n)[others], getattr(good, n)[others]), n
    xn = x3.copy()
    xn[2, 30, 5] = np.inf                                           # a non-finite plan value
    bad = track_mc_batch(c, xn, u3, s3, L, S0, S, seed=9, nsub=10, dense=True)
    assert bad.N_BAD[2] == S and np.all(bad.N_BAD[:2] == 0) and _same(bad.raw[:2], good.raw[:2]) and _same(bad.xcov[:2], good.xcov[:2])
    c.close()


def test_process_noise_on_the_device_within_six_standard_errors():
    """the CPU check's inputs and S (test_mc_cpu.w_case), xcov from the device against the device's covariance analysis with w"""
    from test_mc_cpu import W_SAMPLES, W_SEED, w_case
    from successiveconvexification_amd.dynamics import IntegratorCache, cov_propagate_batch, linearize_batch, track_gains_batch, track_mc_batch
    p, par, x, u, s, d_ref, L_ref, S0, w, covK_ref = w_case()
    pp, po = _flyable()
    c = IntegratorCache(pp, npts=10)
    sl = slice(0, 1)
    _, d = linearize_batch(c, x[sl], u[sl], s[sl], 1.0 / (po.K + 1))
    L = track_gains_batch(c, d)
    covK = cov_propagate_batch(c, x[sl], u[sl], d, L, S0[None], w, dense=("covK",)).covK[0]
    r = track_mc_batch(c, x[sl], u[sl], s[sl], L, S0, W_SAMPLES, seed=W_SEED, w=w, nsub=10)
    worst, over = mr.se_check(r.xcov[0], covK[:14, :14], W_SAMPLES)
    quiet = track_mc_batch(c, x[sl], u[sl], s[sl], L, S0, W_SAMPLES, seed=W_SEED, nsub=10)
    worst0, over0 = mr.se_check(quiet.xcov[0], covK[:14, :14], W_SAMPLES)
    print("device, plan 0, S = %d: worst entry of xcov %.2f standard errors, %d over 6 (without impulses: %.2f, %d over 6); device covK "
          "vs the reference's %.3e" % (W_SAMPLES, worst, over, worst0, over0, np.abs(covK - covK_ref).max()))
    assert r.N_BAD[0] == 0 and r.S[0] == W_SAMPLES
    assert over == 0, (worst, over)
    assert over0 > 0
    c.close()


def test_batch_level_call_and_the_batch_is_untouched():
    import bench
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache, track_mc_batch
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
    for clamp in (False, True):
        rb = b.track_mc(sd, samples=70, seed=4, w=w, clamp=clamp, tol=1e-6, dense=True)
        rh = track_mc_batch(c, x, u, s, b.track_gains(), sd, 70, seed=4, w=w, nsub=10, clamp=clamp, tol=1e-6, dense=True)
        assert _all_same(rb, rh) and rb.flights.shape == (B, 70, 16)
    print("batch: P_ANY %s OUT_LO %s MEAN_MISS_R %s" % (rb.P_ANY, rb.OUT_LO, rb.MEAN_MISS_R))
    lean = b.track_mc(sd, samples=70, seed=4, w=w, clamp=True, tol=1e-6)
    assert _same(lean.raw, rb.raw) and lean.flights is None
    S0 = np.stack([np.diag(sd * sd)] * B)
    assert _same(b.track_mc(S0, samples=70, seed=4).raw, b.track_mc(sd, samples=70, seed=4).raw)
    assert _same(b.track_mc(sd, samples=70, seed=4, q=1.0, r=1e-2, qf=1e4).raw,
                 track_mc_batch(c, x, u, s, b.track_gains(1.0, 1e-2, 1e4), sd, 70, seed=4).raw)
    # float tiles: the gains come from the widened tiles
    b.set_linearization_f32(True)
    r32 = b.track_mc(sd, samples=70, seed=4, w=w, dense=True)
    h32 = track_mc_batch(c, x, u, s, b.track_gains(), sd, 70, seed=4, w=w, nsub=10, dense=True)
    assert _all_same(r32, h32) and not _same(r32.raw, b.track_mc(sd, samples=70, seed=4, w=w, clamp=True).raw)
    b.set_linearization_f32(False)
    after = (b.trajectory_record(),) + b.scalars() + b.flags() + b.linearization()
    for a0, a1 in zip(before, after):
        assert _same(a0, a1)
    b.close(), c.close()


def test_rocketland_track_mc_single_problem():
    from successiveconvexification_amd import rocketland as rl, sample_problems as sp
    from successiveconvexification_amd.dynamics import IntegratorCache
    p = sp.base_prob_scaled
    c = IntegratorCache(p, npts=10)
    ip = rl.create_initial(p, c)
    ip, _, _ = rl.solve_step(ip, c)
    sd = np.zeros(14)
    sd[1:7] = 1e-3
    r = rl.track_mc(ip, c, sd, samples=66, seed=2, w=1e-9, dense=True)
    assert len(r) == 1 and r.flights.shape == (1, 66, 16) and r.S[0] == 66 and np.isfinite(r.raw[0, :13]).all()
    rb = ip.model.track_mc(sd, samples=66, seed=2, w=1e-9, dense=True)
    assert _same(r.raw[0], rb.raw[0]) and _same(r.flights[0], rb.flights[0]) and _same(r.xcov[0], rb.xcov[0])
    with pytest.raises(ValueError):
        rl.track_mc(ip, c)
    c.close()


def test_arguments_are_checked():
    from successiveconvexification_amd import _lib
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache, _p, linearize_batch, track_gains_batch, track_mc_batch
    pp, po, x, u, s = _golden()
    c = IntegratorCache(pp, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (po.K + 1))
    gain = track_gains_batch(c, d)
    L, h, K, S = c._L, c.handle, pp.K, 4
    C0 = np.ascontiguousarray(np.stack([np.eye(14) * 1e-3] * 2))
    xi0, eta = np.zeros((S, 14)), np.zeros((S, K, 14))
    rep, xm, xc = np.full((2, 48), 7.0), np.full((2, 14), 7.0), np.full((2, 14, 14), 7.0)
    err = lambda: L.scvx_last_error(h).decode()   # noqa: E731
    dev = lambda v: C.c_void_p(1) if v is not None else None   # noqa: E731  the checks come before any device pointer is used

    def bad(v):
        a = np.zeros(14)
        a[3] = v
        return a

    cases = [(dict(S=0), "S >= 1"), (dict(B=0), "B"), (dict(K=K - 1), "K must equal"), (dict(nsub=0), "nsub"), (dict(nsub=1001), "nsub"),
             (dict(flags=2), "unknown flags"), (dict(sw=bad(-1.0)), "sw must be"), (dict(sw=bad(np.nan)), "sw must be"),
             (dict(sw=bad(np.inf)), "sw must be"), (dict(tol=-1.0), "tol must be"), (dict(tol=np.nan), "tol must be"),
             (dict(tol=np.inf), "tol must be"), (dict(eta=eta, sw=None), "eta without sw"), (dict(reserved=1), "reserved")]
    cases += [({n: None}, "null") for n in ("x", "u", "s", "gain", "C0", "xi0", "rep", "xm", "xc")]
    for kw, word in cases:
        v = dict(B=2, K=K, S=S, x=x, u=u, s=s, gain=gain, C0=C0, xi0=xi0, eta=None, sw=np.zeros(14), reserved=None, nsub=10, flags=0, tol=0.0,
                 rep=rep, xm=xm, xc=xc)
        v.update(kw)
        psw = None if v["sw"] is None else _p(np.ascontiguousarray(v["sw"]))
        res = None if v["reserved"] is None else C.c_void_p(v["reserved"])
        ptr = lambda n: None if v[n] is None else _p(v[n])   # noqa: E731
        tail = [psw, res, v["nsub"], v["flags"], v["tol"]]
        a_host = [v["B"], v["K"], v["S"]] + [ptr(n) for n in ("x", "u", "s", "gain", "C0", "xi0", "eta")] + tail + [ptr("rep"), ptr("xm"), ptr("xc"),
                                                                                                             None, None, None]
        a_dev = [v["B"], v["K"], v["S"]] + [dev(v[n]) for n in ("x", "u", "s", "gain", "C0", "xi0", "eta")] + tail + [dev(v["rep"]), dev(v["xm"]),
                                                                                                             dev(v["xc"]), None, None, None]
        for fn, a in ((L.scvx_track_mc_f64_host, a_host), (L.scvx_track_mc_f64, a_dev)):
            assert fn(h, *a) == -1, (kw, fn)
            assert word in err(), (kw, err())
    assert np.all(rep == 7.0) and np.all(xm == 7.0) and np.all(xc == 7.0)          # nothing ran
    b = ScvxBatch(c, 2).init(None)
    b.set_trajectory(x, u, s)
    q, r, qf = np.ones(14), np.ones(3), np.full(14, 100.0)
    call = lambda **kw: L.scvx_batch_track_mc(b.handle, kw.get("q", _p(q)), _p(kw.get("r", r)), _p(qf), kw.get("S", S), kw.get("C0", _p(C0)),   # noqa: E731
                                              _p(xi0), kw.get("eta", None), kw.get("sw", _p(np.zeros(14))), None, kw.get("nsub", 0),
                                              kw.get("flags", 0), kw.get("tol", 0.0), _p(rep), _p(xm), _p(xc), None, None, None)
    for kw, word in ((dict(S=0), "S >= 1"), (dict(C0=None), "null"), (dict(eta=_p(eta), sw=None), "eta without sw"), (dict(flags=4), "unknown flags"),
                     (dict(tol=-1e-9), "tol must be"), (dict(nsub=2000), "nsub"), (dict(r=np.zeros(3)), "r must be"), (dict(q=None), "null")):
        assert call(**kw) == -1 and word in err(), (kw, err())
    assert np.all(rep == 7.0)
    assert call() == 0 and not np.all(rep == 7.0) and np.all(rep[:, 45] == S)      # and with every argument in order it runs
    with pytest.raises(_lib.ScvxError, match="sw must be|w must be"):
        track_mc_batch(c, x, u, s, gain, np.full(14, 1e-3), 4, w=-1.0)
    with pytest.raises(ValueError):
        track_mc_batch(c, x, u, s, gain, np.full(14, 1e-3), 0)
    with pytest.raises(ValueError):
        track_mc_batch(c, x, u, s, gain[:, :, :, :16], np.full(14, 1e-3), 4)
    with pytest.raises(ValueError):
        track_mc_batch(c, x, u, s, gain, np.full(14, 1e-3), 4, draws=(xi0, eta[:, :3]))
    with pytest.raises(ValueError):
        b.track_mc(np.zeros((3, 14, 14)), samples=4)
    b.close(), c.close()
