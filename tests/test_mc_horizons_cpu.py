"""The CPU references of the sampled closed-loop dispersion (mc_reference, mc_nav_reference, mc_rng_reference, mc_vehicle_reference) at
the horizons of horizon_cases.MC_HORIZONS -- K = 1, 2 and 100 -- on tiles from oracle.dynamics.linearize and the gains of
track_reference.gains: they are vetted here before test_gpu_mc_horizons.py compares the device against them.  No GPU.  K = 100 is the
random-segments branch of horizon_cases.case (no device, no solve); aero+fins+torque runs at K = 1 and 2 only (its reference is driven
substep by substep in Python).

What holds EXACTLY on the references (np.array_equal, every model and horizon), and what the GPU file therefore asserts bit for bit:
  * without impulses mc_reference.fly_plan is track_reference.fly on the same dx0 (the rule of test_mc_cpu.py), and with theta = 0
    mc_vehicle_reference.chain is mc_reference.chain, impulses and clamp included (the rule of test_mc_vehicle_cpu.py);
  * draws: the counter layout is per node (group 1 + k of the sample's stream), so the K = 1 draws are the leading groups of the
    K = 100 draws of the same seed, plan and sample -- in the longdouble reference, in its float64 form and in the numpy twin
    (montecarlo.mc_draws_device / mc_nav_draws_device); the host draws (mc_draws, mc_nav_draws) are prefixes as well;
  * truncation of the error recursion: eps+_k and eps_k see only the tiles, filter gains and draws of the nodes before them, so
    navfed[..., :j, :] and before[..., :j + 1, :] of the K-horizon recursion are the j-horizon recursion on the inputs cut to j nodes,
    float64 and longdouble, m = 0, 3 and 14.  The filter gains are a FORWARD recursion (nav_reference.propagate; test_horizons_cpu.py
    shows kf of node 0 independent of the later nodes), so nothing here depends on later nodes and the check stays in both files.

The float64-to-longdouble distances of the error recursion printed here are the `own` term of the device's bound (8 x own + 4 ulp of
max|eps|, test_gpu_mc_nav._recursion_against_the_reference) at the same horizons.

The conditional count comparison: test_gpu_mc._impulse_parity compares OUT_LO / OUT_HI only where the commanded norm's distance to a
thrust bound exceeds bound * max(1, |L|max), bound = K 1e-12 A_cl.  count_condition() below forms that condition from the reference
alone, with that helper's own draws, noise level and seed; at least two thirds of the plans of every (model, K) must take the
equality.  (Without a device the K = 100 plans are the random segments, not the solved batch of the GPU file, and the tiles are the
oracle's: the GPU file keeps its own tally and asserts the same cap on it.)
"""
import numpy as np
import pytest

import cov_reference as cr
import horizon_cases as hc
import mc_nav_reference as mn
import mc_reference as mr
import mc_rng_reference as rr
import mc_vehicle_reference as vr
import nav_reference as nr
import track_reference as tr
from test_gpu_mc_nav import _model

NPTS = 4
SEED_DRAWS = 2 ** 63 + 5
CASES = [(m, K) for m in hc.MODELS for K in hc.MC_HORIZONS] + [(hc.FLIGHT_ONLY_MODEL, K) for K in hc.MC_SHORT]
W = np.full(14, 1e-8)
W[0] = 0.0
_TILES = {}


def _setup(model, K, aero_tables):
    """the case with its oracle tiles, the reference's gains and S0"""
    key = (model, K)
    if key not in _TILES:
        pp, po, dyn, par, x, u, s = hc.case(model, K, aero_tables)
        from oracle import dynamics as od
        # the oracle linearizes the model without the torque: for the torque model its tiles only supply SOME gains to both chains
        _, d = od.linearize(od.Params(po) if "torque" in model else par, x, u, s, 1.0 / (K + 1), NPTS)
        S0 = np.stack([cr.handover_s0(x[b, 0])[0] for b in range(x.shape[0])])
        _TILES[key] = (po, dyn, par, x, u, s, d, tr.gains(d, K)[0], S0)
    return _TILES[key]


def count_condition(po, dyn, par, x, u, s, L, S0, nsub, S, seed):
    """per plan, from the reference alone: does test_gpu_mc._impulse_parity take the OUT_LO / OUT_HI equality (that helper's draws, its
    w = 1e-8 and its rule margin > K 1e-12 A_cl max(1, |L|max)); also the margins and the bounds"""
    from successiveconvexification_amd.montecarlo import handover_factor, mc_draws
    K = po.K
    xi0, eta = mc_draws(S, K, seed, noise=True)
    imp = eta * np.sqrt(W)
    taken, margins, bounds = [], [], []
    for b in range(x.shape[0]):
        dx0 = xi0 @ handover_factor(S0[b]).T
        _, _, _, cmd = mr.fly_plan(dyn, po, x[b], u[b], s[b], L[b], dx0, nsub, 0, imp, par)
        A = mr.sensitivity(dyn, po, x[b], u[b], s[b], L[b], dx0, nsub, 1e-9, 0, imp, par=par)
        bound = K * 1e-12 * A
        margin = float(np.minimum(np.abs(cmd - po.Tmin), np.abs(cmd - po.Tmax)).min())
        taken.append(margin > bound * max(1.0, float(np.abs(L).max())))
        margins.append(margin)
        bounds.append(bound * max(1.0, float(np.abs(L).max())))
    return taken, margins, bounds


@pytest.mark.parametrize("model,K", CASES)
def test_no_noise_chain_is_the_tracked_flight_and_theta_zero_is_the_plain_chain(model, K, aero_tables):
    from successiveconvexification_amd.montecarlo import handover_factor, mc_draws
    po, dyn, par, x, u, s, d, L, S0 = _setup(model, K, aero_tables)
    nsub, S = hc.mc_nsub(K), hc.MC_S
    xi0, eta = mc_draws(S, K, hc.MC_SEED, noise=True)
    imp = eta * np.sqrt(W)
    bc = lambda a: np.broadcast_to(np.asarray(a, float), (S,) + np.shape(a))   # noqa: E731
    for b in range(hc.B):
        dx0 = xi0 @ handover_factor(S0[b]).T
        for flags in (0, tr.CLAMP):
            mine = mr.fly_plan(dyn, po, x[b], u[b], s[b], L[b], dx0, nsub, flags, None, par)
            ref = tr.fly(dyn, po, bc(x[b]), bc(u[b]), np.full(S, float(s[b])), bc(L[b]), dx0, nsub, flags, par)
            for a0, a1 in zip(ref, mine):
                assert np.array_equal(a0, a1, equal_nan=True), (model, K, b, flags)
            assert mine[1].shape == (S, K + 1, 14) and mine[3].shape == (S, K) and np.isfinite(mine[1]).all()
            assert np.array_equal(mine[1][:, 0], x[b, 0] + dx0) and np.array_equal(mine[2][:, 0], bc(u[b, 0]))
            # theta = 0 with impulses: the vehicle chain is the plain chain
            a = (dyn, par, po, bc(x[b]), bc(u[b]), np.full(S, float(s[b])), bc(L[b]), dx0, nsub)
            plain = mr.chain(*a, flags, imp)
            veh = vr.chain(*a, np.zeros((S, 6)), flags, imp)
            for a0, a1 in zip(plain, veh):
                assert np.array_equal(a0, a1, equal_nan=True), (model, K, b, flags)
            # the impulses are felt, and the last one reaches the landing row alone
            assert not np.array_equal(plain[2][:, -1], mine[1][:, -1])
            if K == 1:
                assert np.array_equal(plain[2][:, 1], mine[1][:, 1] + imp[:, 0]) and np.array_equal(plain[4], mine[3])
    print("%s K = %d nsub %d: fly_plan without impulses == track_reference.fly, vehicle chain at theta = 0 == mc_reference.chain, %d plans x "
          "%d flights, with and without the clamp" % (model, K, nsub, hc.B, S))


@pytest.mark.parametrize("K", hc.MC_HORIZONS)
@pytest.mark.parametrize("model", hc.MODELS)
def test_error_recursion_float64_against_longdouble_and_its_truncation(model, K, aero_tables):
    from successiveconvexification_amd.montecarlo import handover_factor, mc_draws, mc_nav_draws
    po, dyn, par, x, u, s, d, L, S0 = _setup(model, K, aero_tables)
    N0 = 0.25 * S0
    S = hc.MC_S
    eta = mc_draws(S, K, 21, noise=True)[1]
    for m in (0, 3, 14):
        H, rm = _model(m, x[0, 0])
        xin, nud = mc_nav_draws(S, K, m, 21)
        for wv, et in ((None, None), (W, eta)):
            kf = nr.propagate(d, K, L, np.zeros((hc.B, 14, 14)), N0, H, rm, wv)[1] if m else None
            for b in range(hc.B):
                CN = handover_factor(N0[b])
                a = (d[b], None if kf is None else kf[b], H, rm, CN, xin, nud, wv, et)
                f64, b64 = mn.eps_recursion(*a)
                fld, bld = mn.eps_recursion(*a, dtype=np.longdouble)
                own = float(max(np.abs(f64 - fld).max(), np.abs(b64 - bld).max()))
                big = float(np.abs(bld).max())
                print("%s K = %d plan %d m %d eta %s: max|eps| %.3e, float64 vs longdouble %.3e (%.1f ulp of max|eps|)"
                      % (model, K, b, m, et is not None, big, own, own / np.spacing(big)))
                assert f64.shape == (S, K, 14) and b64.shape == (S, K + 1, 14) and np.isfinite(f64).all() and np.isfinite(b64).all()
                assert np.isfinite(fld.astype(float)).all() and big > 0.0
                assert np.array_equal(b64[:, 0], xin @ CN.T)
                if m == 0:
                    assert np.array_equal(f64, b64[:, :K])                     # no measurement: nothing is corrected
                # truncation: the first j nodes are the j-horizon recursion on the inputs cut to j nodes
                for j in sorted({1, 2, K // 2} - {0}):
                    if j >= K:
                        continue
                    cut = (d[b, :j], None if kf is None else kf[b, :j], H, rm, CN, xin, None if nud is None else nud[:, :j], wv,
                           None if et is None else et[:, :j])
                    for dtype, (fK, bK) in ((np.float64, (f64, b64)), (np.longdouble, (fld, bld))):
                        fj, bj = mn.eps_recursion(*cut, dtype=dtype)
                        assert np.array_equal(fj, fK[:, :j]) and np.array_equal(bj, bK[:, :j + 1]), (model, K, b, m, j, dtype)
    # the filter gains themselves are a forward recursion: cut to j nodes they are the j-horizon gains, whatever follows
    H, rm = _model(14, x[0, 0])
    kK = nr.propagate(d, K, L, np.zeros((hc.B, 14, 14)), N0, H, rm, W)[1]
    for j in (1, 2):
        if j < K:
            assert np.array_equal(nr.propagate(d[:, :j], j, L[:, :j], np.zeros((hc.B, 14, 14)), N0, H, rm, W)[1], kK[:, :j])
    # ... and so are the host's draws
    for j in (1, 2):
        if j < K:
            assert np.array_equal(mc_nav_draws(S, j, 3, 21)[1], mc_nav_draws(S, K, 3, 21)[1][:, :j])
            assert np.array_equal(mc_draws(S, j, 21, noise=True)[1], eta[:, :j])


@pytest.mark.parametrize("s_lo", [0, 2 ** 33])
def test_k1_draws_are_the_leading_groups_of_the_k100_draws(s_lo):
    from successiveconvexification_amd.montecarlo import mc_draws_device, mc_nav_draws_device
    S = 7
    for plans in (None, (0, 1, 2)):
        for stream in (rr.STREAM_TRUTH, rr.STREAM_NAV):
            for dtype in (np.longdouble, np.float64):
                s1, n1 = rr.draws(SEED_DRAWS, stream, S, 1, s_lo, plans, dtype)
                sL, nL = rr.draws(SEED_DRAWS, stream, S, hc.LONG, s_lo, plans, dtype)
                assert n1.shape[-2:] == (1, 14) and nL.shape[-2:] == (hc.LONG, 14) and np.isfinite(nL.astype(float)).all()
                assert np.array_equal(s1, sL) and np.array_equal(n1, nL[:, :, :1]), (plans, stream, dtype)
                assert len(np.unique(nL.astype(float))) == nL.size                # K = 100 forms groups no shorter horizon forms
        t1 = mc_draws_device(S, 1, SEED_DRAWS, noise=True, lo=s_lo, plans=plans) + mc_nav_draws_device(S, 1, 14, SEED_DRAWS, lo=s_lo, plans=plans)
        tL = mc_draws_device(S, hc.LONG, SEED_DRAWS, noise=True, lo=s_lo, plans=plans) + mc_nav_draws_device(S, hc.LONG, 14, SEED_DRAWS, lo=s_lo,
                                                                                                         plans=plans)
        for i in (0, 2):
            assert np.array_equal(t1[i], tL[i]) and np.array_equal(t1[i + 1], tL[i + 1][..., :1, :]), (plans, i)
        ld = rr.draws(SEED_DRAWS, rr.STREAM_TRUTH, S, hc.LONG, s_lo, plans)[1]
        tw = tL[1][None] if plans is None else tL[1]
        print("s_lo %d plans %s: K = 1 draws are the leading groups of the K = 100 draws (reference, float64 form, twin); twin vs longdouble "
              "at K = 100 %.2f ulp" % (s_lo, plans, float(rr.ulp_distance(tw, ld).max())))


@pytest.mark.parametrize("K", hc.MC_HORIZONS)
@pytest.mark.parametrize("model", hc.MODELS)
def test_count_comparison_is_taken_by_two_thirds_of_the_plans(model, K, aero_tables):
    po, dyn, par, x, u, s, d, L, S0 = _setup(model, K, aero_tables)
    taken, margins, bounds = count_condition(po, dyn, par, x, u, s, L, S0, hc.mc_nsub(K), hc.MC_S, hc.MC_SEED)
    print("%s K = %d: count equality taken by %d of %d plans (share %.2f); closest commanded norm to a bound %s, rule's threshold %s"
          % (model, K, sum(taken), len(taken), sum(taken) / len(taken), " ".join("%.3e" % v for v in margins),
             " ".join("%.3e" % v for v in bounds)))
    assert 3 * sum(taken) >= 2 * len(taken)
