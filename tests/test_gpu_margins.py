"""Thrust-band back-offs in the conic solve and covariance-driven replanning on the MI355X (scvx_batch_set_thrust_margins,
scvx_cov_path_sigma_f64, scvx_batch_thrust_margins_from_cov, scvx_batch_replan; include/scvx.h) against the independent CPU oracle
under the same back-offs (tests/margin_reference.py; fixture tests/golden/oracle_margin_runs.npz) and against the properties that
define the feature.

Bounds, none of them taken from the device:
  * one subproblem against the independent oracle: those of the unmargined comparison of test_gpu_scvx.py (both sides at 1e-9: 2e-5 on
    the minimiser, 1e-8 relative on the objective);
  * a complete run from the straight-line guess: CONVERGED, the oracle's accept / reject sequence, the band at every node to 1e-6 (the
    bound test_flyable_problem_converges uses for Tmax; the lower side follows from the linearised row by Cauchy-Schwarz), the
    re-propagation defect < 1e-5, final mass, r and v within 1e-4 of the oracle's (the project's contract for a complete run at 1e-8);
  * path sigma: the rule of test_gpu_cov.py -- with e_ref the largest difference between the float64 and the longdouble reference of
    a column, the device must be within max(16 e_ref, K n 2^-52 max|column|) of the longdouble reference;
  * robustify: N_TMIN and N_TMAX >= 2 afterwards (the oracle: 2.90 and 3.02 on plan 0), < 1e-4 before.
Every comparison prints its figures before it asserts.
"""
import os

import numpy as np
import pytest

import cov_reference as cr
import margin_reference as mr
import track_reference as tr
from conftest import GOLDEN
from test_gpu_flight import _flyable

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
_ROB = {}


def _fixture():
    return np.load(os.path.join(GOLDEN, "oracle_margin_runs.npz"))


def _s0(x):
    return np.stack([cr.handover_s0(x[b, 0], 0, 1e-3)[0] for b in range(x.shape[0])])


@pytest.mark.parametrize("variant", ["waves1", "waves2", "waves4", "float tiles", "fins"])
def test_one_subproblem_with_backoffs_against_the_independent_oracle(variant, monkeypatch):
    """scvx_socp_solve at the straight-line guess under the fixture's back-offs against the oracle's solve of the edited SOCP"""
    from successiveconvexification_amd import sample_problems as sp
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache
    g = _fixture()
    lo, hi = g["lo"][:1], g["hi"][:1]
    pp, po = _flyable()
    if variant == "fins":
        pp, ic, pre = sp.base_prob_fin_scaled(), None, "fin_"
    else:
        ic, pre = g["ic"][:1], "sub32_" if variant == "float tiles" else "sub_"
    if variant.startswith("waves"):
        monkeypatch.setenv("SCVX_K4_WAVES", variant[-1])
    ref = {k: (g[pre + k] if variant == "fins" else g[pre + k][0]) for k in ("x", "u", "dsig", "nu", "pobj")}
    c = IntegratorCache(pp, npts=10)
    b = ScvxBatch(c, 1, tol=1e-9)
    if variant == "float tiles":
        b.set_linearization_f32(True)
    b.init(ic)
    xb, ub, sg = b.trajectory()
    free = b.socp_solve()
    b.set_thrust_margins(lo, hi)
    x, u, snew, nu = b.socp_solve()
    st, its, merit, pobj = b.solver_stats()
    ex, eu, es, en = (float(np.abs(x[0] - ref["x"]).max()), float(np.abs(u[0] - ref["u"]).max()), float(abs(snew[0] - sg[0] - ref["dsig"])),
                      float(np.abs(nu[0] - ref["nu"]).max()))
    K = pp.K
    obj = (-x[0, K, 0] + pp.wNu * np.linalg.norm(nu[0]) + 0.5 * np.linalg.norm(np.concatenate([(x - xb)[0].ravel(), (u - ub)[0].ravel()]))
           + abs(snew[0] - sg[0]))
    t = np.linalg.norm(u[0, :, :3], axis=1)
    print("%s: status %d merit %.2e its %d; device-vs-oracle x %.2e u %.2e dsigma %.2e nu %.2e; objective %.10f vs %.10f; |u| in [%.5f, %.5f], "
          "Tmax - hi - |u| >= %.2e; moved by the back-offs: %.2e"
          % (variant, st[0], merit[0], its[0], ex, eu, es, en, obj, ref["pobj"], t.min(), t.max(), (pp.Tmax - hi[0] - t).min(),
             np.abs(u - free[1]).max()))
    assert st[0] == 0 and merit[0] < 1e-9
    assert ex < 2e-5 and eu < 2e-5 and es < 2e-5 and en < 2e-5
    assert abs(obj - ref["pobj"]) < 1e-8 * abs(ref["pobj"])
    assert (t <= pp.Tmax - hi[0] + 1e-8).all()
    assert np.abs(u - free[1]).max() > 1e-4      # the back-offs bind: the unmargined solve of the same subproblem is elsewhere
    b.close(), c.close()


def _state(b, r):
    return tuple(r) + (b.trajectory_record(),) + b.scalars() + b.flags() + b.solver_stats()


@pytest.mark.parametrize("waves", ["1", "2", "4"])
def test_zero_backoffs_and_cleared_backoffs_change_nothing(waves, monkeypatch):
    import bench
    from successiveconvexification_amd import sample_problems as sp
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache
    monkeypatch.setenv("SCVX_K4_WAVES", waves)
    p = sp.base_prob_scaled
    B = 4
    ic = bench.disperse_ics(p, 0, B, 20261018)
    c = IntegratorCache(p, npts=10)
    plain, zero, cleared = (ScvxBatch(c, B).init(ic) for _ in range(3))
    zero.set_thrust_margins(0.0, 0.0)
    cleared.set_thrust_margins(0.1 * (p.Tmax - p.Tmin), 0.2 * (p.Tmax - p.Tmin)).set_thrust_margins(None, None)
    assert not zero.thrust_margins()[0].any() and not cleared.thrust_margins()[1].any() and not plain.thrust_margins()[0].any()
    for step in range(2):
        ref = _state(plain, plain.solve_step())
        for name, b in (("zero", zero), ("cleared", cleared)):
            got = _state(b, b.solve_step())
            for a0, a1 in zip(ref, got):
                assert np.array_equal(a0, a1, equal_nan=True), (name, step)
    # reset keeps the back-offs, init clears them
    lo = np.full((B, p.K + 1), 0.05 * (p.Tmax - p.Tmin))
    zero.set_thrust_margins(lo, 2 * lo)
    zero.reset()
    assert np.array_equal(zero.thrust_margins()[0], lo) and np.array_equal(zero.thrust_margins()[1], 2 * lo)
    zero.init(ic)
    assert not zero.thrust_margins()[0].any() and not zero.thrust_margins()[1].any()
    got = _state(zero, zero.solve_step())
    plain.init(ic)
    for a0, a1 in zip(_state(plain, plain.solve_step()), got):
        assert np.array_equal(a0, a1, equal_nan=True)
    for b in (plain, zero, cleared):
        b.close()
    c.close()


@pytest.mark.parametrize("tiles", ["double", "float"])
def test_backoffs_of_one_trajectory_disturb_no_other(tiles):
    import bench
    from successiveconvexification_amd import sample_problems as sp
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache
    p = sp.base_prob_scaled
    B = 4
    ic = bench.disperse_ics(p, 0, B, 20261018)
    c = IntegratorCache(p, npts=10)
    plain, marg = (ScvxBatch(c, B).set_linearization_f32(tiles == "float").init(ic) for _ in range(2))
    lo = np.zeros((B, p.K + 1))
    lo[1] = 0.3 * (p.Tmax - p.Tmin)
    marg.set_thrust_margins(lo, lo)
    assert np.array_equal(marg.thrust_margins()[0], lo) and np.array_equal(marg.thrust_margins()[1], lo)
    others = [0, 2, 3]
    for step in range(2):
        r0, r1 = _state(plain, plain.solve_step()), _state(marg, marg.solve_step())
        for a0, a1 in zip(r0, r1):
            assert np.array_equal(a0[others], a1[others], equal_nan=True), step
        d = float(np.abs(r0[3][1] - r1[3][1]).max())
        print("%s tiles, step %d: trajectory 1 moved by %.3e, statuses %s / %s" % (tiles, step, d, r0[0], r1[0]))
        assert d > 1e-4
    for b in (plain, marg):
        b.close()
    c.close()


def test_full_run_from_the_straight_line_guess_under_backoffs():
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache, propagate_batch
    g = _fixture()
    pp, po = _flyable()
    ic, lo, hi = g["ic"], g["lo"], g["hi"]
    B, K = ic.shape[0], pp.K
    c = IntegratorCache(pp, npts=10)
    b = ScvxBatch(c, B).init(ic).set_thrust_margins(lo, hi)
    st, it, nu, dj = b.solve()
    x, u, s = b.trajectory()
    # the accept / reject sequence, from a twin stepped one solve_step at a time
    twin = ScvxBatch(c, B).init(ic).set_thrust_margins(lo, hi)
    seq = [[] for _ in range(B)]
    done = np.zeros(B, bool)
    for _ in range(pp.imax - 1):
        s1 = twin.solve_step()[0]
        for t in range(B):
            if not done[t]:
                seq[t].append(0 if s1[t] == 2 else 1)
                done[t] = s1[t] not in (1, 2)
        if done.all():
            break
    want = [[int(v) for v in row if v >= 0] for row in g["guess_accepted"]]
    un = np.linalg.norm(u[..., :3], axis=-1)
    xp = propagate_batch(c, x, u, s, 1.0 / (K + 1))
    defect = float(np.abs(xp - x[:, 1:]).max())
    gx, gu = g["guess_x"], g["guess_u"]
    print("status %s iters %s (oracle %s); sequences %s (oracle %s)" % (st, it, [len(w) for w in want], seq, want))
    print("band: |u| - (Tmin + lo) >= %.3e, (Tmax - hi) - |u| >= %.3e; defect %.3e" % ((un - (pp.Tmin + lo)).min(), ((pp.Tmax - hi) - un).min(), defect))
    print("final mass %s (oracle %s); device-vs-oracle: mass %.2e r %.2e v %.2e | q %.2e w %.2e u %.2e sigma %.2e (the last four: printed only)"
          % (x[:, -1, 0], gx[:, -1, 0], np.abs(x[:, -1, 0] - gx[:, -1, 0]).max(), np.abs(x[:, :, 1:4] - gx[:, :, 1:4]).max(),
             np.abs(x[:, :, 4:7] - gx[:, :, 4:7]).max(), np.abs(x[:, :, 7:11] - gx[:, :, 7:11]).max(), np.abs(x[:, :, 11:] - gx[:, :, 11:]).max(),
             np.abs(u - gu).max(), np.abs(s - g["guess_sigma"]).max()))
    assert np.all(st == 0), (st, it)
    assert seq == want
    assert [int(v) for v in it] == [len(w) for w in want]
    assert (un >= pp.Tmin + lo - 1e-6).all() and (un <= pp.Tmax - hi + 1e-6).all()
    assert defect < 1e-5
    assert np.abs(x[:, -1, 0] - gx[:, -1, 0]).max() < 1e-4
    assert np.abs(x[:, :, 1:4] - gx[:, :, 1:4]).max() < 1e-4 and np.abs(x[:, :, 4:7] - gx[:, :, 4:7]).max() < 1e-4
    # the audit keeps the true band: the headroom shows as negative G_TMIN / G_TMAX at the nodes
    plan = b.flight_check(mode="plan")
    print("G_TMIN %s G_TMAX %s" % (plan.G_TMIN, plan.G_TMAX))
    assert np.all(plan.G_TMAX < 0)
    b.close(), twin.close(), c.close()


def test_path_sigma_against_the_longdouble_reference():
    from successiveconvexification_amd import _lib
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache, cov_path_sigma_batch, cov_propagate_batch, linearize_batch
    g = np.load(os.path.join(GOLDEN, "oracle_flight_runs.npz"))
    pp, po = _flyable()
    x, u, s = g["x"], g["u"], g["sigma"]
    K = po.K
    c = IntegratorCache(pp, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (K + 1))
    S0 = _s0(x)
    noise = np.random.default_rng(5).uniform(0.0, 1e-8, 14)
    for w in ((1.0, 1.0, 100.0), (1.0, 1e-2, 1e4)):
        L, _ = tr.gains(d, K, *w)
        for nz in (None, noise):
            p64 = mr.path_sigma(po, x, u, cr.propagate(d, K, L, S0, nz))
            pld = mr.path_sigma(po, x, u, cr.propagate(d, K, L, S0, nz, np.longdouble), np.longdouble)
            rep, got = cov_path_sigma_batch(c, x, u, d, L, S0, nz)
            assert got.shape == (2, K + 1, _lib.PSIG_N) and np.isfinite(got).all() and not got[:, 0].any()
            for i, name in enumerate(_lib.PSIG_COLUMNS):
                e_ref = float(np.abs(p64[..., i] - pld[..., i]).max())
                bound = max(16.0 * e_ref, K * 17 * EPS * float(np.abs(pld[..., i]).max()))
                e = float(np.abs(got[..., i] - pld[..., i]).max())
                print("weights %s w %s %-6s: device-vs-longdouble %.3e (float64 reference %.3e, bound %.3e), max %.3e"
                      % (w, "0" if nz is None else "> 0", name, e, e_ref, bound, float(np.abs(pld[..., i]).max())))
                assert e <= bound, (w, name, e, bound)
            # the report of the same launch is that of scvx_cov_propagate_f64, bit for bit; S_THRUST is the largest s_T
            plain = cov_propagate_batch(c, x, u, d, L, S0, nz)
            assert np.array_equal(rep.raw, plain.raw, equal_nan=True)
            assert np.array_equal(got[:, :, _lib.PSIG_INDEX["THRUST"]].max(axis=1), plain.S_THRUST)
    # the batch form: its own tiles and gains
    b = ScvxBatch(c, 2).init(g["ic"])
    b.set_trajectory(x, u, s)
    before = (b.trajectory_record(),) + b.scalars() + b.flags() + b.thrust_margins()
    pb = b.path_sigma(S0, noise)
    assert np.array_equal(pb, cov_path_sigma_batch(c, x, u, b.linearization()[1], b.track_gains(), S0, noise)[1])
    for a0, a1 in zip(before, (b.trajectory_record(),) + b.scalars() + b.flags() + b.thrust_margins()):
        assert np.array_equal(a0, a1, equal_nan=True)
    # a NaN in one trajectory's tile poisons its rows only
    dn = d.copy()
    dn.reshape(2, K, -1, 14)[1, 30, 2, 5] = np.nan
    L, _ = tr.gains(d, K)
    good, bad = cov_path_sigma_batch(c, x, u, d, L, S0)[1], cov_path_sigma_batch(c, x, u, dn, L, S0)[1]
    assert np.isnan(bad[1]).all() and np.array_equal(bad[0], good[0])
    b.close(), c.close()


def _robustified():
    """(cache, base batch, robustified batch, S0, psig of the base plans, robustify's return) on the fixture's starts, made once"""
    if not _ROB:
        from successiveconvexification_amd.batch import ScvxBatch
        from successiveconvexification_amd.dynamics import IntegratorCache
        g = _fixture()
        pp, po = _flyable()
        c = IntegratorCache(pp, npts=10)
        base, rob = (ScvxBatch(c, g["ic"].shape[0]).init(g["ic"]) for _ in range(2))
        st0 = base.solve()[0]
        rob.solve()
        assert np.all(st0 == 0), st0
        S0 = _s0(base.trajectory()[0])
        psig = rob.path_sigma(S0)
        _ROB["v"] = (c, base, rob, S0, psig, rob.robustify(S0, nsigma=3, rounds=1))
    return _ROB["v"]


def test_robustify_restores_the_thrust_headroom():
    from successiveconvexification_amd import _lib
    g = _fixture()
    pp, po = _flyable()
    c, base, rob, S0, psig, (st, it, nu, dj, lo, hi) = _robustified()
    band = pp.Tmax - pp.Tmin
    before, after = base.covariance(S0), rob.covariance(S0)
    x0, xr = base.trajectory()[0], rob.trajectory()[0]
    print("replan: status %s in %s steps (oracle %s); final mass %s -> %s (oracle replan %s)"
          % (st, it, [int((r >= 0).sum()) for r in g["replan_accepted"]], x0[:, -1, 0], xr[:, -1, 0], g["replan_x"][:, -1, 0]))
    print("N_TMIN %s -> %s, N_TMAX %s -> %s (oracle replan %s, %s); S_THRUST %s -> %s; back-offs up to %s"
          % (before.N_TMIN, after.N_TMIN, before.N_TMAX, after.N_TMAX, g["replan_rep"][:, cr.IDX["N_TMIN"]], g["replan_rep"][:, cr.IDX["N_TMAX"]],
             before.S_THRUST, after.S_THRUST, lo.max(axis=1)))
    assert np.all(st == 0), (st, it)
    want = np.minimum(3.0 * psig[:, :, _lib.PSIG_INDEX["THRUST"]], 0.25 * band)
    assert np.array_equal(lo, want) and np.array_equal(hi, want)
    assert np.all(before.N_TMIN < 1e-4) and np.all(before.N_TMAX < 1e-4)
    assert np.all(after.N_TMIN >= 2.0) and np.all(after.N_TMAX >= 2.0)
    # the replanned trajectories hold the band they were given, and restarted from create_initial's scalars
    un = np.linalg.norm(rob.trajectory()[1][..., :3], axis=-1)
    assert (un >= pp.Tmin + lo - 1e-6).all() and (un <= pp.Tmax - hi + 1e-6).all()
    assert np.all(it < pp.imax - 1) and np.all(rob.scalars()[2] == it)


def test_commanded_controls_leave_the_band_less_often_after_robustify():
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.montecarlo import gaussian_handover
    pp, po = _flyable()
    c, base, rob, S0, psig, _ = _robustified()
    N, P = 256, S0.shape[0]
    counts = {}
    fleet = ScvxBatch(c, N * P).init(np.repeat(np.load(os.path.join(GOLDEN, "oracle_margin_runs.npz"))["ic"], N, axis=0))
    for name, b in (("base", base), ("robustified", rob)):
        x, u, s = b.trajectory()
        dx0 = np.concatenate([gaussian_handover(S0[i], 0, N, 20261018) for i in range(P)])
        fleet.set_trajectory(cr.rep(x, N), cr.rep(u, N), cr.rep(s, N))
        r = fleet.track(dx0, dense=True)
        t = np.linalg.norm(r.ufly[:, :, :3], axis=-1).reshape(P, N, -1)
        counts[name] = ((t < pp.Tmin) | (t > pp.Tmax)).sum(axis=(1, 2))
    print("commanded node controls outside [Tmin, Tmax], %d starts per plan x %d nodes: base %s, robustified %s"
          % (N, pp.K + 1, counts["base"], counts["robustified"]))
    assert np.all(counts["robustified"] < counts["base"]), counts
    fleet.close()


def test_arguments_are_refused():
    import ctypes as C
    from successiveconvexification_amd import _lib, sample_problems as sp
    from successiveconvexification_amd.batch import ScvxBatch, _p
    from successiveconvexification_amd.dynamics import IntegratorCache
    p = sp.base_prob_scaled
    c = IntegratorCache(p, npts=10)
    b = ScvxBatch(c, 2)
    K, band = p.K, p.Tmax - p.Tmin
    with pytest.raises(_lib.ScvxError, match="scvx_batch_init first"):
        b.set_thrust_margins(0.0, 0.0)
    b.init(None)
    L, h = c._L, b.handle
    err = lambda: L.scvx_last_error(c.handle).decode()   # noqa: E731
    z = np.zeros((2, K + 1))

    def one(v):
        a = z.copy()
        a[1, 7] = v
        return a

    assert L.scvx_batch_set_thrust_margins(h, _p(z), None) == -1 and "both" in err()
    assert L.scvx_batch_set_thrust_margins(h, None, _p(z)) == -1 and "both" in err()
    for v in (-1e-9, np.nan, np.inf):
        assert L.scvx_batch_set_thrust_margins(h, _p(one(v)), _p(z)) == -1 and "finite" in err(), v
        assert L.scvx_batch_set_thrust_margins(h, _p(z), _p(one(v))) == -1 and "finite" in err(), v
    assert L.scvx_batch_set_thrust_margins(h, _p(one(0.5 * band)), _p(one(0.5 * band))) == -1 and "Tmax - Tmin" in err()
    assert not b.thrust_margins()[0].any()                       # nothing was set
    assert L.scvx_batch_set_thrust_margins(h, _p(one(0.4 * band)), _p(one(0.4 * band))) == 0
    assert b.thrust_margins()[0][1, 7] == 0.4 * band and L.scvx_batch_get_thrust_margins(h, None, None) == 0
    q, r, qf = np.ones(14), np.ones(3), np.full(14, 100.0)
    S0 = np.ascontiguousarray(np.broadcast_to(1e-6 * np.eye(14), (2, 14, 14)))
    call = lambda S, w, ns, cap: L.scvx_batch_thrust_margins_from_cov(h, _p(q), _p(r), _p(qf), S, w, C.c_double(ns), C.c_double(cap), None)   # noqa: E731
    assert call(None, None, 3.0, 0.25) == -1 and "null" in err()
    for ns in (-1.0, np.nan, np.inf):
        assert call(_p(S0), None, ns, 0.25) == -1 and "nsigma" in err(), ns
    for cap in (0.0, 0.5, -0.1, np.nan):
        assert call(_p(S0), None, 3.0, cap) == -1 and "cap" in err(), cap
    bad_w = np.zeros(14)
    bad_w[3] = -1.0
    assert call(_p(S0), _p(bad_w), 3.0, 0.25) == -1 and "w must be" in err()
    assert L.scvx_batch_thrust_margins_from_cov(h, _p(q), _p(np.zeros(3)), _p(qf), _p(S0), None, C.c_double(3.0), C.c_double(0.25), None) == -1
    assert b.thrust_margins()[0][1, 7] == 0.4 * band and b.thrust_margins()[0].sum() == 0.4 * band   # the refused calls left them alone
    with pytest.raises(ValueError):
        b.set_thrust_margins(z, None)
    with pytest.raises(ValueError):
        b.robustify(S0, rounds=0)
    # replan: a failed trajectory stays frozen, the others restart from create_initial's scalars with their iterate
    b.set_thrust_margins(None, None)
    b.solve_step()
    st, ac, lv = b.flags()
    b.set_flags(status=np.array([3, 1]), active=np.array([0, 1]), live=np.array([0, 1]))
    rec, (rk0, cost0, it0) = b.trajectory_record(), b.scalars()
    b.replan()
    rk, cost, it = b.scalars()
    st, ac, lv = b.flags()
    assert np.array_equal(b.trajectory_record(), rec)
    assert rk[1] == 100.0 and np.isinf(cost[1]) and it[1] == 0 and (st[1], ac[1], lv[1]) == (1, 1, 1)
    assert rk[0] == rk0[0] and cost[0] == cost0[0] and it[0] == it0[0] and (st[0], ac[0], lv[0]) == (3, 0, 0)
    s1, nu1, dj1 = b.solve_step()
    assert s1[0] == 3 and s1[1] == 1 and np.isinf(dj1[1]) and b.scalars()[0][1] == 100.0 * p.bet   # the rho = NaN branch
    b.close(), c.close()
