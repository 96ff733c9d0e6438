"""The flight check (scvx_flight_check_f64 / scvx_batch_flight_check) on the MI355X against the independent CPU reference
(tests/flight_reference.py: the C oracle -- or, for the aerodynamic torque, tests/aero_torque_reference.py -- driven substep by substep).

Bounds, none of them taken from the device:
  * PLAN states: 1e-12, the bound the suite holds between K2 and the oracle (test_gpu_discretize.py:50); xfly vs scvx_propagate_f64 of
    the same arrays: 1e-13, the bound between K1's endpoint and K2, the same map in two kernels (:52).  (Measured: bit for bit on the
    B = 5 cases without fins, 7e-18 with them, 1.7e-18 over the 8,192 headline rows -- the compiler contracts the same source
    differently in the two kernels -- so bitwise equality is printed, not asserted.)
  * SHOOT states: K * 1e-12 * A -- one K2-sized difference per segment, carried to the end with the sensitivity A the REFERENCE chain
    shows (flight_reference.sensitivity, eps = 1e-9 unless stated).
  * G_* columns: the state bound times flight_reference.g_lipschitz (2-norms of a few components times tan gammaGs, 1 / cos deltaMax).
Every comparison prints its figures before it asserts.
"""
import os
from dataclasses import replace

import numpy as np
import pytest

import flight_reference as fr
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

MODELS = ["exo", "aero", "aero+dpmax", "aero+fins", "aero+torque", "aero+fins+torque"]
_STATE_VALUE_COLS = ("GAP", "MISS_R", "MISS_V", "MISS_Q", "MISS_W", "MASS_END", "QNORM")


def _problems(model, aero_tables):
    """(product problem, oracle problem, dyn module of the reference, its Params)"""
    import aero_torque_reference as atr
    from oracle import dynamics as od, model as om
    from successiveconvexification_amd import sample_problems as sp
    from successiveconvexification_amd.defns import AtmosphericData
    a, oa = AtmosphericData(*aero_tables), om.AeroData(*aero_tables)
    torque = "torque" in model
    if model == "exo":
        pp, po = sp.base_prob_scaled, om.base_prob_scaled()
    elif "fins" in model:
        pp, po = sp.base_prob_fin_scaled(a, torque=torque), om.base_prob_fin_scaled(oa)
    else:
        pp, po = sp.base_prob_aero_scaled(a, torque=torque), om.base_prob_scaled(oa)
    if "dpmax" in model:
        vm = 1.02 * float(np.linalg.norm(po.vIi)) * 1.1 * np.sqrt(3)   # above every dispersed initial speed
        dpmax = 0.5 * po.rho * vm**2
        pp, po = replace(pp, dpMax=dpmax, model_flags=pp.model_flags | 1), replace(po, enforce_dp=True, dpMax=dpmax)
    if torque:
        return pp, po, atr, atr.Params(po, torque=True)
    return pp, po, od, od.Params(po)


def _compare(tag, dev, ref, bound, po):
    """device report vs reference report [B][16]: state-valued columns within `bound`, G_* within bound * Lipschitz factor"""
    L = fr.g_lipschitz(po)
    worst_s = worst_g = 0.0
    for n in fr.COLUMNS:
        d, r = dev[:, fr.IDX[n]], ref[:, fr.IDX[n]]
        inf = np.isneginf(r)
        assert np.array_equal(inf, np.isneginf(d)), (tag, n, d, r)
        e = float(np.abs(d[~inf] - r[~inf]).max()) if (~inf).any() else 0.0
        if n in _STATE_VALUE_COLS:
            worst_s = max(worst_s, e)
        else:
            worst_g = max(worst_g, e)
    print("%s: state columns %.3e (bound %.3e), G columns %.3e (bound %.3e)" % (tag, worst_s, bound, worst_g, bound * L))
    assert worst_s <= bound, (tag, worst_s, bound)
    assert worst_g <= bound * L, (tag, worst_g, bound * L)
    return worst_s, worst_g


_CASES = {}


def _case(model, aero_tables):
    """dispersed B = 5 batch after 3 solve_steps (unconverged, large defects): (pp, po, dyn, par, x, u, sigma)"""
    if model not in _CASES:
        from oracle import model as om
        from successiveconvexification_amd.batch import ScvxBatch
        from successiveconvexification_amd.dynamics import IntegratorCache
        pp, po, dyn, par = _problems(model, aero_tables)
        c = IntegratorCache(pp, npts=10)
        b = ScvxBatch(c, 5).init(om.disperse_ics(po, 5, 20261016))
        for _ in range(3):
            st, _, _ = b.solve_step()
            assert np.isin(st, (0, 1, 2)).all(), st
        _CASES[model] = (pp, po, dyn, par) + b.trajectory()
        b.close()
        c.close()
    return _CASES[model]


@pytest.mark.parametrize("nsub", [1, 4, 10])
@pytest.mark.parametrize("model", MODELS)
def test_plan_parity(model, nsub, aero_tables):
    from successiveconvexification_amd.dynamics import IntegratorCache, flight_check_batch, propagate_batch
    pp, po, dyn, par, x, u, s = _case(model, aero_tables)
    c = IntegratorCache(pp, npts=nsub)
    rep = flight_check_batch(c, x, u, s, mode="plan", dense=True)       # nsub = the context's
    xn = propagate_batch(c, x, u, s, 1.0 / (po.K + 1))
    k2 = float(np.abs(rep.xfly[:, 1:] - xn).max())
    print("%s nsub %d PLAN: xfly vs scvx_propagate_f64 %.3e, bitwise %s" % (model, nsub, k2, np.array_equal(rep.xfly[:, 1:], xn)))
    assert k2 <= 1e-13
    assert np.array_equal(rep.xfly[:, 0], x[:, 0])
    ref, xref = fr.fly(dyn, po, x, u, s, nsub, fr.PLAN, par)
    assert float(np.abs(rep.xfly - xref).max()) <= 1e-12
    assert ref[:, 0].max() > 1e-4      # unconverged plans: defects far above any tolerance here, nothing cancels
    _compare("%s nsub %d PLAN" % (model, nsub), rep.raw, ref, 1e-12, po)
    # the report without the dense output is the same report
    assert np.array_equal(flight_check_batch(c, x, u, s, mode="plan").raw, rep.raw, equal_nan=True)
    c.close()


@pytest.mark.parametrize("nsub", [1, 4, 10])
@pytest.mark.parametrize("model", MODELS)
def test_shoot_parity(model, nsub, aero_tables):
    from successiveconvexification_amd.dynamics import IntegratorCache, flight_check_batch
    pp, po, dyn, par, x, u, s = _case(model, aero_tables)
    c = IntegratorCache(pp, npts=10)
    rep = flight_check_batch(c, x, u, s, nsub=nsub, mode="shoot", dense=True)   # nsub is the call's, not the context's
    ref, xref = fr.fly(dyn, po, x, u, s, nsub, fr.SHOOT, par)
    A = fr.sensitivity(dyn, po, x, u, s, nsub, 1e-9, par=par)
    bound = po.K * 1e-12 * A
    dx = float(np.abs(rep.xfly - xref).max())
    print("%s nsub %d SHOOT: A %.3f, bound %.3e, device's largest state difference %.3e" % (model, nsub, A, bound, dx))
    assert dx <= bound
    _compare("%s nsub %d SHOOT" % (model, nsub), rep.raw, ref, bound, po)
    c.close()


def _flyable():
    from oracle import model as om
    from successiveconvexification_amd import sample_problems as sp
    kw = dict(mdry=0.55, nuTol=1e-6, delTol=1e-3, imax=40, tf_guess=8.0)
    return replace(sp.base_prob_scaled, **kw), replace(om.base_prob_scaled(), **kw)


def test_oracle_converged_plans_through_the_device():
    from oracle import dynamics as od
    from successiveconvexification_amd.dynamics import IntegratorCache, flight_check_batch
    g = np.load(os.path.join(GOLDEN, "oracle_flight_runs.npz"))
    pp, po = _flyable()
    x, u, s = g["x"], g["u"], g["sigma"]
    c = IntegratorCache(pp, npts=10)
    plan = flight_check_batch(c, x, u, s, mode="plan")
    _compare("oracle plans PLAN", plan.raw, g["report_plan"], 1e-12, po)
    A = fr.sensitivity(od, po, x, u, s, 10, 1e-9)
    shoot = flight_check_batch(c, x, u, s, mode="shoot")
    print("oracle plans SHOOT: A %.3f, GAP %s (stored %s)" % (A, shoot.GAP, g["report_shoot"][:, 0]))
    _compare("oracle plans SHOOT", shoot.raw, g["report_shoot"], po.K * 1e-12 * A, po)
    # the violation only this feature shows: on the bound at the nodes, below it in between
    print("G_TMIN", shoot.G_TMIN, plan.G_TMIN, "at nodes", (po.Tmin - np.linalg.norm(u, axis=-1)).max())
    assert np.all(shoot.G_TMIN > 1e-4) and np.all(plan.G_TMIN > 1e-4)
    assert (po.Tmin - np.linalg.norm(u, axis=-1)).max() <= 1e-8
    assert not shoot.ok(1e-5).any() and shoot.ok(1e-3).all()
    # a plan made with 10 substeps flown with 40
    s40 = flight_check_batch(c, x, u, s, nsub=40, mode="shoot")
    A40 = fr.sensitivity(od, po, x, u, s, 40, 1e-9)
    _compare("oracle plans SHOOT nsub 40", s40.raw, g["report_shoot_nsub40"], po.K * 1e-12 * A40, po)
    print("SHOOT GAP nsub 10 -> 40:", shoot.GAP, s40.GAP)
    assert np.abs(s40.GAP - shoot.GAP).max() < 1e-7
    c.close()


def test_device_converged_plans_and_the_batch_is_untouched():
    import bench
    from oracle import dynamics as od
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache
    pp, po = _flyable()
    B = 8
    ic = bench.disperse_ics(pp, 0, B, 7)
    c = IntegratorCache(pp, npts=10)
    b = ScvxBatch(c, B).init(ic)
    twin = ScvxBatch(c, B).init(ic)
    st, it, nu, dj = b.solve()
    twin.solve()
    assert np.all(st == 0), (st, it)
    before = (b.trajectory_record(),) + b.scalars() + b.flags() + b.linearization()
    shoot = b.flight_check(mode="shoot", dense=True)
    plan = b.flight_check(nsub=10, mode="plan", dense=True)
    after = (b.trajectory_record(),) + b.scalars() + b.flags() + b.linearization()
    for a0, a1 in zip(before, after):
        assert np.array_equal(a0, a1, equal_nan=True)
    x, u, s = b.trajectory()
    par = od.Params(po)
    rp, _ = fr.fly(od, po, x, u, s, 10, fr.PLAN, par)
    _compare("device plans PLAN", plan.raw, rp, 1e-12, po)
    rs, xs = fr.fly(od, po, x, u, s, 10, fr.SHOOT, par)
    A9 = fr.sensitivity(od, po, x, u, s, 10, 1e-9, par=par)
    _compare("device plans SHOOT", shoot.raw, rs, po.K * 1e-12 * A9, po)
    assert float(np.abs(shoot.xfly - xs).max()) <= po.K * 1e-12 * A9
    assert plan.GAP.max() < 1e-5                     # the defect bound of test_flyable_problem_converges
    # every segment's defect is a perturbation injected on the way; the 2 covers second order
    A6 = fr.sensitivity(od, po, x, u, s, 10, 1e-6, par=par)
    defects = np.abs(plan.xfly[:, 1:] - x[:, 1:]).max(axis=2).sum(axis=1)
    print("device plans: A(1e-6) %.3f, sum of defects %s, SHOOT GAP %s" % (A6, defects, shoot.GAP))
    assert np.all(shoot.GAP <= 2.0 * A6 * defects)
    # convex in a first-order hold / monotone: cannot fail between nodes when they hold at them
    print("G_TMAX %s G_MASS %s G_TMIN %s" % (shoot.G_TMAX.max(), shoot.G_MASS.max(), shoot.G_TMIN))
    assert shoot.G_TMAX.max() <= 1e-6 and shoot.G_MASS.max() <= 1e-6
    # a following solve_step equals, bit for bit, that of a twin batch never checked
    r1, r2 = b.solve_step(), twin.solve_step()
    for a0, a1 in zip(r1 + (b.trajectory_record(),) + b.scalars(), r2 + (twin.trajectory_record(),) + twin.scalars()):
        assert np.array_equal(a0, a1, equal_nan=True)
    b.close(), twin.close(), c.close()


def test_at_size_headline_batch():
    import bench
    from oracle import dynamics as od, model as om
    from successiveconvexification_amd import montecarlo as mc, sample_problems as sp
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache, flight_check_batch, propagate_batch
    pp, po = sp.base_prob_scaled, om.base_prob_scaled()
    B, K = 8192, pp.K
    c = IntegratorCache(pp, npts=10)
    b = ScvxBatch(c, B).init(bench.disperse_ics(pp, 0, B, 20261004))
    for _ in range(14):
        b.solve_step_async()
    status, _, _ = b.flags()
    x, u, s = b.trajectory()
    plan = b.flight_check(mode="plan", dense=True)
    xn = propagate_batch(c, x, u, s, 1.0 / (K + 1))
    d = float(np.abs(plan.xfly[:, 1:] - xn).max())
    print("B = 8192 PLAN xfly vs propagate_batch: %.3e over all rows, bitwise %s" % (d, np.array_equal(plan.xfly[:, 1:], xn)))
    assert d <= 1e-13
    shoot = b.flight_check(mode="shoot")
    assert np.isfinite(plan.raw[:, [i for i in range(16) if i not in (13, 14)]]).all()
    assert np.isfinite(shoot.raw[:, [i for i in range(16) if i not in (13, 14)]]).all()
    assert np.all(np.isneginf(shoot.raw[:, 13:15]))
    # the host-array form gives the batch form's rows
    assert np.array_equal(flight_check_batch(c, x, u, s, mode="shoot").raw, shoot.raw)
    rows = np.random.default_rng(20261016).choice(B, 16, replace=False)
    par = od.Params(po)
    ref, _ = fr.fly(od, po, x[rows], u[rows], s[rows], 10, fr.SHOOT, par)
    A = fr.sensitivity(od, po, x[rows], u[rows], s[rows], 10, 1e-9, par=par)
    print("B = 8192 SHOOT rows %s: A %.3f, bound %.3e" % (rows.tolist(), A, K * 1e-12 * A))
    _compare("B = 8192 SHOOT", shoot.raw[rows], ref, K * 1e-12 * A, po)
    summ = mc.flight_summary(shoot, status, 0.0)
    assert sum(summ["counts"].values()) == B == summ["n"]
    b.close(), c.close()


def test_nan_row_is_contained_and_arguments_are_checked():
    import ctypes as C
    from oracle import model as om
    from successiveconvexification_amd import _lib, sample_problems as sp
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache, flight_check_batch, _p
    pp, po = sp.base_prob_scaled, om.base_prob_scaled()
    c = IntegratorCache(pp, npts=10)
    b = ScvxBatch(c, 5).init(om.disperse_ics(po, 5, 20261004))
    b.solve_step()
    x, u, s = b.trajectory()
    for mode in ("shoot", "plan"):
        clean = flight_check_batch(c, x, u, s, mode=mode, dense=True)
        xb = x.copy()
        xb[2, 7, 4] = np.nan
        bad = flight_check_batch(c, xb, u, s, mode=mode, dense=True)
        keep = [0, 1, 3, 4]
        assert np.array_equal(bad.raw[keep], clean.raw[keep]) and np.array_equal(bad.xfly[keep], clean.xfly[keep])
        for n in ("GAP", "MISS_R", "MISS_V", "MISS_Q", "MISS_W", "G_MASS", "G_GLIDE", "G_TILT", "G_RATE", "QNORM"):
            assert np.isnan(getattr(bad, n)[2]), (mode, n)
        for n in ("G_TMAX", "G_TMIN", "G_GIMBAL"):
            assert getattr(bad, n)[2] == getattr(clean, n)[2], (mode, n)
        assert not bad.ok(1e9)[2]
    # arguments: SCVX_ERR_ARG and a message each
    L, h, K = c._L, c.handle, pp.K
    rep = np.zeros((5, 16))
    args = lambda **kw: [kw.get("B", 5), kw.get("K", K), kw.get("x", _p(x)), kw.get("u", _p(u)), kw.get("s", _p(s)),  # noqa: E731
                         kw.get("nsub", 10), kw.get("mode", 0), kw.get("rep", _p(rep)), None]
    cases = [(dict(nsub=0), "nsub"), (dict(nsub=-3), "nsub"), (dict(mode=2), "mode"), (dict(mode=-1), "mode"), (dict(B=0), "B >= 1"),
             (dict(K=K - 1), "K must equal"), (dict(x=None), "null"), (dict(u=None), "null"), (dict(s=None), "null"), (dict(rep=None), "null")]
    for kw, word in cases:
        for fn in (L.scvx_flight_check_f64_host, L.scvx_flight_check_f64):
            a = args(**kw)
            if fn is L.scvx_flight_check_f64:   # device form: the checks come before any pointer is used
                a = a[:2] + [C.c_void_p(1) if v is not None else None for v in a[2:5]] + a[5:7] + [C.c_void_p(1) if a[7] is not None else None, None]
            assert fn(h, *a) == -1, (kw, fn)
            assert word in L.scvx_last_error(h).decode(), (kw, L.scvx_last_error(h))
    assert L.scvx_batch_flight_check(b.handle, -1, 0, _p(rep), None) == -1 and "nsub" in L.scvx_last_error(h).decode()
    assert L.scvx_batch_flight_check(b.handle, 0, 7, _p(rep), None) == -1 and "mode" in L.scvx_last_error(h).decode()
    assert L.scvx_batch_flight_check(b.handle, 0, 0, None, None) == -1 and "null" in L.scvx_last_error(h).decode()
    with pytest.raises(_lib.ScvxError, match="mode"):
        b.flight_check(mode=7)
    with pytest.raises(ValueError, match="mode"):
        b.flight_check(mode="glide")
    with pytest.raises(ValueError):
        flight_check_batch(c, x[:, :, :13], u, s)
    # the context and the batch still work
    assert np.array_equal(b.flight_check(mode="shoot").raw, flight_check_batch(c, x, u, s, mode="shoot").raw)
    b.close(), c.close()


def test_rocketland_fly_single_problem():
    from successiveconvexification_amd import rocketland as rl, sample_problems as sp
    from successiveconvexification_amd.dynamics import IntegratorCache, flight_check_batch
    p = sp.base_prob_scaled
    c = IntegratorCache(p, npts=10)
    ip = rl.create_initial(p, c)
    ip, _, _ = rl.solve_step(ip, c)
    r = rl.fly(ip, c, mode="plan", dense=True)
    x, u, s = ip.model.trajectory()
    assert len(r) == 1 and np.array_equal(r.raw, flight_check_batch(c, x, u, s, mode="plan").raw)
    assert np.array_equal(r.raw, ip.model.flight_check(mode="plan").raw) and r.xfly.shape == (1, p.K + 1, 14)
