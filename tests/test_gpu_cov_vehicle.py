"""Vehicle errors in the covariance and navigation analyses on the MI355X (scvx_vehicle_tiles_f64, scvx_cov_vehicle_f64,
scvx_nav_cov_vehicle_f64, the scvx_batch_*_veh forms; include/scvx.h) against the independent CPU reference
(tests/cov_vehicle_reference.py) and against the device's own sampled flights.

Bounds, none of them taken from the device:
  * vehicle tiles: the reference's own truncation estimate |value(h / 2) - extrapolate| plus the rounding term K 1e-12 / h.
  * sens: 8 x the float64 numpy recursion's distance from the longdouble one plus 4 ulp of the largest |J|.
  * decomposition: the kernel forms t = sum_j (J_aj J_cj) p_j by six fused multiply-adds (one rounding of each product, one of each
    partial sum: 7 eps sum_j |J_aj J_cj p_j|) and adds it to Sigma (one more rounding of the sum); the yardstick is formed in
    longdouble: eps (8 sum_j |J_aj J_cj p_j| + |Sigma^tot|).
  * report, cov, sig, covK: test_gpu_cov.py's _check_parity on Sigma^tot; psig: test_gpu_nav_margins.py's _check_psig.
  * landing rows: the central difference's own truncation estimate (h and h / 2) plus K 1e-12 A_cl / h.
  * statistics: six standard errors (mc_reference.se_check; s / sqrt(2 (N - 1)) for a standard deviation).
Every comparison prints its figures before it asserts.
"""
import os

import numpy as np
import pytest

import cov_reference as cr
import cov_vehicle_reference as cv
import mc_reference as mr
import mc_vehicle_reference as vr
import track_reference as tr
from conftest import GOLDEN
from test_gpu_cov import _check_parity
from test_gpu_flight import _flyable
from test_gpu_nav_margins import _check_psig

pytestmark = pytest.mark.gpu

CASES = ["exo", "aero+fins", "aero+fins+torque", "golden"]
EPS = 2.0 ** -52
SP = {3: np.array([1e-3, 1e-3, 2e-3, 1e-3, 0.0, 0.0]), 5: np.array([1e-3, 2e-3, 1e-3, 3e-3, 5e-2, 1e-2])}
_C = {}


def _case(name, aero_tables):
    """(pp, po, dyn, par, x, u, s, K): B = 3 at K = 3 for a model name (tests/horizon_cases.py), the two golden plans at K = 50"""
    if name not in _C:
        if name == "golden":
            from oracle import dynamics as od
            g = np.load(os.path.join(GOLDEN, "oracle_flight_runs.npz"))
            pp, po = _flyable()
            _C[name] = (pp, po, od, od.Params(po), g["x"], g["u"], g["sigma"], po.K)
        else:
            import horizon_cases as hc
            _C[name] = hc.case(name, 3, aero_tables) + (3,)
    return _C[name]


def _s0(x):
    return np.stack([cr.handover_s0(x[b, 0])[0] for b in range(x.shape[0])])


def _sp(name, nu):
    sp = SP[nu].copy()
    if name == "golden" or name == "exo":
        sp[4:] = 0.0
    return sp


@pytest.mark.parametrize("name", CASES)
def test_vehicle_tiles_against_the_finite_difference_reference(name, aero_tables):
    from successiveconvexification_amd.dynamics import IntegratorCache, vehicle_tiles_batch
    pp, po, dyn, par, x, u, s, K = _case(name, aero_tables)
    c = IntegratorCache(pp, npts=10)
    vt = vehicle_tiles_batch(c, x, u, s)
    ref, trunc = cv.vtile_fd(dyn, po, par, x, u, s)
    for col, tag in ((0, "ISP"), (1, "AERO")):
        err = np.abs(vt[:, :, col] - ref[:, :, col])
        bound = trunc[:, :, col] + cv.rounding(K, cv.H_FD)
        print("%s %s tile: values to %.3e, device against central differences %.3e, bound %.3e .. %.3e"
              % (name, tag, np.abs(ref[:, :, col]).max(), err.max(), bound.min(), bound.max()))
        assert np.all(err <= bound), (name, tag, err.max())
    assert vt.shape == (x.shape[0], K, 2, 14) and np.abs(vt[:, :, 0]).max() > 0.0
    if "aero" in name:
        assert np.abs(vt[:, :, 1]).max() > 0.0
    else:
        assert not vt[:, :, 1].any()                                  # exactly zero without aerodynamics
    assert np.array_equal(vehicle_tiles_batch(c, x, u, s), vt)         # two launches agree bit for bit
    assert np.array_equal(vehicle_tiles_batch(c, x[:1], u[:1], s[:1]), vt[:1])   # B = 1: the last block's idle lanes write nothing
    c.close()


@pytest.mark.parametrize("mfma", ["0", "1"])
@pytest.mark.parametrize("name", CASES)
def test_zero_errors_are_the_calls_extended_bit_for_bit(name, mfma, aero_tables, monkeypatch):
    from successiveconvexification_amd.dynamics import (IntegratorCache, cov_path_sigma_batch, cov_propagate_batch, linearize_batch,
                                                          nav_cov_batch, nav_path_sigma_batch, vehicle_tiles_batch)
    import nav_margin_reference as nm
    monkeypatch.setenv("SCVX_COV_MFMA", mfma)
    pp, po, dyn, par, x, u, s, K = _case(name, aero_tables)
    c = IntegratorCache(pp, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (K + 1))
    L, _ = tr.gains(d, K)
    S0 = _s0(x)
    vt = vehicle_tiles_batch(c, x, u, s)
    veh = dict(vehicle=(np.zeros(6), np.zeros(6)), vtile=vt)
    same = lambda a, b: np.array_equal(a, b, equal_nan=True)   # noqa: E731
    w = np.full(14, 1e-9)
    plain, new = cov_propagate_batch(c, x, u, d, L, S0, w, dense=True), cov_propagate_batch(c, x, u, d, L, S0, w, dense=True, **veh)
    assert same(plain.raw, new.raw) and same(plain.sig, new.sig) and same(plain.covK, new.covK) and same(plain.cov, new.cov)
    (r0, p0), (r1, p1) = cov_path_sigma_batch(c, x, u, d, L, S0, w), cov_path_sigma_batch(c, x, u, d, L, S0, w, **veh)
    assert same(r0.raw, r1.raw) and same(p0, p1)
    H, rm = nm.position_model(x[0, 0])
    plain, new = nav_cov_batch(c, x, u, d, L, S0, S0, H, rm, w, dense=True), nav_cov_batch(c, x, u, d, L, S0, S0, H, rm, w, dense=True, **veh)
    for n_ in ("raw", "navraw", "sig", "navsig", "kf", "joint"):
        assert same(getattr(plain, n_), getattr(new, n_)), n_
    (r0, p0), (r1, p1) = nav_path_sigma_batch(c, x, u, d, L, S0, S0, H, rm, w), nav_path_sigma_batch(c, x, u, d, L, S0, S0, H, rm, w, **veh)
    assert same(r0.raw, r1.raw) and same(r0.navraw, r1.navraw) and same(p0, p1)
    c.close()


def _cov_reference(po, x, u, d, K, L, S0, sp, vt):
    """float64 and longdouble runs of the reference, and the tuple test_gpu_cov._check_parity takes"""
    r64 = cv.cov_run(po, x, u, d, K, L, S0, sp, vt)
    rld = cv.cov_run(po, x, u, d, K, L, S0, sp, vt, dtype=np.longdouble)
    rep_ld, det = cr.report(po, x, u, rld["cov"], np.longdouble, detail=True)
    return r64, rld, (L, r64["report"], r64["cov"], r64["sig"], rep_ld, rld["cov"], rld["sig"], det)


@pytest.mark.parametrize("mfma", ["0", "1"])
@pytest.mark.parametrize("name", CASES)
def test_covariance_form_against_the_longdouble_reference(name, mfma, aero_tables, monkeypatch):
    """sens, the decomposition, the report, the dense outputs and psig of Sigma^tot; B = 3 (2 on the golden plans) and B = 1"""
    from successiveconvexification_amd.dynamics import (IntegratorCache, cov_path_sigma_batch, cov_propagate_batch, linearize_batch,
                                                          vehicle_tiles_batch)
    monkeypatch.setenv("SCVX_COV_MFMA", mfma)
    pp, po, dyn, par, x, u, s, K = _case(name, aero_tables)
    c = IntegratorCache(pp, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (K + 1))
    L, _ = tr.gains(d, K)
    S0 = _s0(x)
    sp = _sp(name, c.nu)
    n = 14 + c.nu
    vt = vehicle_tiles_batch(c, x, u, s)
    veh = dict(vehicle=(np.zeros(6), sp), vtile=vt)
    r64, rld, ref = _cov_reference(po, x, u, d, K, L, S0, sp, vt)
    dev = cov_propagate_batch(c, x, u, d, L, S0, dense=("sig", "covK", "cov", "sens"), **veh)
    plain = cov_propagate_batch(c, x, u, d, L, S0, dense=("cov",))
    tag = "%s SCVX_COV_MFMA=%s" % (name, mfma)
    # sens
    e_ref, jmax = float(np.abs(r64["J"] - rld["J"]).max()), float(np.abs(rld["J"]).max())
    e, bound = float(np.abs(dev.sens - rld["J"]).max()), 8.0 * e_ref + 4.0 * EPS * jmax
    print("%s sens: device-vs-longdouble %.3e (float64 reference %.3e, bound %.3e), max %.3e" % (tag, e, e_ref, bound, jmax))
    assert dev.sens.shape == (x.shape[0], K + 1, n, 6) and not dev.sens[:, 0].any()
    if c.nu == 3:
        assert not dev.sens[..., 5].any()                             # no fins: the FIN column is zero
    if "aero" not in name:
        assert not dev.sens[..., 4].any()
    assert e <= bound, (tag, e, bound)
    # decomposition, on the device's own numbers
    Jl, pl = dev.sens.astype(np.longdouble), (sp * sp).astype(np.longdouble)
    terms = np.einsum("bkic,bkjc,c->bkij", np.abs(Jl), np.abs(Jl), pl)
    want = plain.cov.astype(np.longdouble) + np.einsum("bkic,bkjc,c->bkij", Jl, Jl, pl)
    err = np.abs(dev.cov - want).astype(np.float64)
    bnd = (EPS * (8.0 * terms + np.abs(want))).astype(np.float64)
    print("%s decomposition: cov - (plain cov + sens diag(sp^2) sens') %.3e, bound up to %.3e, worst ratio %.3f"
          % (tag, err.max(), bnd.max(), float((err / np.where(bnd > 0, bnd, 1.0)).max())))
    assert np.all(err <= bnd)
    # the report and the dense outputs of Sigma^tot, psig
    _check_parity(tag, K, dev, ref)
    rep, psig = cov_path_sigma_batch(c, x, u, d, L, S0, **veh)
    assert np.array_equal(rep.raw, dev.raw)
    _check_psig(tag, po, K, n, psig, r64["psig"], rld["psig"])
    assert np.all(dev.SIG_R > cov_propagate_batch(c, x, u, d, L, S0).SIG_R)
    # B = 1: the first plan alone is the first row
    one = cov_propagate_batch(c, x[:1], u[:1], d[:1], L[:1], S0[:1], dense=("cov", "sens"), vehicle=(np.zeros(6), sp), vtile=vt[:1])
    assert np.array_equal(one.cov, dev.cov[:1]) and np.array_equal(one.sens, dev.sens[:1]) and np.array_equal(one.raw, dev.raw[:1])
    c.close()


@pytest.mark.parametrize("name", CASES)
def test_navigation_form(name, aero_tables):
    """N0 = 0, m = 0: the covariance form to rounding (both against the covariance reference).  m = 3, 6: the eps blocks of joint, navsig,
    kf and NAV_* are the plain call's bit for bit; the truth block, the report, psig and EST_R / EST_V against the reference"""
    import nav_margin_reference as nm
    import nav_reference as nr
    from successiveconvexification_amd.dynamics import IntegratorCache, linearize_batch, nav_cov_batch, nav_path_sigma_batch, vehicle_tiles_batch
    from successiveconvexification_amd.montecarlo import measurement_rows
    from test_nav_cpu import pv_model
    pp, po, dyn, par, x, u, s, K = _case(name, aero_tables)
    c = IntegratorCache(pp, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (K + 1))
    L, _ = tr.gains(d, K)
    S0 = _s0(x)
    sp = _sp(name, c.nu)
    n = 14 + c.nu
    vt = vehicle_tiles_batch(c, x, u, s)
    veh = dict(vehicle=(np.zeros(6), sp), vtile=vt)
    r64, rld, ref = _cov_reference(po, x, u, d, K, L, S0, sp, vt)
    Z = np.zeros((14, 14))
    rep, psig = nav_path_sigma_batch(c, x, u, d, L, S0, Z, None, None, dense=("sens",), **veh)
    _check_psig("%s nav form, N0 = 0, m = 0" % name, po, K, n + 14, psig, r64["psig"], rld["psig"])
    e_ref, jmax = float(np.abs(r64["J"] - rld["J"]).max()), float(np.abs(rld["J"]).max())
    e = float(np.abs(rep.sens - rld["J"]).max())
    print("%s nav form sens: device-vs-longdouble %.3e (float64 reference %.3e), max %.3e" % (name, e, e_ref, jmax))
    assert e <= 8.0 * e_ref + 4.0 * EPS * jmax
    for m in (3, 6):
        H, rm = nm.position_model(x[0, 0]) if m == 3 else pv_model(x[0, 0])
        assert np.shape(H)[0] == m
        plain = nav_cov_batch(c, x, u, d, L, S0, S0, H, rm, dense=True)
        dev = nav_cov_batch(c, x, u, d, L, S0, S0, H, rm, dense=("sig", "navsig", "kf", "joint", "sens"), **veh)
        assert np.array_equal(dev.joint[:, :, n:, :], plain.joint[:, :, n:, :]) and np.array_equal(dev.joint[:, :, :, n:], plain.joint[:, :, :, n:])
        assert np.array_equal(dev.navsig, plain.navsig) and np.array_equal(dev.kf, plain.kf)
        assert np.array_equal(dev.navraw[:, :6], plain.navraw[:, :6])
        q64 = cv.nav_run(po, x, u, d, K, L, S0, S0, H, rm, sp, vt)
        qld = cv.nav_run(po, x, u, d, K, L, S0, S0, H, rm, sp, vt, dtype=np.longdouble)
        N = n + 14
        for nm_, got, f64, fld in (("joint", dev.joint, q64["joint"], qld["joint"]), ("EST", dev.navraw[:, 6:], q64["navrep"][:, 6:], qld["navrep"][:, 6:]),
                                   ("SIG_R", dev.SIG_R, q64["report"][:, cr.IDX["SIG_R"]], qld["report"][:, cr.IDX["SIG_R"]]),
                                   ("S_THRUST", dev.S_THRUST, q64["report"][:, cr.IDX["S_THRUST"]], qld["report"][:, cr.IDX["S_THRUST"]])):
            er = float(np.abs(f64 - fld).max())
            bound = max(16.0 * er, K * N * EPS * float(np.abs(fld).max()))
            e = float(np.abs(got - fld).max())
            print("%s nav form m = %d %s: device-vs-longdouble %.3e (float64 reference %.3e, bound %.3e)" % (name, m, nm_, e, er, bound))
            assert e <= bound, (name, m, nm_)
        _, ps = nav_path_sigma_batch(c, x, u, d, L, S0, S0, H, rm, **veh)
        _check_psig("%s nav form m = %d" % (name, m), po, K, N, ps, q64["psig"], qld["psig"])
        assert np.all(dev.navraw[:, 6] > plain.navraw[:, 6])           # EST_R receives J P J' in its truth term
    c.close()


def test_landing_rows_against_the_sampled_sensitivity():
    """sens[:, K, 0:14] against vehicle_sensitivity_batch (central differences of twelve sampled flights) at h and h / 2, extrapolated"""
    from oracle import dynamics as od
    from successiveconvexification_amd.dynamics import (IntegratorCache, cov_propagate_batch, linearize_batch, vehicle_sensitivity_batch,
                                                          vehicle_tiles_batch)
    pp, po, dyn, par, x, u, s, K = _case("golden", None)
    c = IntegratorCache(pp, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (K + 1))
    L, _ = tr.gains(d, K)
    h = cv.H_FD
    J1, J2 = vehicle_sensitivity_batch(c, x, u, s, L, h=h), vehicle_sensitivity_batch(c, x, u, s, L, h=0.5 * h)
    ext = (4.0 * J2 - J1) / 3.0
    trunc = np.abs(J2 - ext)
    th = np.zeros((8, 6))
    for i in range(4):
        th[2 * i, i], th[2 * i + 1, i] = h, -h
    A = max(vr.sensitivity(od, po, x[b], u[b], s[b], L[b], np.zeros((8, 14)), 10, th, 1e-9, par=par) for b in range(2))
    sp = _sp("golden", 3)
    dev = cov_propagate_batch(c, x, u, d, L, _s0(x), dense=("sens",), vehicle=(np.zeros(6), sp), vtile=vehicle_tiles_batch(c, x, u, s))
    err = np.abs(dev.sens[:, K, :14] - ext)
    bound = trunc + cv.rounding(K, 0.5 * h, A)
    print("landing rows: column norms %s; sens against the sampled central differences %.3e, bound %.3e .. %.3e (A_cl %.3f)"
          % (np.linalg.norm(dev.sens[0, K, :14], axis=0), err.max(), bound.min(), bound.max(), A))
    assert np.all(err <= bound)
    c.close()


def test_statistics_on_the_devices_own_sampler():
    """8 x 1,024 independent flights of golden plan 0 with vehicle=, rng="device", dense pathv: the pooled landing covariance against
    covK^tot, the per-node standard deviations of the mass and of the commanded thrust norm against psig^tot; the same flown on an
    estimate against the navigation form"""
    import nav_margin_reference as nm
    from test_cov_vehicle_cpu import golden_case
    from successiveconvexification_amd.dynamics import (IntegratorCache, cov_path_sigma_batch, cov_propagate_batch, linearize_batch,
                                                          nav_cov_batch, nav_path_sigma_batch, track_gains_batch, track_mc_batch,
                                                          track_mc_nav_batch, vehicle_tiles_batch)
    B, S = 8, 1024
    N = B * S
    p, par, x, u, s, d_ref, L_ref, S0, covK_ref, J_fd = golden_case()[:10]
    c = IntegratorCache(_flyable()[0], npts=10)
    sl = slice(0, 1)
    x, u, s = x[sl], u[sl], s[sl]
    _, d = linearize_batch(c, x, u, s, 1.0 / (p.K + 1))
    L = track_gains_batch(c, d)
    sp = np.zeros(6)
    sp[:3] = vr.equal_share_sp(J_fd, (0, 1, 2), float(np.trace(covK_ref)))
    sp[3] = sp[0]
    veh = (np.zeros(6), sp)
    vt = vehicle_tiles_batch(c, x, u, s)
    rep8 = lambda a: np.repeat(np.asarray(a)[:1], B, axis=0)   # noqa: E731
    H, rm = nm.position_model(x[0, 0])

    def check(tag, pathv, xland, covK, covK0, psig):
        xcov = np.cov((xland - x[0, -1]).reshape(N, 14), rowvar=False)
        worst, over = mr.se_check(xcov, covK, N)
        worst0, over0 = mr.se_check(xcov, covK0, N)
        out = {}
        for nm_, col in (("mass", 0), ("thrust", 4)):
            sd = np.transpose(pathv[:, 1:, col], (0, 2, 1)).reshape(N, -1).std(axis=0, ddof=1)
            ref = psig[1:, col]
            out[nm_] = float((np.abs(sd - ref) / cv.sd_stderr(ref, N)).max())
        print("%s, sp %.3e, 8 x 1,024 flights: landing covariance worst entry %.2f standard errors, %d over 6 (without J %.2f, %d over 6); "
              "worst node: mass %.2f, commanded thrust %.2f standard errors" % (tag, sp[0], worst, over, worst0, over0, out["mass"], out["thrust"]))
        assert over == 0 and over0 > 0 and out["mass"] <= 6.0 and out["thrust"] <= 6.0

    r = track_mc_batch(c, rep8(x), rep8(u), rep8(s), rep8(L), S0, S, seed=0, nsub=10, rng="device", independent=True, dense=("xland", "pathv"),
                       vehicle=veh)
    tot = cov_propagate_batch(c, x, u, d, L, S0[None], dense=("covK",), vehicle=veh, vtile=vt)
    base = cov_propagate_batch(c, x, u, d, L, S0[None], dense=("covK",))
    psig = cov_path_sigma_batch(c, x, u, d, L, S0[None], vehicle=veh, vtile=vt)[1][0]
    assert r.N_BAD.sum() == 0
    check("truth-fed", r.pathv, r.xland, tot.covK[0][:14, :14], base.covK[0][:14, :14], psig)
    rn = track_mc_nav_batch(c, rep8(x), rep8(u), rep8(s), rep8(d), rep8(L), S0, S0, H, rm, S, seed=0, nsub=10, rng="device", independent=True,
                            dense=("xland", "pathv"), vehicle=veh)
    n = 14 + c.nu
    jt = nav_cov_batch(c, x, u, d, L, S0[None], S0[None], H, rm, dense=("joint",), vehicle=veh, vtile=vt).joint[0, -1][:14, :14]
    j0 = nav_cov_batch(c, x, u, d, L, S0[None], S0[None], H, rm, dense=("joint",)).joint[0, -1][:14, :14]
    psn = nav_path_sigma_batch(c, x, u, d, L, S0[None], S0[None], H, rm, vehicle=veh, vtile=vt)[1][0]
    assert rn.N_BAD.sum() == 0 and n == 17
    check("flown on an estimate", rn.pathv, rn.xland, jt, j0, psn)
    c.close()


@pytest.mark.parametrize("tiles", ["double", "float"])
def test_batch_calls_are_the_manual_sequence_bit_for_bit(tiles):
    """margins_from_cov(vehicle=) and margins_from_nav(vehicle=): tiles, then path sigma, then min(nsigma s, cap width); covariance() and
    navigation() with vehicle= are the one-shot calls on the batch's own tiles.  Float tiles go through the batch call."""
    from successiveconvexification_amd.dynamics import (cov_path_sigma_batch, cov_propagate_batch, nav_cov_batch, nav_path_sigma_batch,
                                                          vehicle_tiles_batch)
    from test_gpu_nav_margins import _fixture
    from test_gpu_path_margins import _formula, _plans
    pp, c, b, x, u, s = _plans(50, tiles == "float")
    f = _fixture()
    S0, N0, H, rm = f["S0"], f["N0"], f["H"], f["rm"]
    veh = (np.zeros(6), _sp("golden", 3))
    d = b.linearization()[1]
    L = b.track_gains()
    vt = vehicle_tiles_batch(c, x, u, s)
    ps = b.margins_from_cov(S0, vehicle=veh)
    one = cov_path_sigma_batch(c, x, u, d, L, S0, vehicle=veh, vtile=vt)[1]
    lo, pm = _formula(pp, x, one, 3.0, 0.25)
    assert np.array_equal(ps, one) and np.array_equal(b.path_sigma(S0, vehicle=veh), one)
    assert np.array_equal(b.thrust_margins()[0], lo) and np.array_equal(b.thrust_margins()[1], lo) and np.array_equal(b.path_margins(), pm)
    assert np.all(ps[:, 2:, 4] > b.path_sigma(S0)[:, 2:, 4])      # the command of node 1 is L_0 z_0: it has not seen theta yet
    ps = b.margins_from_nav(S0, N0, H, rm, vehicle=veh)
    one = nav_path_sigma_batch(c, x, u, d, L, S0, N0, H, rm, vehicle=veh, vtile=vt)[1]
    lo, pm = _formula(pp, x, one, 3.0, 0.25)
    assert np.array_equal(ps, one) and np.array_equal(b.path_sigma(S0, nav=(N0, H, rm), vehicle=veh), one)
    assert np.array_equal(b.thrust_margins()[0], lo) and np.array_equal(b.path_margins(), pm)
    r = b.covariance(S0, dense=True, vehicle=veh)
    o = cov_propagate_batch(c, x, u, d, L, S0, dense=True, vehicle=veh, vtile=vt)
    assert np.array_equal(r.raw, o.raw) and np.array_equal(r.cov, o.cov) and np.array_equal(r.sig, o.sig)
    r = b.navigation(S0, N0, H, rm, dense=("joint",), vehicle=veh)
    o = nav_cov_batch(c, x, u, d, L, S0, N0, H, rm, dense=("joint",), vehicle=veh, vtile=vt)
    assert np.array_equal(r.raw, o.raw) and np.array_equal(r.navraw, o.navraw) and np.array_equal(r.joint, o.joint)
    b.close(), c.close()


def test_robustify_with_vehicle_errors_converges_and_keeps_more_headroom():
    """one round of robustify(S0, vehicle=) on the two plans of oracle_nav_margin_runs.npz: converged, and in the vehicle-aware report
    N_TMIN and N_TMAX lie above those of a twin robustified without vehicle"""
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache
    from test_gpu_nav_margins import _fixture
    f = _fixture()
    pp, po = _flyable()
    c = IntegratorCache(pp, npts=10)
    veh = (np.zeros(6), np.array([1e-3, 1e-3, 1e-3, 1e-3, 0.0, 0.0]))
    twin, mine = (ScvxBatch(c, f["ic"].shape[0]).init(f["ic"]) for _ in range(2))
    for b in (twin, mine):
        assert np.all(b.solve()[0] == 0)
    r0 = twin.covariance(f["S0"], vehicle=veh)
    print("before: vehicle-aware report SIG_R %s N_TMIN %s N_TMAX %s; plain report SIG_R %s N_TMIN %s N_TMAX %s"
          % (r0.SIG_R, r0.N_TMIN, r0.N_TMAX, twin.covariance(f["S0"]).SIG_R, twin.covariance(f["S0"]).N_TMIN, twin.covariance(f["S0"]).N_TMAX))
    st0, it0 = twin.robustify(f["S0"], nsigma=3, rounds=1)[:2]
    st1, it1, _, _, lo, hi = mine.robustify(f["S0"], nsigma=3, rounds=1, vehicle=veh)
    rt, rm_ = twin.covariance(f["S0"], vehicle=veh), mine.covariance(f["S0"], vehicle=veh)
    print("robustify(vehicle=): status %s in %s steps (twin without: %s in %s); final mass %s (twin %s); back-offs up to %s"
          % (st1, it1, st0, it0, mine.trajectory()[0][:, -1, 0], twin.trajectory()[0][:, -1, 0], lo.max(axis=1)))
    print("vehicle-aware report afterwards: N_TMIN %s (twin %s), N_TMAX %s (twin %s), SIG_R %s (twin %s)"
          % (rm_.N_TMIN, rt.N_TMIN, rm_.N_TMAX, rt.N_TMAX, rm_.SIG_R, rt.SIG_R))
    assert np.all(st1 == 0) and np.all(st0 == 0)
    assert np.all(rm_.N_TMIN > rt.N_TMIN) and np.all(rm_.N_TMAX > rt.N_TMAX)
    with pytest.raises(ValueError):
        mine.robustify(f["S0"], vehicle=veh, mc=dict(samples=64))
    twin.close(), mine.close(), c.close()


def test_refusals(aero_tables):
    """every refusal of include/scvx.h answers SCVX_ERR_ARG (-1) from C; Python raises ValueError before the call"""
    import ctypes as C
    from successiveconvexification_amd.dynamics import IntegratorCache, cov_propagate_batch, linearize_batch, nav_cov_batch, vehicle_tiles_batch
    pp, po, dyn, par, x, u, s, K = _case("exo", aero_tables)
    c = IntegratorCache(pp, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (K + 1))
    L, _ = tr.gains(d, K)
    S0 = _s0(x)
    vt = vehicle_tiles_batch(c, x, u, s)
    B = x.shape[0]
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
    ERR_ARG = -1   # SCVX_ERR_ARG
    rep, nrep = np.empty((B, 16)), np.empty((B, 8))
    xs, us, ds, Ls = (np.ascontiguousarray(a) for a in (x, u, d, L))

    def cov(sp, vtile=vt, s0=S0, K_=K):
        return c._L.scvx_cov_vehicle_f64_host(c.handle, B, K_, p(xs), p(us), p(ds), p(Ls), p(s0) if s0 is not None else None, None, p(rep), None,
                                              None, None, None, p(vtile) if vtile is not None else None, p(sp) if sp is not None else None, None)

    def nav(sp, vtile=vt, m=0):
        return c._L.scvx_nav_cov_vehicle_f64_host(c.handle, B, K, p(xs), p(us), p(ds), p(Ls), p(S0), p(S0), m, None, None, None, p(rep), p(nrep),
                                                  None, None, None, None, None, p(vtile) if vtile is not None else None, p(sp), None)
    ok = np.array([1e-3, 0, 0, 1e-3, 0, 0.0])
    assert cov(ok) == 0 and nav(ok) == 0
    assert cov(np.array([1e-3, 0, 0, 0, 0, 0.0]), vtile=None) == 0                   # no tiles needed without ISP and AERO
    for bad in (np.array([-1e-3, 0, 0, 0, 0, 0.0]), np.array([np.nan, 0, 0, 0, 0, 0.0]), np.array([0, 0, 0, np.inf, 0, 0.0]),
                np.array([0, 0, 0, 0, 1e-3, 0.0]), np.array([0, 0, 0, 0, 0, 1e-3])):
        assert cov(bad) == ERR_ARG == nav(bad), bad
    assert cov(None) == ERR_ARG
    assert cov(ok, vtile=None) == ERR_ARG == nav(ok, vtile=None)               # ISP without the tiles
    assert cov(ok, s0=None) == ERR_ARG and cov(ok, K_=K + 1) == ERR_ARG   # what the call extended refuses
    assert nav(ok, m=15) == ERR_ARG
    assert c._L.scvx_vehicle_tiles_f64_host(c.handle, B, K, p(xs), p(us), None, p(vt)) == ERR_ARG
    assert c._L.scvx_vehicle_tiles_f64_host(c.handle, -1, K, p(xs), p(us), p(np.ascontiguousarray(s)), p(vt)) == ERR_ARG
    for kw in (dict(vehicle=(np.full(6, 1e-3), np.zeros(6))), dict(vehicle=(np.zeros(6), np.array([0, 0, 0, 0, 1e-3, 0.0])), vtile=vt),
               dict(vehicle=(np.zeros(6), ok)), dict(dense=("sens",))):
        with pytest.raises(ValueError):
            cov_propagate_batch(c, x, u, d, L, S0, **kw)
        with pytest.raises(ValueError):
            nav_cov_batch(c, x, u, d, L, S0, S0, None, None, **kw)
    c.close()
