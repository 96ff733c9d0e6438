"""Clamp-aware covariance analysis (scvx_cov_clamp_f64[_host], scvx_batch_cov_clamp) on the MI355X against the independent CPU reference
(tests/cov_clamp_reference.py: the recursion of include/scvx.h in numpy with the full F, G, N, Mtilde, float64 and longdouble with
mpmath's erfc and exp), against the plain call where nobody reaches the band, and against the device's own sampled clamped flights.

Shapes: K = 3 on exo, aero + fins and aero + fins + torque (horizon_cases.case: random-but-physical plans, B = 3 and its first row as
B = 1) and K = 50 on the two golden plans; both SCVX_COV_MFMA forms; double tiles, and float tiles through the batch call.
Bounds, none of them taken from the device:
  * parity (reference gains fed to both sides): every entry of mean, sig, covK, cov, and every column of satk and satrep, within
    8 e_ref + 4 * 2^-52 * scale of the longdouble reference, e_ref the float64 reference's own largest distance from it in that array
    (column) and scale the array's (column's) largest magnitude -- 1 for GAIN_MIN, which is 1 - P_lo - P_hi: a difference of terms of
    size 1.  Three bands: the problem's own, one that clamps only from below (Tmin, inf), one that clamps at every node (Tlo == Thi).
  * the anchor: the four conditions of test_cov_clamp_cpu.py on the device's own flights, gains and analyses.
Every comparison prints its figures before it asserts."""
import ctypes as C
import os

import numpy as np
import pytest

import cov_clamp_reference as sl
import cov_reference as cr
import horizon_cases as hc
import track_reference as tr
from conftest import GOLDEN
from test_gpu_flight import _flyable

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
CASES = ("exo K=3", "aero+fins K=3", "aero+fins+torque K=3", "golden K=50")
BANDS = ("own", "below", "pinned")
_REF, _WORST = {}, {}
_dp = C.POINTER(C.c_double)


def _case(name, tables):
    """(pp, po, x, u, sigma) of a case name"""
    if name.startswith("golden"):
        g = np.load(os.path.join(GOLDEN, "oracle_flight_runs.npz"))
        pp, po = _flyable()
        return pp, po, g["x"], g["u"], g["sigma"]
    pp, po, _, _, x, u, s = hc.case(name.split()[0], 3, tables)
    return pp, po, x, u, s


def _band(name, po):
    return {"own": None, "below": (po.Tmin, np.inf), "pinned": (0.5 * (po.Tmin + po.Tmax),) * 2}[name]


def _s0(x):
    return np.stack([cr.handover_s0(x[b, 0])[0] for b in range(x.shape[0])])


def _reference(name, band, po, u, d, K, S0):
    """(L, float64 outputs, longdouble outputs) under the REFERENCE's gains, each with sig, covK and satrep"""
    if (name, band) not in _REF:
        L, _ = tr.gains(d, K)
        outs = []
        for dt in (np.float64, np.longdouble):
            o = sl.propagate(u, d, K, L, S0, (po.Tmin, po.Tmax) if _band(band, po) is None else _band(band, po), None, dt)
            dg = np.diagonal(o["cov"], axis1=-2, axis2=-1)
            o["sig"], o["covK"], o["satrep"] = np.sqrt(np.where(dg > 0, dg, 0)), o["cov"][:, -1], sl.satrep(o, dt)
            outs.append(o)
        _REF[(name, band)] = (L, outs[0], outs[1])
    return _REF[(name, band)]


def _check_parity(tag, dev, f64, fld):
    """the yardstick of the module docstring on every output; returns the worst error / bound"""
    worst = 0.0
    items = [(k, getattr(dev, k), f64[k], fld[k], None) for k in ("mean", "sig", "covK", "cov")]
    items += [("satk[%s]" % n, dev.satk[:, :, i], f64["satk"][:, :, i], fld["satk"][:, :, i], None)
              for i, n in enumerate(("That", "s", "P_lo", "P_hi"))]
    items += [("satrep[%s]" % n, dev.satraw[:, i], f64["satrep"][:, i], fld["satrep"][:, i], 1.0 if n == "GAIN_MIN" else None)
              for n, i in sl.IDX.items()]
    for name, got, a64, ald, scale in items:
        assert np.isfinite(got).all(), (tag, name)
        e_ref = float(np.abs(a64 - ald).max())
        scale = float(np.abs(ald).max()) if scale is None else scale
        bound = 8.0 * e_ref + 4.0 * EPS * scale
        e = float(np.abs(got - ald).max())
        ratio = e / bound if bound > 0 else (0.0 if e == 0 else np.inf)
        worst = max(worst, ratio)
        print("%s %-18s device-vs-longdouble %.3e (float64 reference %.3e, bound %.3e, scale %.3e) ratio %.3f" % (tag, name, e, e_ref, bound, scale, ratio))
        assert e <= bound, (tag, name, e, bound)
    assert np.array_equal(dev.cov, np.swapaxes(dev.cov, -1, -2)) and np.array_equal(dev.cov[:, -1], dev.covK)
    return worst


@pytest.mark.parametrize("mfma", ["0", "1"])
@pytest.mark.parametrize("name", CASES)
def test_parity_with_the_reference(name, mfma, aero_tables, monkeypatch):
    from successiveconvexification_amd.dynamics import IntegratorCache, cov_propagate_batch, linearize_batch
    monkeypatch.setenv("SCVX_COV_MFMA", mfma)
    pp, po, x, u, s = _case(name, aero_tables)
    K = x.shape[1] - 1
    c = IntegratorCache(pp, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (K + 1))
    S0 = _s0(x)
    for band in BANDS:
        L, f64, fld = _reference(name, band, po, u, d, K, S0)
        dev = cov_propagate_batch(c, x, u, d, L, S0, dense=True, clamp=True, band=_band(band, po))
        assert dev.mean.shape == (x.shape[0], K + 1, 14 + c.nu) and dev.satk.shape == (x.shape[0], K, 4)
        tag = "%s band %s SCVX_COV_MFMA=%s" % (name, band, mfma)
        print("%s: P_lo %s P_hi %s GAIN_MIN %s" % (tag, dev.P_LO, dev.P_HI, dev.GAIN_MIN))
        w = _check_parity(tag, dev, f64, fld)
        one = cov_propagate_batch(c, x[:1], u[:1], d[:1], L[:1], S0[:1], dense=True, clamp=True, band=_band(band, po))   # B = 1
        for k in ("raw", "satraw", "mean", "sig", "covK", "cov", "satk"):
            assert np.array_equal(getattr(one, k), getattr(dev, k)[:1]), (tag, k)
        lean = cov_propagate_batch(c, x, u, d, L, S0, clamp=True, band=_band(band, po))
        assert np.array_equal(lean.raw, dev.raw) and np.array_equal(lean.satraw, dev.satraw) and lean.mean is None and lean.satk is None
        _WORST[(name, band, mfma)] = w
    c.close()


def test_worst_parity_ratio_of_the_module():
    """runs after the parity tests: the figure profiles/cov_clamp.md quotes"""
    assert _WORST
    k = max(_WORST, key=_WORST.get)
    print("worst error / bound over %d parity runs: %.3f at %s" % (len(_WORST), _WORST[k], k))
    assert _WORST[k] <= 1.0


@pytest.mark.parametrize("mfma", ["0", "1"])
@pytest.mark.parametrize("name", CASES)
def test_a_band_nobody_reaches_is_bitwise_the_plain_call(name, mfma, aero_tables, monkeypatch):
    from successiveconvexification_amd.dynamics import IntegratorCache, cov_propagate_batch, linearize_batch
    monkeypatch.setenv("SCVX_COV_MFMA", mfma)
    pp, po, x, u, s = _case(name, aero_tables)
    K = x.shape[1] - 1
    c = IntegratorCache(pp, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (K + 1))
    S0, L = _s0(x), tr.gains(d, K)[0]
    w = np.random.default_rng(5).uniform(0.0, 1e-8, 14)
    for noise in (None, w):
        plain = cov_propagate_batch(c, x, u, d, L, S0, noise, dense=True)
        sat = cov_propagate_batch(c, x, u, d, L, S0, noise, dense=True, clamp=True, band=(0.0, np.inf))
        for k in ("raw", "sig", "covK", "cov"):
            assert np.array_equal(getattr(sat, k), getattr(plain, k)), (name, k)
        assert not sat.mean.any() and not sat.satk[:, :, 2:].any() and np.all(sat.GAIN_MIN == 1.0)
        assert not sat.satraw[:, sl.IDX["BIAS_M"]:sl.IDX["BIAS_W"] + 1].any() and not sat.BIAS_PEAK.any() and not sat.P_LO.any()
        assert np.array_equal(sat.satraw[:, :5], plain.raw[:, :5]) and np.array_equal(sat.RMS_R, plain.SIG_R)
    c.close()


def _device_form(c, x, u, d, L, S0, band, dense=True):
    """scvx_cov_clamp_f64 on another framework's device arrays: a SatCovReport"""
    import torch
    from successiveconvexification_amd.dynamics import SatCovReport
    B, K1, n = x.shape[0], x.shape[1], 14 + c.nu
    up = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")   # noqa: E731
    ins = [up(a) for a in (x, u, d, L, S0)]
    shapes = [(B, 16), (B, 16), (B, K1, n), (B, K1, n), (B, n, n), (B, K1, n, n), (B, K1 - 1, 4)]
    outs = [torch.zeros(sh, dtype=torch.float64, device="cuda") for sh in shapes]
    torch.cuda.synchronize()
    bd = None if band is None else np.ascontiguousarray(band, np.float64)
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    rc = c._L.scvx_cov_clamp_f64(c.handle, B, K1 - 1, *[ptr(t) for t in ins], None, None if bd is None else bd.ctypes.data_as(_dp),
                                 *[ptr(t) if dense or i < 2 else None for i, t in enumerate(outs)])
    assert rc == 0, c._L.scvx_last_error(c.handle)
    c.synchronize()
    o = [t.cpu().numpy() for t in outs]
    return SatCovReport(o[0], o[1], *(o[2:] if dense else ()))


def test_launches_and_forms_agree_bit_for_bit():
    """two launches; the _host form, the form on device arrays and the batch form (double tiles, and float tiles widened on load)"""
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache, cov_propagate_batch
    g = np.load(os.path.join(GOLDEN, "oracle_flight_runs.npz"))
    pp, po = _flyable()
    x, u, s = g["x"], g["u"], g["sigma"]
    c = IntegratorCache(pp, npts=10)
    b = ScvxBatch(c, 2).init(None)
    b.set_trajectory(x, u, s)
    before = (b.trajectory_record(),) + b.scalars() + b.flags() + b.linearization()
    S0 = _s0(x)
    keys = ("raw", "satraw", "mean", "sig", "covK", "cov", "satk")
    for f32 in (False, True):
        b.set_linearization_f32(f32)
        d = b.linearization()[1]
        L = b.track_gains()
        for band in BANDS:
            bd = _band(band, po)
            host = cov_propagate_batch(c, x, u, d, L, S0, dense=True, clamp=True, band=bd)
            again = cov_propagate_batch(c, x, u, d, L, S0, dense=True, clamp=True, band=bd)
            dev = _device_form(c, x, u, d, L, S0, bd)
            own = b.covariance(S0, dense=True, clamp=True, band=bd)
            for k in keys:
                for other in (again, dev, own):
                    assert np.array_equal(getattr(host, k), getattr(other, k)), (f32, band, k)
            lean = b.covariance(S0, clamp=True, band=bd)
            assert np.array_equal(lean.satraw, host.satraw) and lean.cov is None
            print("tiles %s band %s: P_LO %s P_HI %s GAIN_MIN %s BIAS_R %s SIG_R %s" % ("float" if f32 else "double", band, host.P_LO,
                                                                                       host.P_HI, host.GAIN_MIN, host.BIAS_R, host.SIG_R))
        if f32:
            assert np.array_equal(d, d.astype(np.float32).astype(np.float64))
    b.set_linearization_f32(False)
    after = (b.trajectory_record(),) + b.scalars() + b.flags() + b.linearization()
    for a0, a1 in zip(before, after):
        assert np.array_equal(a0, a1, equal_nan=True)
    b.close(), c.close()


def test_a_nan_poisons_only_its_own_trajectory(aero_tables):
    from successiveconvexification_amd.dynamics import IntegratorCache, cov_propagate_batch, linearize_batch
    pp, po, x, u, s = _case("aero+fins K=3", aero_tables)
    x, u, s = (np.concatenate([a, a[:2]]) for a in (x, u, s))       # B = 5
    c = IntegratorCache(pp, npts=10)
    _, d = linearize_batch(c, x, u, s, 0.25)
    S0, L = _s0(x), tr.gains(d, 3)[0]
    keys = ("raw", "satraw", "mean", "sig", "covK", "cov", "satk")
    dn, gn, sn = d.copy(), L.copy(), S0.copy()
    dn.reshape(5, 3, -1, 14)[1, 1, 2, 5] = np.nan
    gn[3, 2, 1, 4] = np.inf
    sn[4, 2, 2] = np.nan
    for mf in ("0", "1"):
        os.environ["SCVX_COV_MFMA"] = mf
        try:
            good = cov_propagate_batch(c, x, u, d, L, S0, dense=True, clamp=True)
            pois = cov_propagate_batch(c, x, u, dn, gn, sn, dense=True, clamp=True)
        finally:
            del os.environ["SCVX_COV_MFMA"]
        assert np.isnan(pois.raw[[1, 3, 4]]).all() and np.isnan(pois.satraw[[1, 3, 4]]).all(), (pois.raw, pois.satraw)
        for k in keys:
            assert np.array_equal(getattr(pois, k)[[0, 2]], getattr(good, k)[[0, 2]]), k
        assert np.array_equal(pois.cov[1, :2], good.cov[1, :2]) and np.isnan(pois.cov[1, 2]).any()
    c.close()


# ---- refusals: (rc, scvx_last_error) of every case equals tests/golden/cov_clamp_refusals.txt --------------------------------------
def refusal_lines():
    """One exo problem, B = 2, K = 3.  Every form starts from a valid call; one argument (or two) is made bad; a refused call leaves the
    outputs at their fill.  The context-level forms are refused before a device pointer is used."""
    from dataclasses import replace
    from successiveconvexification_amd import sample_problems as sp
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache
    B, K, n, NAN, INF = 2, 3, 17, float("nan"), float("inf")
    c = IntegratorCache(replace(sp.base_prob_scaled, K=K), npts=10)
    b, fresh = ScvxBatch(c, B).init(None), ScvxBatch(c, B)
    Lb = c._L

    def args():
        a = dict(B=B, K=K, x=np.ones((B, K + 1, 14)), u=np.ones((B, K + 1, 3)), deriv=np.zeros((B, K, 21, 14)), gain=np.zeros((B, K, 3, n)),
                 S0=np.ascontiguousarray(np.stack([np.eye(14) * 1e-6] * B)), w=np.full(14, 1e-6), band=np.array([0.1, 0.9]),
                 q=np.ones(14), r=np.ones(3), qf=np.full(14, 100.0))
        for name, shape in (("report", (B, 16)), ("satrep", (B, 16)), ("mean", (B, K + 1, n)), ("sig", (B, K + 1, n)), ("covK", (B, n, n)),
                            ("cov", (B, K + 1, n, n)), ("satk", (B, K, 4))):
            a[name] = np.full(shape, 7.0)
        return a
    outs = ("report", "satrep", "mean", "sig", "covK", "cov", "satk")

    def call(entry, a, handle=None):
        p = lambda k: None if a[k] is None else a[k].ctypes.data_as(_dp)   # noqa: E731
        if entry == "scvx_batch_cov_clamp":
            return Lb.scvx_batch_cov_clamp(b.handle if handle is None else handle, p("q"), p("r"), p("qf"), p("S0"), p("w"), p("band"),
                                           *[p(k) for k in outs])
        if entry == "scvx_cov_clamp_f64_host":
            return Lb.scvx_cov_clamp_f64_host(c.handle, a["B"], a["K"], p("x"), p("u"), p("deriv"), p("gain"), p("S0"), p("w"), p("band"),
                                              *[p(k) for k in outs])
        dv = lambda k: None if a[k] is None else C.c_void_p(1)   # noqa: E731  every check comes before a device pointer is used
        return Lb.scvx_cov_clamp_f64(c.handle, a["B"], a["K"], dv("x"), dv("u"), dv("deriv"), dv("gain"), dv("S0"), p("w"), p("band"),
                                     *[dv(k) for k in outs])

    def vec(nn, fill, i, v):
        w = np.full(nn, fill)
        w[i] = v
        return w
    ctx_only, batch_only = 1, 2
    faults = (("B=0", ctx_only, dict(B=0)), ("K=2", ctx_only, dict(K=2)), ("x=NULL", ctx_only, dict(x=None)), ("u=NULL", ctx_only, dict(u=None)),
              ("deriv=NULL", ctx_only, dict(deriv=None)), ("gain=NULL", ctx_only, dict(gain=None)), ("S0=NULL", 0, dict(S0=None)),
              ("report=NULL", ctx_only, dict(report=None)), ("satrep=NULL", ctx_only, dict(satrep=None)),
              ("w<0", 0, dict(w=vec(14, 1e-6, 2, -1e-6))), ("w=NaN", 0, dict(w=vec(14, 1e-6, 1, NAN))), ("w=inf", 0, dict(w=vec(14, 1e-6, 0, INF))),
              ("Tlo<0", 0, dict(band=np.array([-0.1, 0.9]))), ("Tlo=NaN", 0, dict(band=np.array([NAN, 0.9]))),
              ("Tlo=inf", 0, dict(band=np.array([INF, INF]))), ("Thi=NaN", 0, dict(band=np.array([0.1, NAN]))),
              ("Tlo>Thi", 0, dict(band=np.array([0.9, 0.1]))), ("Thi=-inf", 0, dict(band=np.array([0.1, -INF]))),
              ("q=NULL", batch_only, dict(q=None)), ("r=0", batch_only, dict(r=np.array([1.0, 0.0, 1.0]))),
              ("qf=NaN", batch_only, dict(qf=vec(14, 100.0, 13, NAN))))
    pairs = (("S0=NULL", "w<0"), ("S0=NULL", "Tlo<0"), ("w=NaN", "Tlo>Thi"), ("satrep=NULL", "Thi=NaN"), ("satrep=NULL", "w<0"),
             ("Tlo<0", "q=NULL"), ("w<0", "r=0"), ("x=NULL", "Tlo=NaN"))
    table = {n: (need, kw) for n, need, kw in faults}
    lines, valid = [], []
    try:
        for entry in ("scvx_cov_clamp_f64_host", "scvx_cov_clamp_f64", "scvx_batch_cov_clamp"):
            mine = batch_only if entry.startswith("scvx_batch") else ctx_only
            ok = lambda nm: table[nm][0] in (0, mine)   # noqa: E731
            cases = [(nm,) for nm, _, _ in faults if ok(nm)] + [pr for pr in pairs if ok(pr[0]) and ok(pr[1])]
            if mine == batch_only:
                cases.append(("uninitialised",))
            for case in cases:
                a = args()
                for nm in case:
                    if nm in table:
                        a.update(table[nm][1])
                rc = call(entry, a, fresh.handle if case == ("uninitialised",) else None)
                lines.append("cov-clamp-refusal %s %s %d %s" % (entry, "+".join(case), rc, Lb.scvx_last_error(c.handle).decode()))
                assert rc != 0 and all(a[k] is None or np.all(a[k] == 7.0) for k in outs), lines[-1]
        # the valid calls: Thi = +inf and Tlo = 0 are allowed, band2 = NULL is the problem's band, every output of the batch form optional
        for tag, kw in (("valid", {}), ("band=NULL", dict(band=None)), ("band=(0,inf)", dict(band=np.array([0.0, INF]))),
                        ("Tlo=Thi", dict(band=np.array([0.3, 0.3]))), ("w=NULL", dict(w=None))):
            for entry in ("scvx_cov_clamp_f64_host", "scvx_batch_cov_clamp"):
                a = args()
                a.update(kw)
                valid.append("cov-clamp-refusal %s %s %d -" % (entry, tag, call(entry, a)))
        a = args()
        a.update({k: None for k in outs})
        valid.append("cov-clamp-refusal scvx_batch_cov_clamp outputs=NULL %d -" % call("scvx_batch_cov_clamp", a))
    finally:
        b.close(), fresh.close(), c.close()
    return lines + valid


def test_every_refusal_answers_with_its_word():
    """the words: "B >= 1", "K must equal", "null buffer", "w must be", "band2 must be", the tracking weights' own, the batch's own"""
    got = refusal_lines()
    with open(os.path.join(GOLDEN, "cov_clamp_refusals.txt")) as f:
        want = f.read().splitlines()
    assert len(want) > 60 and all(line.startswith("cov-clamp-refusal scvx_") for line in want)
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want)
    assert all(line.endswith(" 0 -") for line in got if line.endswith(" -")) and sum(line.endswith(" -") for line in got) == 11


def test_python_layers_and_their_refusals():
    from successiveconvexification_amd import _lib, montecarlo as mc, rocketland as rl, sample_problems as sp
    from successiveconvexification_amd.dynamics import IntegratorCache, SatCovReport
    p = sp.base_prob_scaled
    c = IntegratorCache(p, npts=10)
    ip = rl.create_initial(p, c)
    ip, _, _ = rl.solve_step(ip, c)
    sd = np.zeros(14)
    sd[1:7] = 1e-3
    r = rl.covariance(ip, c, sd, dense=True, clamp=True)
    assert isinstance(r, SatCovReport) and len(r) == 1 and r.mean.shape == (1, p.K + 1, 17) and r.satk.shape == (1, p.K, 4)
    assert np.isfinite(r.satraw).all() and 0.0 <= r.GAIN_MIN[0] <= 1.0
    rb = ip.model.covariance(sd, dense=True, clamp=True)
    assert np.array_equal(r.satraw, rb.satraw) and np.array_equal(r.cov, rb.cov) and np.array_equal(r.mean, rb.mean)
    wide = rl.covariance(ip, c, sd, clamp=True, band=(0.0, np.inf))
    assert np.array_equal(wide.raw, rl.covariance(ip, c, sd).raw) and np.all(wide.GAIN_MIN == 1.0)
    sm = mc.clamp_summary(r, np.zeros(1, int))
    assert sm["converged"] == 1 and sm["stats"]["P_LO"]["max"] == r.P_LO[0]
    veh = mc.vehicle_errors(thrust=1e-3)
    for call in (lambda: rl.covariance(ip, c, sd, clamp=True, vehicle=veh), lambda: ip.model.covariance(sd, clamp=True, vehicle=veh)):
        with pytest.raises(ValueError, match="no vehicle-error form"):
            call()
    H, rm = np.eye(14)[1:4], np.full(3, 1e-6)
    for call in (lambda: rl.navigation(ip, c, sd, sd, H, rm, clamp=True), lambda: ip.model.navigation(sd, sd, H, rm, clamp=True)):
        with pytest.raises(ValueError, match="no navigation form"):
            call()
    with pytest.raises(ValueError, match="band"):
        rl.covariance(ip, c, sd, clamp=True, band=(0.5, 0.4))
    with pytest.raises(ValueError, match="needs clamp"):
        ip.model.covariance(sd, band=(0.1, 0.9))
    with pytest.raises(_lib.ScvxError, match="w must be"):
        ip.model.covariance(sd, w=-1.0, clamp=True)
    c.close()


@pytest.mark.parametrize("scale", [0.1, 1.0])
def test_device_anchor_against_its_own_sampled_clamped_flights(scale):
    """THE DEVICE'S ANCHOR.  Golden plan 0 under the device's gains: 8 x 1,024 independent clamped flights of scvx_track_mc (draws made
    on the device, every row a stream of its own) pooled, against the device's scvx_cov_clamp_f64 and scvx_cov_propagate_f64: the four
    conditions of test_cov_clamp_cpu.py's anchor."""
    from successiveconvexification_amd.dynamics import IntegratorCache, cov_propagate_batch, linearize_batch, track_gains_batch, track_mc_batch
    g = np.load(os.path.join(GOLDEN, "oracle_flight_runs.npz"))
    pp, po = _flyable()
    R, S = 8, 1024
    x, u, s = (np.repeat(g[k][:1], R, axis=0) for k in ("x", "u", "sigma"))
    c = IntegratorCache(pp, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (po.K + 1))
    L = track_gains_batch(c, d)
    S0 = cr.handover_s0(x[0, 0], scale=scale)[0]
    mcr = track_mc_batch(c, x, u, s, L, S0, S, seed=20261021, nsub=10, clamp=True, rng="device", independent=True)
    assert np.all(mcr.N_BAD == 0) and np.all(mcr.S == S)
    m = mcr.xmean.mean(axis=0)                                     # equal sample counts: the pooled mean
    dm = mcr.xmean - m
    pooled = ((S - 1) * mcr.xcov.sum(axis=0) + S * np.einsum("bi,bj->ij", dm, dm)) / (R * S - 1)
    sat = cov_propagate_batch(c, x[:1], u[:1], d[:1], L[:1], S0[None], dense=("covK", "mean"), clamp=True)
    lin = cov_propagate_batch(c, x[:1], u[:1], d[:1], L[:1], S0[None], dense=("covK",))
    f = sl.anchor_figures(sat.covK[0][:14, :14], sat.mean[0, -1, :14], sat.P_LO[0], sat.P_HI[0], lin.covK[0][:14, :14], m, pooled,
                          mcr.OUT_LO.mean(), mcr.OUT_HI.mean())
    c.close()
    sl.anchor_assert("device, plan 0 scale %.1f, %d x %d flights" % (scale, R, S), f)
