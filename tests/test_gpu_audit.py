"""The segment audit (scvx_segment_audit_f64 / scvx_batch_segment_audit), the back-offs taken from it (scvx_batch_audit_margins) and the
hardening loop (ScvxBatch.harden) on the MI355X against the independent CPU reference (tests/audit_reference.py: the sample states of
flight_reference.chain in PLAN mode, the back-off rule in numpy, the oracle's own runs in tests/golden/oracle_audit_runs.npz).

Bounds, none of them taken from the device:
  * seg and the reduced report against the reference: the bound test_gpu_flight.py applies to PLAN-mode reports (its _compare): the
    state-valued columns (DEFECT, QNORM; GAP, MISS_*, MASS_END) within 1e-12, the G_* within 1e-12 * flight_reference.g_lipschitz;
  * the back-off kernel against the numpy rule on the same launch's seg: 1 ulp (the kernel may contract old + gain e);
  * the run from the straight-line guess under the fixture's round-1 back-offs: the bounds of test_gpu_margins.py's complete run
    (the oracle's accept / reject sequence, defect < 1e-5, final mass, r and v within 1e-4 of the oracle's);
  * hardening from the guess: every selected G <= 1e-7 within 4 rounds (the oracle needs 3 and 1).
Every comparison prints its figures before it asserts.
"""
import ctypes as C
import os

import numpy as np
import pytest

import audit_reference as ar
import flight_reference as fr
import horizon_cases as hc
from conftest import GOLDEN, random_segments
from test_gpu_flight import _compare, _flyable

pytestmark = pytest.mark.gpu

TOL = 1e-7
_STATE_SEG = ("DEFECT", "QNORM")


def _compare_seg(tag, dev, ref, bound, po):
    """device seg vs reference seg [B][K][11] with test_gpu_flight._compare's rule: state-valued columns within `bound`, G_* within
    bound * the Lipschitz factor, -inf where the reference has it"""
    L = fr.g_lipschitz(po)
    worst_s = worst_g = 0.0
    for n in ar.COLUMNS:
        d, r = dev[..., ar.IDX[n]], ref[..., ar.IDX[n]]
        inf = np.isneginf(r)
        assert np.array_equal(inf, np.isneginf(d)), (tag, n)
        e = float(np.abs(d[~inf] - r[~inf]).max()) if (~inf).any() else 0.0
        if n in _STATE_SEG:
            worst_s = max(worst_s, e)
        else:
            worst_g = max(worst_g, e)
    print("%s: state columns %.3e (bound %.3e), G columns %.3e (bound %.3e)" % (tag, worst_s, bound, worst_g, bound * L))
    assert worst_s <= bound, (tag, worst_s, bound)
    assert worst_g <= bound * L, (tag, worst_g, bound * L)


def _check_launch(tag, c, po, dyn, par, x, u, s, nsub, ref=None):
    from successiveconvexification_amd.dynamics import flight_check_batch, segment_audit_batch
    rep = segment_audit_batch(c, x, u, s, nsub=nsub)
    B, K = x.shape[0], x.shape[1] - 1
    assert rep.seg.shape == (B, K, 11) and rep.flight.raw.shape == (B, 16)
    seg_ref, rep_ref = ref if ref is not None else ar.audit(dyn, po, x, u, s, nsub, par)
    _compare_seg(tag + " seg", rep.seg, seg_ref, 1e-12, po)
    # the reduced report: bitwise the maximum of the same launch's seg, and the PLAN-mode flight check within the same bound
    for name, col in ar.report_from_seg(rep.seg).items():
        assert np.array_equal(getattr(rep.flight, name), col), (tag, name)
    _compare(tag + " report vs reference", rep.flight.raw, rep_ref, 1e-12, po)
    _compare(tag + " report vs flight check", rep.flight.raw, flight_check_batch(c, x, u, s, nsub=nsub, mode="plan").raw, 1e-12, po)
    # two launches agree bit for bit
    again = segment_audit_batch(c, x, u, s, nsub=nsub)
    assert np.array_equal(again.seg, rep.seg) and np.array_equal(again.flight.raw, rep.flight.raw)
    return rep


@pytest.mark.parametrize("nsub", [1, 10, 40])
@pytest.mark.parametrize("model,K", [("exo", 3), ("aero+fins", 3), ("aero+fins+torque", 3), ("exo", 1), ("aero+fins", 1)])
def test_kernel_parity_short_horizons(model, K, nsub, aero_tables):
    _parity_case(model, K, nsub, aero_tables)


@pytest.mark.parametrize("model", ["aero", "aero+torque"])
def test_kernel_parity_of_the_other_instantiations(model, aero_tables):
    """the two instantiations the cases above do not reach (aerodynamics without fins, with and without the body torque)"""
    _parity_case(model, 3, 10, aero_tables)


def _parity_case(model, K, nsub, aero_tables):
    from successiveconvexification_amd.dynamics import IntegratorCache
    pp, po, dyn, par, x, u, s = hc.case(model, K, aero_tables)
    c = IntegratorCache(pp, npts=10)
    rep = _check_launch("%s K %d nsub %d" % (model, K, nsub), c, po, dyn, par, x, u, s, nsub)
    assert np.all(np.isneginf(rep.G_DP)) and np.all(np.isneginf(rep.G_FIN)) == ("fins" not in model)
    val, k = rep.worst("G_TMIN")
    assert np.array_equal(val, rep.G_TMIN.max(axis=1)) and np.array_equal(rep.G_TMIN[np.arange(len(rep)), k], val)
    c.close()


@pytest.mark.parametrize("B", [1, 65])
def test_kernel_parity_across_wavefronts_and_plans(B):
    """B = 65 at K = 3: 195 segments, four wavefronts, plans that straddle them; B = 1: one partly filled wavefront; with the dynamic
    pressure cone enforced"""
    from dataclasses import replace
    from oracle import dynamics as od
    from successiveconvexification_amd.dynamics import IntegratorCache
    pp, po = _flyable()
    vm = 0.9 * float(np.linalg.norm(po.vIi))
    pp = replace(pp, K=3, dpMax=0.5 * po.rho * vm**2, model_flags=pp.model_flags | 1)
    po = replace(po, K=3, enforce_dp=True, dpMax=0.5 * po.rho * vm**2)
    x, u, s = random_segments(po, B, 3, 20261021 + B)
    c = IntegratorCache(pp, npts=10)
    rep = _check_launch("B %d" % B, c, po, od, od.Params(po), x, u, s, 10)
    assert np.isfinite(rep.G_DP).all()
    c.close()


def test_kernel_parity_on_the_golden_plans():
    """K = 50: the oracle's converged plans, against the fixture's audit (nsub 10) and the reference at nsub 40; what the audit shows"""
    from oracle import dynamics as od
    from successiveconvexification_amd import montecarlo as mc
    from successiveconvexification_amd.dynamics import IntegratorCache
    g = np.load(os.path.join(GOLDEN, "oracle_flight_runs.npz"))
    a = np.load(os.path.join(GOLDEN, "oracle_audit_runs.npz"))
    pp, po = _flyable()
    x, u, s = g["x"], g["u"], g["sigma"]
    c = IntegratorCache(pp, npts=10)
    base = np.stack([a["seg_0"], a["seg_1"]])
    rep = _check_launch("golden nsub 10", c, po, od, None, x, u, s, 10, ref=(base, g["report_plan"]))
    _check_launch("golden nsub 40", c, po, od, od.Params(po), x, u, s, 40)
    summ = mc.audit_summary(rep, np.zeros(2, np.int32), TOL)
    print("golden plans on the device: G_TMIN > tol in %s segments (largest %s), G_TILT in %s (largest %s); summary %s"
          % ((rep.G_TMIN > TOL).sum(axis=1), rep.G_TMIN.max(axis=1), (rep.G_TILT > TOL).sum(axis=1), rep.G_TILT.max(axis=1), summ["stats"]))
    assert (rep.G_TMIN > TOL).sum(axis=1).tolist() == [4, 9] and (rep.G_TILT > TOL).sum(axis=1).tolist() == [3, 3]
    assert summ["stats"]["G_TMIN"]["plans"] == 1.0 and summ["stats"]["G_TMIN"]["segments"] == 13 / 100 and summ["stats"]["G_MASS"]["plans"] == 0.0
    c.close()


def test_a_nan_node_is_contained_in_its_segment(aero_tables):
    from successiveconvexification_amd.dynamics import IntegratorCache, segment_audit_batch
    pp, po, dyn, par, x, u, s = hc.case("exo", 3, aero_tables)
    c = IntegratorCache(pp, npts=10)
    clean = segment_audit_batch(c, x, u, s)
    xb = x.copy()
    xb[1, 2, 4] = np.nan       # node 2 of plan 1: the start of segment 2, and the node the end of segment 1 is compared with
    bad = segment_audit_batch(c, xb, u, s)
    state = [ar.IDX[n] for n in ("DEFECT", "G_MASS", "G_GLIDE", "G_TILT", "G_RATE", "QNORM")]
    ctrl = [ar.IDX[n] for n in ("G_TMAX", "G_TMIN", "G_GIMBAL", "G_DP", "G_FIN")]
    assert np.isnan(bad.seg[1, 2, state]).all() and np.array_equal(bad.seg[1, 2, ctrl], clean.seg[1, 2, ctrl])
    assert np.isnan(bad.seg[1, 1, ar.IDX["DEFECT"]]) and np.array_equal(bad.seg[1, 1, 1:], clean.seg[1, 1, 1:])
    keep = np.ones((3, 3), bool)
    keep[1, 1:] = False
    assert np.array_equal(bad.seg[keep], clean.seg[keep])
    assert np.array_equal(bad.flight.raw[[0, 2]], clean.flight.raw[[0, 2]])
    for n in ("GAP", "MISS_R", "MISS_V", "MISS_Q", "MISS_W", "G_MASS", "G_GLIDE", "G_TILT", "G_RATE", "QNORM"):
        assert np.isnan(getattr(bad.flight, n)[1]), n
    for n in ("G_TMAX", "G_TMIN", "G_GIMBAL"):
        assert getattr(bad.flight, n)[1] == getattr(clean.flight, n)[1], n
    c.close()


def _golden_batch(c, f32=False):
    from successiveconvexification_amd.batch import ScvxBatch
    g = np.load(os.path.join(GOLDEN, "oracle_flight_runs.npz"))
    b = ScvxBatch(c, 2).set_linearization_f32(f32).init(g["ic"])
    b.set_trajectory(g["x"], g["u"], g["sigma"])
    return b, g


def test_host_device_and_batch_forms_agree_bit_for_bit():
    import torch
    from successiveconvexification_amd.dynamics import IntegratorCache, segment_audit_batch
    pp, po = _flyable()
    c = IntegratorCache(pp, npts=10)
    for f32 in (False, True):
        b, g = _golden_batch(c, f32)
        before = (b.trajectory_record(),) + b.scalars() + b.flags() + b.thrust_margins() + (b.path_margins(),)
        host = segment_audit_batch(c, g["x"], g["u"], g["sigma"])
        bat = b.audit()
        after = (b.trajectory_record(),) + b.scalars() + b.flags() + b.thrust_margins() + (b.path_margins(),)
        for a0, a1 in zip(before, after):
            assert np.array_equal(a0, a1, equal_nan=True)
        assert np.array_equal(bat.seg, host.seg) and np.array_equal(bat.flight.raw, host.flight.raw)
        assert np.array_equal(b.audit(nsub=40).seg, segment_audit_batch(c, g["x"], g["u"], g["sigma"], nsub=40).seg)
        b.close()
    up = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")   # noqa: E731
    ins = [up(g[k]) for k in ("x", "u", "sigma")]
    seg, rep = torch.zeros((2, 50, 11), dtype=torch.float64, device="cuda"), torch.zeros((2, 16), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    assert c._L.scvx_segment_audit_f64(c.handle, 2, 50, *[ptr(t) for t in ins], 0, ptr(seg), ptr(rep)) == 0, c._L.scvx_last_error(c.handle)
    c.synchronize()
    assert np.array_equal(seg.cpu().numpy(), host.seg) and np.array_equal(rep.cpu().numpy(), host.flight.raw)
    seg.zero_()
    torch.cuda.synchronize()
    assert c._L.scvx_segment_audit_f64(c.handle, 2, 50, *[ptr(t) for t in ins], 10, ptr(seg), None) == 0   # without the report
    c.synchronize()
    assert np.array_equal(seg.cpu().numpy(), host.seg)
    c.close()


def _rule(po, b, seg, lo, pm, kinds, gain, tol, cap):
    x = b.trajectory()[0]
    out = [ar.backoff_rule(po, x[t], seg[t], lo[t], pm[t], kinds, gain, tol, cap) for t in range(b.B)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def _ulp_close(tag, dev, ref):
    d = np.abs(dev - ref)
    print("%s: largest difference %.3e, in ulps of the reference %.2f" % (tag, d.max(), float((d / np.spacing(np.maximum(np.abs(ref), 1e-300))).max())))
    assert np.all(d <= np.spacing(np.abs(ref))), tag


def test_backoffs_equal_the_numpy_rule_on_the_same_seg():
    """on a batch that carries none, on one that carries robustify-style back-offs (accumulation), across the caps and the forced zeros;
    a constraint that is not selected keeps its buffer bit for bit"""
    from successiveconvexification_amd.dynamics import IntegratorCache
    pp, po = _flyable()
    K = pp.K
    c = IntegratorCache(pp, npts=10)
    # -- none carried; thrust + tilt at the defaults: nothing reaches a cap
    b, g = _golden_batch(c)
    seg = b.margins_from_audit(("thrust", "tilt"), gain=1.5, tol=TOL, cap=0.25)
    assert np.array_equal(seg, b.audit().seg)
    lo, hi = b.thrust_margins()
    pm = b.path_margins()
    rlo, rpm = _rule(po, b, seg, np.zeros((2, K + 1)), np.zeros((2, K + 1, 4)), ("thrust", "tilt"), 1.5, TOL, 0.25)
    _ulp_close("none carried: lo", lo, rlo), _ulp_close("none carried: pm", pm, rpm)
    assert not hi.any() and (lo > 0).sum(axis=1).tolist() == [(ar.excess(seg[t, :, ar.IDX["G_TMIN"]], TOL) > 0).sum() for t in range(2)]
    assert (lo > 0).any() and (pm[..., 2] > 0).any() and not pm[..., [0, 1, 3]].any()
    # -- accumulation on what is there, all four kinds, a gain that drives entries into the cap (cap 1e-3 of the widths)
    seg2 = b.margins_from_audit(("thrust", "glide", "tilt", "rate"), gain=1e3, tol=0.0, cap=1e-3)
    assert np.array_equal(seg2, seg)                       # the iterate did not move: the audit is against the true constants
    lo2, hi2 = b.thrust_margins()
    pm2 = b.path_margins()
    rlo2, rpm2 = _rule(po, b, seg, lo, pm, ("thrust", "glide", "tilt", "rate"), 1e3, 0.0, 1e-3)
    _ulp_close("accumulated: lo", lo2, rlo2), _ulp_close("accumulated: pm", pm2, rpm2)
    assert not hi2.any() and (lo2 == 1e-3 * (pp.Tmax - pp.Tmin)).any()
    for t in range(2):
        ar.pr.check_contract(po, rpm2[t]), ar.pr.check_contract(po, pm2[t])
    assert not pm2[:, K, 1:].any() and not pm2[:, 0, [1, 3]].any() and not pm2[..., 0].any()
    b.close()
    # -- robustify-style back-offs carried: lo = hi and tilt from a covariance; only tilt selected: the thrust buffer is untouched
    b, g = _golden_batch(c)
    S0 = np.ascontiguousarray(np.broadcast_to(1e-6 * np.eye(14), (2, 14, 14)))
    b.margins_from_cov(S0, constraints=("thrust", "tilt", "rate"))
    lo0, hi0 = b.thrust_margins()
    pm0 = b.path_margins()
    assert lo0.any() and pm0[..., 2].any()
    seg = b.margins_from_audit(("tilt",), gain=2.0, tol=TOL, cap=0.25)
    lo1, hi1 = b.thrust_margins()
    pm1 = b.path_margins()
    assert np.array_equal(lo1, lo0) and np.array_equal(hi1, hi0) and np.array_equal(pm1[..., [0, 1, 3]], pm0[..., [0, 1, 3]])
    _, rpm = _rule(po, b, seg, lo0, pm0, ("tilt",), 2.0, TOL, 0.25)
    _ulp_close("carried: tilt", pm1[..., 2], rpm[..., 2])
    assert (pm1[..., 2] > pm0[..., 2]).any() and (pm1[..., 2] >= pm0[..., 2]).all()
    # thrust alone: hi and the path buffer are untouched
    b.margins_from_audit(("thrust",), gain=2.0, tol=TOL, cap=0.25, want_seg=False)
    lo2, hi2 = b.thrust_margins()
    rlo, _ = _rule(po, b, seg, lo1, pm1, ("thrust",), 2.0, TOL, 0.25)
    assert np.array_equal(hi2, hi0) and np.array_equal(b.path_margins(), pm1)
    _ulp_close("carried: lo", lo2, rlo)
    assert np.all(lo2 + hi2 < pp.Tmax - pp.Tmin)
    b.close(), c.close()


def test_a_nan_plan_keeps_its_backoffs_and_refusals_answer_with_their_word():
    from successiveconvexification_amd import _lib
    from successiveconvexification_amd.dynamics import IntegratorCache
    pp, po = _flyable()
    c = IntegratorCache(pp, npts=10)
    b, g = _golden_batch(c)
    x = g["x"].copy()
    x[1, 20, 9] = np.nan
    b.set_trajectory(x, g["u"], g["sigma"])
    b.set_path_margins(tilt=1e-4)
    pm0 = b.path_margins()
    b.margins_from_audit(("thrust", "tilt"))
    lo, _ = b.thrust_margins()
    pm = b.path_margins()
    assert np.array_equal(pm[1], pm0[1]) and not lo[1].any()            # the NaN plan: as it was
    assert (pm[0, :, 2] > pm0[0, :, 2]).any() and lo[0].any()           # its neighbour: served
    L, h = c._L, c.handle
    cases = [(dict(gain=0.5), "gain"), (dict(gain=np.nan), "gain"), (dict(gain=np.inf), "gain"), (dict(tol=-1e-9), "tol"),
             (dict(tol=np.nan), "tol"), (dict(cap=0.0), "cap"), (dict(cap=0.5), "cap"), (dict(cap=np.nan), "cap"), (dict(which=0), "which"),
             (dict(which=32), "which"), (dict(which=2), "mass"), (dict(which=3), "mass"), (dict(nsub=-1), "nsub"), (dict(nsub=1001), "nsub")]
    before = b.thrust_margins() + (b.path_margins(),)
    for kw, word in cases:
        a = dict(nsub=0, which=9, gain=1.5, tol=1e-7, cap=0.25)
        a.update(kw)
        assert L.scvx_batch_audit_margins(b.handle, a["nsub"], a["which"], a["gain"], a["tol"], a["cap"], None) == -1, kw
        assert word in L.scvx_last_error(h).decode(), (kw, L.scvx_last_error(h))
    for a0, a1 in zip(before, b.thrust_margins() + (b.path_margins(),)):
        assert np.array_equal(a0, a1)
    seg, rep = np.zeros((2, 50, 11)), np.zeros((2, 16))
    p = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
    xs, us, ss = (np.ascontiguousarray(g[k]) for k in ("x", "u", "sigma"))
    args = lambda **kw: [kw.get("B", 2), kw.get("K", 50), kw.get("x", p(xs)), kw.get("u", p(us)), kw.get("s", p(ss)), kw.get("nsub", 10),  # noqa: E731
                         kw.get("seg", p(seg)), p(rep)]
    for kw, word in [(dict(nsub=-3), "nsub"), (dict(nsub=1001), "nsub"), (dict(B=0), "B >= 1"), (dict(K=49), "K must equal"),
                     (dict(x=None), "null"), (dict(u=None), "null"), (dict(s=None), "null"), (dict(seg=None), "null")]:
        for fn in (L.scvx_segment_audit_f64_host, L.scvx_segment_audit_f64):
            a = args(**kw)
            if fn is L.scvx_segment_audit_f64:   # device form: the checks come before any pointer is used
                a = a[:2] + [C.c_void_p(1) if v is not None else None for v in a[2:5]] + [a[5]] + [C.c_void_p(1) if a[6] is not None else None, None]
            assert fn(h, *a) == -1, (kw, fn)
            assert word in L.scvx_last_error(h).decode(), (kw, L.scvx_last_error(h))
    assert L.scvx_batch_segment_audit(b.handle, -1, p(seg), None) == -1 and "nsub" in L.scvx_last_error(h).decode()
    assert L.scvx_batch_segment_audit(b.handle, 0, None, None) == -1 and "null" in L.scvx_last_error(h).decode()
    with pytest.raises(ValueError, match="mass"):
        b.margins_from_audit(("mass",))
    with pytest.raises(ValueError):
        b.harden(restart="again")
    with pytest.raises(_lib.ScvxError, match="gain"):
        b.margins_from_audit(gain=0.0)
    b.close(), c.close()


def _sequence(b, pp):
    """the accept / reject sequence of a solve from the batch's state, stepped one solve_step at a time"""
    seq = [[] for _ in range(b.B)]
    done = np.zeros(b.B, bool)
    for _ in range(pp.imax - 1):
        s1 = b.solve_step()[0]
        for t in range(b.B):
            if not done[t]:
                seq[t].append(0 if s1[t] == 2 else 1)
                done[t] = s1[t] not in (1, 2)
        if done.all():
            break
    return seq


def test_from_the_guess_under_the_fixture_backoffs_against_the_oracle():
    """plan 0, the fixture's round-1 back-offs set directly, reset() + solve(): the oracle's accept / reject sequence, the bounds of
    test_gpu_margins.py's complete run, and G_TMIN <= tol in its audit"""
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache, propagate_batch
    a = np.load(os.path.join(GOLDEN, "oracle_audit_runs.npz"))
    g = np.load(os.path.join(GOLDEN, "oracle_flight_runs.npz"))
    pp, po = _flyable()
    K = pp.K
    c = IntegratorCache(pp, npts=10)
    lo, pm = a["r0_0_lo"][None], a["r0_0_pm"][None]
    b = ScvxBatch(c, 1).init(g["ic"][:1]).set_thrust_margins(lo, np.zeros_like(lo))
    b._chk(b._L.scvx_batch_set_path_margins(b.handle, np.ascontiguousarray(pm).ctypes.data_as(C.POINTER(C.c_double))), "scvx_batch_set_path_margins")
    st, it, nu, dj = b.reset().solve()
    x, u, s = b.trajectory()
    twin = ScvxBatch(c, 1).init(g["ic"][:1]).set_thrust_margins(lo, np.zeros_like(lo))
    twin._chk(twin._L.scvx_batch_set_path_margins(twin.handle, np.ascontiguousarray(pm).ctypes.data_as(C.POINTER(C.c_double))), "scvx_batch_set_path_margins")
    seq = _sequence(twin, pp)
    want = [int(v) for v in a["r0_0_accepted"]]
    gx = a["r0_0_x"][None]
    defect = float(np.abs(propagate_batch(c, x, u, s, 1.0 / (K + 1)) - x[:, 1:]).max())
    rep = b.audit()
    print("status %s iters %s; sequence %s (oracle %s); defect %.3e; device-vs-oracle mass %.2e r %.2e v %.2e; G_TMIN %.3e G_TILT %.3e (oracle %.3e %.3e)"
          % (st, it, seq[0], want, defect, abs(x[0, -1, 0] - gx[0, -1, 0]), np.abs(x[..., 1:4] - gx[..., 1:4]).max(),
             np.abs(x[..., 4:7] - gx[..., 4:7]).max(), rep.G_TMIN.max(), rep.G_TILT.max(), a["r0_0_seg"][:, ar.IDX["G_TMIN"]].max(),
             a["r0_0_seg"][:, ar.IDX["G_TILT"]].max()))
    assert st[0] == 0 and seq[0] == want and int(it[0]) == len(want)
    assert defect < 1e-5
    assert abs(x[0, -1, 0] - gx[0, -1, 0]) < 1e-4
    assert np.abs(x[..., 1:4] - gx[..., 1:4]).max() < 1e-4 and np.abs(x[..., 4:7] - gx[..., 4:7]).max() < 1e-4
    assert rep.G_TMIN.max() <= TOL
    b.close(), twin.close(), c.close()


def test_harden_from_the_guess_and_by_replanning():
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache
    g = np.load(os.path.join(GOLDEN, "oracle_flight_runs.npz"))
    pp, po = _flyable()
    c = IntegratorCache(pp, npts=10)
    kinds = ("thrust", "tilt")
    cols = ("G_TMIN", "G_TILT")
    worst = lambda rep: np.max([getattr(rep, n).max(axis=1) for n in cols], axis=0)   # noqa: E731

    def start():
        b = ScvxBatch(c, 2).init(g["ic"])
        st = b.solve()[0]
        assert np.all(st == 0), st
        return b
    # -- from the guess: at most 4 rounds is a condition (the oracle needs 3 and 1)
    b = start()
    base = b.audit()
    m0 = b.trajectory()[0][:, -1, 0]
    st, it, nu, dj, rep, used = b.harden(kinds, rounds=4, restart="guess")
    print("harden from the guess: %d rounds, status %s iters %s, worst selected G %s -> %s, final mass %s -> %s"
          % (used, st, it, worst(base), worst(rep), m0, b.trajectory()[0][:, -1, 0]))
    assert np.all(worst(base) > 1e-4)
    assert np.all(st == 0) and 1 <= used <= 4
    assert np.all(worst(rep) <= TOL)
    assert np.array_equal(rep.seg, b.audit().seg)
    b.close()
    # -- by replanning: round for round the manual sequence, bit for bit
    h, m = start(), start()
    back = lambda bb: bb.thrust_margins() + (bb.path_margins(),)   # noqa: E731
    rounds = 0
    for r in range(3):
        if not (worst(m.audit()) > TOL).any():
            break
        m.margins_from_audit(kinds, want_seg=False)
        m.replan()
        sm = m.solve()
        out = h.harden(kinds, rounds=1, restart="replan")
        rounds += 1
        assert out[5] == 1
        for a0, a1 in zip(back(h), back(m)):
            assert np.array_equal(a0, a1), r
        assert np.array_equal(h.trajectory_record(), m.trajectory_record()) and np.array_equal(out[0], sm[0])
    w = start()
    st, it, nu, dj, rep, used = w.harden(kinds, rounds=rounds, restart="replan")
    for a0, a1 in zip(back(w), back(m)):
        assert np.array_equal(a0, a1)
    print("harden by replanning: %d rounds, status %s iters %s, worst selected G %s -> %s, final mass %s -> %s"
          % (used, st, it, worst(base), worst(rep), m0, w.trajectory()[0][:, -1, 0]))
    assert used == rounds and np.all(st == 0)
    assert np.all(worst(rep) < worst(base))
    h.close(), m.close(), w.close(), c.close()
