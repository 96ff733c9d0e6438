"""Per-flight vehicle errors of the sampled closed-loop dispersion (the _veh forms), without a GPU: the CPU reference chain
(tests/mc_vehicle_reference.py) against mc_reference.chain at theta = 0, the numpy twin of the device's stream 8 against numpy's own
Philox words, the three bindings of the new symbols, the host helpers, and the statistical anchors through the C oracle.

Bounds, none of them taken from the code under test:
  * theta = 0: equality with mc_reference.chain.
  * words: equality with np.random.Philox(...).random_raw.
  * anchors: six standard errors per entry (mc_reference.se_check) of Sigma_K + J diag(sp^2) J', Sigma_K the first-order recursion from
    the handover of test_mc_cpu.w_case alone, J by central differences (step 2^-10) through the same chain, sp the value at which
    J diag(sp^2) J' has the trace of Sigma_K; the twin's draws, seed 0.  Recorded on the CPU reference: control-side components
    (THRUST, MIS_Y, MIS_Z; 8,192 flights) sp 8.719e-05, worst entry 1.89 standard errors (147 entries over 6 against Sigma_K alone);
    ISP (2,048 flights, one oracle parameter set per flight) sp 2.413e-03, worst 1.61 (95 entries over 6 against Sigma_K alone).
    AERO has no converged plan without a device, and on the aerodynamic plans at hand |dx_K/dAERO| is so small that the sp matching
    w_case's handover would be far above 1; so its sp is set to a plausible 0.1 and the HANDOVER is scaled down to the same share
    instead (aero_anchor_case; se_check is relative).  Recorded: K = 3, 8,192 flights, one oracle parameter set per flight,
    |dx_K/dAERO| 5.97e-07, trace of Sigma_K 3.56e-15, worst 2.87 (93 entries over 6 against Sigma_K alone)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cov_reference as cr
import mc_reference as mr
import mc_rng_reference as rr
import mc_vehicle_reference as vr
import track_reference as tr
from conftest import ROOT
from test_mc_rng_cpu import LOS, SEEDS

H_FD = 2.0 ** -10
ISP_SAMPLES = 2048    # one oracle parameter set per flight: about half a minute
AERO_K, AERO_SP, AERO_SAMPLES = 3, 0.1, 8192    # a short horizon: one oracle parameter set per flight here too


def test_reference_chain_at_theta_zero_is_the_plain_chain_bit_for_bit():
    from oracle import dynamics as od
    import track_reference as tr
    from test_cov_cpu import _data
    p, par, x, u, s, d = _data()
    L, _ = tr.gains(d, p.K)
    dx0 = np.zeros((2, 14))
    dx0[:, 1:7] = 1e-3
    imp = np.zeros((2, p.K, 14))
    imp[:, 9, 4] = 1e-4
    for flags in (0, tr.CLAMP):
        ref = mr.chain(od, par, p, x, u, s, L, dx0, 2, flags, imp)
        mine = vr.chain(od, par, p, x, u, s, L, dx0, 2, np.zeros((2, 6)), flags, imp)
        for a0, a1 in zip(ref, mine):
            assert np.array_equal(a0, a1)
    # the applied control: scale, first-order rotation about body y and z, fins
    uu = np.array([[0.8, 0.1, -0.2, 0.03, -0.04]])
    th = np.array([[0.01, 2e-3, -3e-3, 0.5, 0.5, -0.1]])
    ua = vr.apply(uu, th)[0]
    dxu = np.cross([0.0, 2e-3, -3e-3], uu[0, :3])
    assert np.allclose(ua[:3], 1.01 * (uu[0, :3] + dxu), rtol=1e-15) and np.allclose(ua[3:], 0.9 * uu[0, 3:], rtol=1e-15)
    # ISP and AERO reach the integrator through its own constructor
    q = vr.scaled_params(od, p, par, 0.25, 0.0)
    assert q is not par and q.c.alpha == p.alpha * 1.25 and vr.scaled_params(od, p, par, 0.0, 0.0) is par
    with pytest.raises(ValueError):
        vr.scaled_params(od, p, par, 0.0, 0.1)                        # the golden plans are exo-atmospheric
    with pytest.raises(ValueError):
        vr.chain(od, par, p, x, u, s, L, dx0, 2, np.array([[0, 0, 0, 0, 0, 0.1]] * 2))
    # a vehicle error moves the landing and leaves the commanded node 1 alone; the mass flow sees the applied thrust and alpha
    th = np.zeros((2, 6))
    th[0, vr.THRUST], th[1, vr.ISP] = 1e-2, 1e-2
    S1, US1, xf1, uf1, cmd1 = vr.chain(od, par, p, x, u, s, L, dx0, 2, th)
    S0_, US0, xf0, uf0, cmd0 = mr.chain(od, par, p, x, u, s, L, dx0, 2)
    assert np.array_equal(uf1[:, :2], uf0[:, :2]) and np.array_equal(cmd1[:, 0], cmd0[:, 0]) and not np.array_equal(xf1[:, -1], xf0[:, -1])
    dm1, dm0 = xf1[:, 1, 0] - xf1[:, 0, 0], xf0[:, 1, 0] - xf0[:, 0, 0]
    assert np.allclose(dm1 / dm0, 1.01, rtol=1e-4)


@pytest.mark.parametrize("seed", SEEDS)
def test_stream_8_words_are_numpys_philox_words(seed):
    from successiveconvexification_amd.montecarlo import MC_STREAM_VEH, mc_vehicle_draws_device, philox4x64_blocks
    assert MC_STREAM_VEH == 8
    j = 1 + np.arange(2, dtype=np.uint64)                   # the two blocks that hold the six normals
    for lo in LOS:
        for c2 in (0, 1, 3, 1 + 2 ** 40):                   # shared; independent plans 0, 2 and 2^40
            for s in (0, 1, 65):
                mine = philox4x64_blocks(seed, j, 8, c2, lo + s)
                assert mine.dtype == np.uint64 and np.array_equal(mine, rr.words(seed, 8, c2, lo + s, 2)), (seed, lo, c2, s)
    # the twin's normals sit on these words: the longdouble reference of the device's Box-Muller, 8 ulp (test_mc_rng_cpu.py's bound)
    for lo in LOS:
        for plans in (None, (0, 2)):
            z = mc_vehicle_draws_device(5, seed, lo=lo, plans=plans)
            assert z.shape == ((5, 6) if plans is None else (2, 5, 6))
            for i, c2 in enumerate([0] if plans is None else [1, 3]):
                for s in range(5):
                    ref = rr.normals(rr.words(seed, 8, c2, lo + s, 2)).reshape(-1)[:6]
                    got = (z if plans is None else z[i])[s]
                    assert rr.ulp_distance(got, ref).max() <= 8.0
    # a shard is the rows of the whole
    assert np.array_equal(mc_vehicle_draws_device(66, seed, lo=64), mc_vehicle_draws_device(130, seed)[64:])


def test_header_binding_and_julia_carry_the_six_symbols():
    from successiveconvexification_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "scvx.h")).read()
    jl = open(os.path.join(ROOT, "julia", "ScvxAMD.jl")).read()
    S = _lib.SIGNATURES
    ext = {"scvx_track_mc_veh_f64": "scvx_track_mc_q_f64", "scvx_track_mc_veh_f64_host": "scvx_track_mc_q_f64_host",
           "scvx_track_mc_nav_veh_f64": "scvx_track_mc_nav_q_f64", "scvx_track_mc_nav_veh_f64_host": "scvx_track_mc_nav_q_f64_host",
           "scvx_batch_track_mc_veh": "scvx_batch_track_mc_q", "scvx_batch_track_mc_nav_veh": "scvx_batch_track_mc_nav_q"}
    for sym, old in ext.items():
        n = len(S[old][1]) + 5
        m = re.search(r"\bint %s\(([^;]*?)\);" % sym, hdr, flags=re.S)
        mo = re.search(r"\bint %s\(([^;]*?)\);" % old, hdr, flags=re.S)
        assert m and mo, sym
        args = [" ".join(a.split()) for a in m.group(1).split(",")]
        assert len(args) == n == len(S[sym][1]), sym
        # the argument list of the _q form, verbatim, then the five
        assert args[:-5] == [" ".join(a.split()) for a in mo.group(1).split(",")], sym
        assert [a.split("*")[0].strip() if "*" in a else a.split()[0] for a in args[-5:]] == \
            ["const scvx_mc_rng", "int", "const scvx_mc_vehicle", "const double", "double"], sym
        assert list(S[sym][1][:-5]) == list(S[old][1]) and S[sym][1][-5] is _lib._rp and S[sym][1][-4] is C.c_int
        assert S[sym][1][-3]._type_ is _lib.ScvxMcVehicle
        j = re.search(r"ccall\(\(:%s, LIB\), Cint,\s*\(([^)]*)\)" % sym, jl, flags=re.S)
        assert j, sym
        assert len([a for a in j.group(1).split(",") if a.strip()]) == n, sym
    assert C.sizeof(_lib.ScvxMcVehicle) == 104
    assert re.search(r"double mu\[SCVX_VEH_N\], sp\[SCVX_VEH_N\];\s*int32_t reserved\[2\];", hdr)
    assert int(re.search(r"#define SCVX_VEH_N (\d+)", hdr).group(1)) == 6 == _lib.VEH_N
    for i, name in enumerate(_lib.VEH_COLUMNS):
        assert int(re.search(r"#define SCVX_VEH_%s (\d+)" % name, hdr).group(1)) == i == _lib.VEH_INDEX[name]
    assert int(re.search(r"#define SCVX_ABI_VERSION (\d+)", hdr).group(1)) == 4 == _lib.ABI_VERSION
    assert "struct McVehicle" in jl and jl.index("function track_mc_veh(b::Batch") < jl.index("function install!")


def test_host_helpers_and_keyword_checks_before_any_library_call():
    from successiveconvexification_amd import montecarlo as mc
    from successiveconvexification_amd.dynamics import _McVeh, _mc_rng
    mu, sp = mc.vehicle_errors(thrust=1e-3, misalign=(1e-3, 2e-3), isp=3e-3, aero=4e-3, fin=5e-3)
    assert not mu.any() and sp.tolist() == [1e-3, 1e-3, 2e-3, 3e-3, 4e-3, 5e-3]
    mu, sp = mc.vehicle_errors(misalign=1e-3, mean=[1, 2, 3, 4, 5, 6])
    assert mu.tolist() == [1, 2, 3, 4, 5, 6] and sp.tolist() == [0, 1e-3, 1e-3, 0, 0, 0]
    with pytest.raises(ValueError):
        mc.vehicle_errors(mean=[0.0] * 5)
    z = mc.mc_vehicle_draws(130, 3)
    assert z.shape == (130, 6) and np.array_equal(mc.mc_vehicle_draws(66, 3, lo=64), z[64:]) and len(np.unique(z)) == z.size
    assert not np.isin(z, mc.mc_draws(130, 2, 3)[0]).any()
    # the budget: the rows add up to the diagonal of the first-order covariance
    rng = np.random.default_rng(0)
    J, cK = rng.standard_normal((14, 6)), np.diag(rng.uniform(1e-8, 1e-6, 14))
    spv = np.array([1e-3, 2e-3, 0.0, 1e-4, 0.0, 0.0])
    bud = mc.vehicle_budget(J, spv, cK)
    assert np.allclose(bud["cov"], cK + J @ np.diag(spv ** 2) @ J.T, rtol=1e-14, atol=0)
    assert np.allclose(bud["var"].sum(0), np.diag(bud["cov"]), rtol=1e-13) and abs(bud["share"].sum() - 1.0) < 1e-14
    assert bud["var"][2].max() == 0.0 and np.allclose(bud["sigma_r"][0], 1e-3 * np.linalg.norm(J[1:4, 0]), rtol=1e-14)
    with pytest.raises(ValueError):
        mc.vehicle_budget(J[:, :5], spv, cK)
    # the keyword: off by default, "theta" only with it, zeta and rng="device" exclude each other
    off = _McVeh(None, ("xland", "pathv"))
    assert not off.on and set(off.rest) == {"xland", "pathv"}
    with pytest.raises(ValueError):
        _McVeh(None, ("theta",))
    with pytest.raises(ValueError):
        _McVeh((np.zeros(5), np.zeros(6)), ())
    on = _McVeh(mc.vehicle_errors(thrust=1e-3), ("theta", "xland"))
    assert on.on and on.rest == ("xland",) and on.veh.sp[0] == 1e-3 and list(on.veh.reserved) == [0, 0]
    f = on.fields(3, 7, None, 5, 64)
    assert list(f) == ["veh", "zeta", "theta"] and f["veh"] is on.veh and f["zeta"] is on.zeta and f["theta"] is on.theta
    assert on.theta.shape == (3, 7, 6) and np.array_equal(on.zeta, mc.mc_vehicle_draws(7, 5, lo=64))
    dev = _McVeh((np.zeros(6), np.zeros(6), np.zeros((7, 6))), ())
    with pytest.raises(ValueError):
        dev.fields(3, 7, _mc_rng("device", None, False, 0, 0, 0), 0, 0)
    with pytest.raises(ValueError):
        _McVeh((np.zeros(6), np.zeros(6), np.zeros((8, 6))), ()).fields(3, 7, None, 0, 0)
    f = _McVeh(mc.vehicle_errors(isp=1e-3), ()).fields(3, 7, _mc_rng("device", None, False, 0, 0, 0), 0, 0)
    assert f["veh"] is not None and f["zeta"] is None and f["theta"] is None
    # (rng, noise) of the _veh tail, on the recorded call: NULL and 0 with host draws whatever w is, the stream and 1 with the device's
    from py_call_recorder import Recorder, make_cache, pattern
    from successiveconvexification_amd.dynamics import track_mc_batch
    rec = Recorder()
    plan = (pattern((2, 4, 14)), pattern((2, 4, 3)), pattern((2,)), pattern((2, 3, 3, 17)), np.full(14, 0.5), 7)
    track_mc_batch(make_cache(rec, 3, False), *plan, seed=5, w=0.25, vehicle=mc.vehicle_errors(thrust=1e-3), sample_lo=64)
    track_mc_batch(make_cache(rec, 3, False), *plan, w=0.25, vehicle=mc.vehicle_errors(isp=1e-3), rng="device")
    track_mc_batch(make_cache(rec, 3, False), *plan, vehicle=mc.vehicle_errors(isp=1e-3), rng="device")
    assert [ln.split("(")[0] for ln in rec.lines] == ["scvx_track_mc_veh_f64_host"] * 3
    assert ", rng=NULL, noise=0, veh=&ScvxMcVehicle{" in rec.lines[0] and ", zeta=<f8[7, 6] crc=" in rec.lines[0]
    assert ", rng=&ScvxMcRng{" in rec.lines[1] and ", noise=1, veh=&ScvxMcVehicle{" in rec.lines[1] and rec.lines[1].endswith("zeta=NULL, theta=NULL)")
    assert ", rng=&ScvxMcRng{" in rec.lines[2] and ", noise=0, veh=&ScvxMcVehicle{" in rec.lines[2]


def anchor_case():
    """The inputs of the statistical anchors, shared with tests/test_gpu_mc_vehicle.py: test_mc_cpu.w_case's plan 0, gains and handover,
    Sigma_K [14][14] of the recursion from S0 ALONE, and J [14][6] by central differences through the reference chain (the exo model:
    columns THRUST .. ISP).  (p, par, x, u, s, d, L, S0, Sigma_K, J)"""
    from oracle import dynamics as od
    from test_mc_cpu import w_case
    p, par, x, u, s, d, L, S0, _, _ = w_case()
    covK = cr.propagate(d[:1], p.K, L[:1], S0[None], None)[0, -1][:14, :14]
    J = vr.sensitivity_fd(od, p, x[0], u[0], s[0], L[0], 10, H_FD, (vr.THRUST, vr.MIS_Y, vr.MIS_Z, vr.ISP), par=par)
    return p, par, x, u, s, d, L, S0, covK, J


def aero_anchor_case(aero_tables):
    """The inputs of the AERO anchor, an aerodynamic plan made without a device: start, controls and sigma of plan 0 of the K = AERO_K
    aero + fins case of tests/horizon_cases.py, the states the C oracle's open-loop flight of those controls from that start (the
    case's own states are random segments, no trajectory: a closed loop leaves them by O(1), and the recursion over their tiles is then
    not the linearisation of what is flown); tiles of oracle.dynamics.linearize about that flight, reference gains, J by central
    differences through the reference chain, and the handover of cov_reference.handover_s0 scaled DOWN until Sigma_K of the recursion
    from it alone has the trace of J diag(sp^2) J' at sp[AERO] = AERO_SP -- both are linear in their source, and se_check is relative.
    Same tuple as anchor_case."""
    import flight_reference as fr
    import horizon_cases as hc
    pp, po, dyn, par, x, u, s = hc.case("aero+fins", AERO_K, aero_tables)
    x, u, s, dt = x[:1].copy(), u[:1], s[:1], 1.0 / (AERO_K + 1)
    for k in range(AERO_K):
        x[:, k + 1] = fr._substeps(dyn, par, x[:, k], u[:, k], u[:, k + 1], s, dt, 10)[0][:, -1]
    _, d = dyn.linearize(par, x, u, s, dt, 10)
    L, _ = tr.gains(d, AERO_K)
    J = vr.sensitivity_fd(dyn, po, x[0], u[0], s[0], L[0], 10, H_FD, (vr.AERO,), par=par)
    S0, _ = cr.handover_s0(x[0, 0])
    prop = lambda S: cr.propagate(d[:1], AERO_K, L[:1], S[None], None)[0, -1][:14, :14]   # noqa: E731
    S0 = S0 * (AERO_SP ** 2 * float(J[:, vr.AERO] @ J[:, vr.AERO]) / float(np.trace(prop(S0))))
    return po, par, x, u, s, d, L, S0, prop(S0), J


def _anchor(tag, comps, N, case=None):
    from oracle import dynamics as od
    from successiveconvexification_amd.montecarlo import handover_factor, mc_draws_device, mc_vehicle_draws_device, vehicle_budget
    p, par, x, u, s, d, L, S0, covK, J = case or anchor_case()
    sp = np.zeros(6)
    sp[list(comps)] = vr.equal_share_sp(J, comps, float(np.trace(covK)))
    print("%s: |dx_K/dtheta| %s, trace of Sigma_K from S0 alone %.3e, sp %.3e" % (tag, np.linalg.norm(J, axis=0), np.trace(covK), sp.max()))
    xi0, _ = mc_draws_device(N, p.K, 0)
    theta = mc_vehicle_draws_device(N, 0) * sp
    dx0 = xi0 @ handover_factor(S0).T
    _, xf, _, _ = vr.fly_plan(od, p, x[0], u[0], s[0], L[0], dx0, 10, theta, par=par)
    _, _, xcov = mr.reduce(np.zeros((N, 16)), xf[:, -1] - x[0, -1], 0, 0, p.K)
    full = vehicle_budget(J, sp, covK)["cov"]
    assert np.allclose(np.trace(full), 2.0 * np.trace(covK), rtol=1e-12)
    worst, over = mr.se_check(xcov, full, N)
    worst0, over0 = mr.se_check(xcov, covK, N)
    print("C oracle, plan 0, S = %d, device streams seed 0: worst entry of the landing covariance %.2f standard errors of Sigma_K + "
          "J diag(sp^2) J', %d over 6; against Sigma_K alone %.2f, %d over 6" % (N, worst, over, worst0, over0))
    assert over == 0, (worst, over)
    assert over0 > 0


def test_anchor_control_side_components_within_six_standard_errors():
    """8,192 flights of golden plan 0 through the C oracle, the handover of w_case, THRUST, MIS_Y and MIS_Z dispersed with the sp at
    which they contribute the trace of Sigma_K: every entry of the sample landing covariance within six standard errors of
    Sigma_K + J diag(sp^2) J', and the same flights miss Sigma_K alone."""
    from test_mc_cpu import W_SAMPLES
    _anchor("THRUST, MIS_Y, MIS_Z", (vr.THRUST, vr.MIS_Y, vr.MIS_Z), W_SAMPLES)


def test_anchor_isp_within_six_standard_errors():
    """The same with ISP alone: one oracle parameter set per flight, so fewer flights (ISP_SAMPLES); the bound stays six standard
    errors."""
    _anchor("ISP", (vr.ISP,), ISP_SAMPLES)


def test_anchor_aero_within_six_standard_errors(aero_tables):
    """AERO alone on an aerodynamic plan (aero_anchor_case): a 1 sigma of AERO_SP on force_scalar, one oracle parameter set per flight,
    AERO_SAMPLES flights, the handover scaled to the same share; the bound stays six standard errors, and the same flights miss
    Sigma_K alone."""
    _anchor("AERO", (vr.AERO,), AERO_SAMPLES, aero_anchor_case(aero_tables))
