"""Plan tracking without a GPU: the independent reference (tests/track_reference.py: the recursion of include/scvx.h in numpy, the
closed loop driven through the C oracle) against the properties that define an LQR and a closed loop, the three bindings (header,
_lib.SIGNATURES, julia/ScvxAMD.jl) against each other, and montecarlo.disperse_handover.

Data: the two plans the oracle converges on (tests/golden/oracle_flight_runs.npz), tiles from oracle.dynamics.linearize."""
import os
import re
from dataclasses import replace

import numpy as np
import pytest

import flight_reference as fr
import track_reference as tr
from conftest import GOLDEN, ROOT

WEIGHTS = [(1.0, 1.0, 100.0), (1.0, 1e-2, 1e4), (10.0, 1.0, 1e6)]
_DATA = {}


def _data():
    """(oracle problem, dyn Params, x, u, sigma, deriv) of the golden converged plans"""
    if not _DATA:
        from oracle import dynamics as od, model
        g = np.load(os.path.join(GOLDEN, "oracle_flight_runs.npz"))
        p = replace(model.base_prob_scaled(), mdry=0.55, nuTol=1e-6, delTol=1e-3, imax=40, tf_guess=8.0)
        par = od.Params(p)
        x, u, s = g["x"], g["u"], g["sigma"]
        _, d = od.linearize(par, x, u, s, 1.0 / (p.K + 1), 10)
        _DATA["v"] = (p, par, x, u, s, d)
    return _DATA["v"]


def _handover(x, seed, size=1e-3):
    from successiveconvexification_amd.montecarlo import disperse_handover
    return disperse_handover(x[:, 0], 0, x.shape[0], seed, frac_r=size, frac_v=size, rate=size)


@pytest.mark.parametrize("w", WEIGHTS)
def test_cost_identity_and_float64_against_longdouble(w):
    """z0' P0 z0 is the cost of the closed loop (F + G L) from z0: the property that makes (L, P0) the solution of the recursion."""
    p, par, x, u, s, d = _data()
    L, P0 = tr.gains(d, p.K, *w)
    Ll, Pl = tr.gains(d, p.K, *w, dtype=np.longdouble)
    e = tr.cost_identity(d, p.K, L, P0, *w)
    eL = float(np.abs(L - Ll).max() / np.abs(Ll).max())
    eP = float(np.abs(P0 - Pl).max() / np.abs(Pl).max())
    print("weights %s: cost identity %.2e, float64 vs longdouble gains %.2e (max|L| %.1f), P0 %.2e" % (w, e, eL, np.abs(L).max(), eP))
    assert e < 1e-12
    assert np.abs(P0 - np.swapaxes(P0, 1, 2)).max() == 0.0
    assert np.all(np.linalg.eigvalsh(P0) > -1e-9 * np.abs(P0).max())
    if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps:
        assert eL < 1e-8 and eP < 1e-10 and tr.cost_identity(d, p.K, Ll, Pl, *w) < 1e-15


def test_zero_state_weights_give_zero_gains_exactly():
    p, par, x, u, s, d = _data()
    L, P0 = tr.gains(d, p.K, 0.0, 1.0, 0.0)
    assert not L.any() and not P0.any()


def test_zero_gains_closed_loop_is_the_shoot_flight():
    p, par, x, u, s, d = _data()
    from oracle import dynamics as od
    rep, xfly, ufly, _ = tr.fly(od, p, x, u, s, np.zeros((2, p.K, 3, 17)), None, 10, 0, par)
    ref, xref = fr.fly(od, p, x, u, s, 10, fr.SHOOT, par)
    assert np.array_equal(rep, ref) and np.array_equal(xfly, xref) and np.array_equal(ufly, u)


def test_flown_deviation_is_the_linear_prediction_to_second_order():
    """dx0 = eps xi: flown deviation (relative to the dx0 = 0 closed loop, which carries the plan's own defect) minus the linear
    prediction z_{k+1} = (F + G L) z_k scales with eps^2."""
    from oracle import dynamics as od
    p, par, x, u, s, d = _data()
    L, _ = tr.gains(d, p.K)
    A, Bm, Bp = tr.split_tiles(d, p.K)
    xi = np.random.default_rng(3).uniform(-1.0, 1.0, (2, 14))
    _, x00, _, _ = tr.fly(od, p, x, u, s, L, None, 10, 0, par)
    res = {}
    for eps in (1e-4, 1e-6):
        _, xf, _, _ = tr.fly(od, p, x, u, s, L, eps * xi, 10, 0, par)
        r = np.zeros(2)
        for b in range(2):
            z = np.concatenate([eps * xi[b], np.zeros(3)])
            for k in range(p.K):
                F, G = tr.fg(A[b, k], Bm[b, k], Bp[b, k])
                z = (F + G @ L[b, k]) @ z
                r[b] = max(r[b], np.abs(xf[b, k + 1] - x00[b, k + 1] - z[:14]).max())
        res[eps] = r
    ratio = res[1e-4] / res[1e-6]
    print("second-order residuals", res, "ratio", ratio)
    assert np.all(ratio >= 5e3) and np.all(ratio <= 2e4)


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 6])
def test_closed_loop_beats_open_loop(seed):
    from oracle import dynamics as od
    p, par, x, u, s, d = _data()
    L, _ = tr.gains(d, p.K)
    dx0 = _handover(x, seed)
    assert 1e-5 < np.abs(dx0).max() < 2e-3
    ro, _, _, _ = tr.fly(od, p, x, u, s, np.zeros_like(L), dx0, 10, 0, par)
    rc, _, _, _ = tr.fly(od, p, x, u, s, L, dx0, 10, 0, par)
    for n in ("MISS_R", "MISS_V"):
        print("seed %d %s open loop %s closed loop %s" % (seed, n, ro[:, fr.IDX[n]], rc[:, fr.IDX[n]]))
        assert np.all(rc[:, fr.IDX[n]] < ro[:, fr.IDX[n]])


def test_clamp_keeps_the_applied_thrust_in_its_bounds():
    from oracle import dynamics as od
    p, par, x, u, s, d = _data()
    L, _ = tr.gains(d, p.K)
    dx0 = _handover(x, 1)
    _, _, uf, cmd = tr.fly(od, p, x, u, s, L, dx0, 10, 0, par)
    _, _, uc, cmdc = tr.fly(od, p, x, u, s, L, dx0, 10, tr.CLAMP, par)
    t = np.linalg.norm(uc[:, 1:], axis=-1)
    assert t.min() >= p.Tmin * (1 - 4e-16) and t.max() <= p.Tmax * (1 + 4e-16)
    assert (np.abs(np.linalg.norm(uf[:, 1:], axis=-1) - cmd) < 1e-15).all()
    # the unclamped run leaves the bounds somewhere (else the test shows nothing) ...
    tf = np.linalg.norm(uf[:, 1:], axis=-1)
    assert tf.min() < p.Tmin or tf.max() > p.Tmax
    # ... and up to the first node that clamps the two runs are the same run
    for b in range(2):
        inside = (cmd[b] >= p.Tmin) & (cmd[b] <= p.Tmax)
        first = int(np.argmin(inside)) if not inside.all() else p.K
        assert np.array_equal(uc[b, :first + 1], uf[b, :first + 1])
    # a law that asks for nothing out of bounds is not touched: zero gains on a plan whose nodes hold the bounds to 1e-8
    un = u[:, 1:].reshape(-1, 3).copy()
    inb = (np.linalg.norm(un, axis=1) >= p.Tmin) & (np.linalg.norm(un, axis=1) <= p.Tmax)
    assert np.array_equal(tr.clamp_control(p, un.copy())[inb], un[inb])


def test_header_binding_and_julia_carry_the_same_symbols():
    from successiveconvexification_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "scvx.h")).read()
    jl = open(os.path.join(ROOT, "julia", "ScvxAMD.jl")).read()
    nargs = {"scvx_track_gains_f64": 9, "scvx_track_gains_f64_host": 9, "scvx_track_fly_f64": 13, "scvx_track_fly_f64_host": 13,
             "scvx_batch_track_gains": 6, "scvx_batch_track_fly": 10}
    for sym, n in nargs.items():
        m = re.search(r"\bint %s\(([^;]*?)\);" % sym, hdr, flags=re.S)
        assert m, sym
        assert len(m.group(1).split(",")) == n, sym
        assert len(_lib.SIGNATURES[sym][1]) == n, sym
        j = re.search(r"ccall\(\(:%s, LIB\), Cint,\s*\(([^)]*)\)" % sym, jl, flags=re.S)
        assert j, sym
        assert len([a for a in j.group(1).split(",") if a.strip()]) == n, sym
    mac = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define SCVX_TRACK_([A-Z_]+) (\d+)", hdr)}
    assert mac == {"CLAMP": 1} and _lib.TRACK_CLAMP == 1 == tr.CLAMP
    assert int(re.search(r"const TRACK_CLAMP = (\d+)", jl).group(1)) == 1
    assert "function track_gains(b::Batch" in jl and "function track(b::Batch" in jl
    # outside install!(): that function's body is pinned to the reference's by test_abi_harness.py
    inst = jl.index("function install!")
    assert jl.index("function track_gains(b::Batch") < inst or "track" not in jl[inst:jl.index("\nend", inst)]


def test_flight_report_keeps_its_constructor_and_gains_ufly():
    from successiveconvexification_amd.dynamics import FlightReport, _track_weights
    raw = np.zeros((2, 16))
    r = FlightReport(raw, None, "plan")
    assert r.mode == "plan" and r.xfly is None and r.ufly is None
    r = FlightReport(raw, np.zeros((2, 3, 14)), "track", np.ones((2, 3, 3)))
    assert r.mode == "track" and r.ufly.shape == (2, 3, 3)
    q, rr, qf = _track_weights(5, None, None, None)
    assert q.tolist() == [1.0] * 14 and rr.tolist() == [1.0] * 5 and qf.tolist() == [100.0] * 14
    q, rr, qf = _track_weights(3, np.arange(14.0), 2.0, 7)
    assert q.tolist() == list(range(14)) and rr.tolist() == [2.0] * 3 and qf.tolist() == [7.0] * 14
    with pytest.raises(ValueError):
        _track_weights(3, np.ones(13), None, None)


def test_disperse_handover():
    from successiveconvexification_amd.montecarlo import disperse_handover
    p, par, x, u, s, d = _data()
    x0 = np.tile(x[:1, 0], (12, 1))
    x0[:, 7:11] = np.random.default_rng(0).normal(size=(12, 4))
    x0[:, 7:11] /= np.linalg.norm(x0[:, 7:11], axis=1, keepdims=True)
    kw = dict(frac_r=1e-2, frac_v=2e-2, angle=0.05, rate=1e-3)
    whole = disperse_handover(x0, 0, 12, 99, **kw)
    assert whole.shape == (12, 14)
    assert np.array_equal(disperse_handover(x0[5:9], 5, 9, 99, **kw), whole[5:9])          # shards agree with the whole batch
    assert np.array_equal(disperse_handover(x0[0], 0, 3, 99, **kw)[0], whole[0])           # one x0 for all
    assert not np.array_equal(whole, disperse_handover(x0, 0, 12, 100, **kw))
    assert np.abs(np.linalg.norm((x0 + whole)[:, 7:11], axis=1) - 1.0).max() < 4e-16       # unit quaternion kept
    ang = 4 * np.arcsin(np.linalg.norm(whole[:, 7:11], axis=1) / 2)                        # |q (x) dq - q| = |dq - 1| = 2 sin(theta / 4)
    assert 0.0 < ang.max() <= 0.05 * (1 + 1e-12)                                           # a rotation by at most `angle`
    assert np.all(whole[:, 0] == 0.0)                                                      # mass untouched
    assert np.all(np.abs(whole[:, 1:4]) <= 1e-2 * np.abs(x0[:, 1:4])) and np.all(np.abs(whole[:, 4:7]) <= 2e-2 * np.abs(x0[:, 4:7]))
    assert whole[:, 1:7].any()
    assert np.abs(whole[:, 11:14]).max() <= 1e-3 and np.abs(whole[:, 11:14]).max() > 0
    assert not disperse_handover(x0, 0, 12, 99).any()                                      # zero arguments give zeros
    only_r = disperse_handover(x0, 0, 12, 99, frac_r=1e-2)
    assert np.array_equal(only_r[:, 1:4], whole[:, 1:4]) and not only_r[:, 4:].any()
